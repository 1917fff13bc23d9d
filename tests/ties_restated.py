"""The tie statement of csrc/k_ties.h, restated in plain Python - the yardstick of the tie tests.

Passing rows are those of tests/abundance_restated.py (the four cut-offs).  T is the highest bits among a read's passing rows.  A read
that abundance_restated does not assign to a subject in 0 .. nseq - 1 - no passing row, or a first-rule best row with a subject outside
that range - adds nothing.  The read's tied set is the distinct subjects in 0 .. nseq - 1 that have a passing row with bits == T (exact
float equality), k its size; a tied subject's representative row is its first such row in the read's order, and the first tied subject is
that of the first passing row with bits == T.

    candidates[s]   reads whose tied set contains s          unique[s]   reads whose tied set is {s}
    share[s]        in units of 2^-32: floor(2^32 / k) per read to every tied subject, the remainder 2^32 - k floor(2^32 / k) to the first
    ambiguous       reads with k > 1
    group_ambiguous reads whose tied set spans more than one group; group_unique[g]: reads whose whole tied set lies in g (with a map)
    any-depth       the representative row of EVERY tied subject adds 1 on sstart .. send (a span not inside its gene adds nothing)

Rows are the 8-tuples of coverage_restated.rows_from_m8 / rows_from_array: (query, subject, nmatch, alnlen, bits, loge, sstart, send).
Everything is built read by read with sets, dicts and Python integers: no difference array, no duplicate scan - nothing the kernel does."""
import numpy as np

import abundance_restated as R

ONE = 1 << 32


def tied_sets(rows, nseq, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """[(query, [(subject, sstart, send)] - the tied subjects in the order of their representative rows, the first tied subject first)]
    for every read that adds something, in the order the reads first appear."""
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge, a, b in rows:
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge, a, b))
    out = []
    for q, rs in by_read.items():
        passing = [r for r in rs if R.passes(r[1], r[2], r[3], r[4], min_ident, min_aln, min_bits, max_loge)]
        if not passing:
            continue
        top = max(r[3] for r in passing)
        tied = [r for r in passing if r[3] == top]
        if not 0 <= tied[0][0] < nseq:                        # (the row abundance_restated assigns the read by)
            continue
        rep = {}
        for r in tied:
            if 0 <= r[0] < nseq and r[0] not in rep:
                rep[r[0]] = (r[0], r[5], r[6])
        out.append((q, list(rep.values())))
    return out


def ties(rows, lengths, group_of=None, ngroups=0, **cut):
    """Every counter of the statement, and the any-depth with its three figures per gene.  lengths: every gene's residues.  group_of:
    one group number per gene, or None."""
    lengths = [int(x) for x in lengths]
    nseq = len(lengths)
    sets = tied_sets(rows, nseq, **cut)
    cand, uniq, share = [0] * nseq, [0] * nseq, [0] * nseq
    gu = [0] * ngroups
    amb = gamb = 0
    depth = [[0] * n for n in lengths]
    for q, members in sets:
        k = len(members)
        assert 1 <= k <= 500
        each = ONE // k
        for s, a, b in members:
            cand[s] += 1
            share[s] += each
            if 0 <= a <= b <= lengths[s] - 1:
                for p in range(a, b + 1):
                    depth[s][p] += 1
        share[members[0][0]] += ONE - k * each
        if k == 1:
            uniq[members[0][0]] += 1
        else:
            amb += 1
        if group_of is not None:
            groups = {int(group_of[s]) for s, _, _ in members}
            if len(groups) == 1:
                gu[groups.pop()] += 1
            else:
                gamb += 1
    return {"candidates": np.array(cand, np.int64), "unique": np.array(uniq, np.int64), "share": np.array(share, np.uint64),
            "group_unique": np.array(gu, np.int64), "ambiguous": amb, "group_ambiguous": gamb,
            "covered_any": np.array([sum(1 for v in d if v > 0) for d in depth], np.int64),
            "spanned_any": np.array([sum(d) for d in depth], np.int64),
            "max_depth_any": np.array([max(d) if d else 0 for d in depth], np.int64),
            "depth_any": np.array([v & 0xFFFFFFFF for d in depth for v in d], np.uint32),
            "k": [len(m) for _, m in sets], "sets": sets}


COUNTERS = ("candidates", "unique", "share", "group_unique")
ANY = ("covered_any", "spanned_any", "max_depth_any")


def same_counters(got, want):
    """whether an Engine.ties() result equals the restatement's"""
    return all(np.array_equal(got[k], want[k]) for k in COUNTERS) and got["ambiguous"] == want["ambiguous"] and got["group_ambiguous"] == want["group_ambiguous"]


def invariants(t, reads, assigned, group_of=None, depth=None):
    """the statement's invariants, as a list of those that do not hold.  t: a ties() result (the restatement's or the engine's); reads,
    assigned: the abundance counters of the same reads; depth: the depth of coverage_restated / the engine beside t["depth_any"]."""
    reads = np.asarray(reads, np.int64)
    bad = []
    if sum(int(v) for v in t["share"]) != assigned * ONE:
        bad.append("sum(share) = assigned x 2^32")
    if int(t["unique"].sum()) + t["ambiguous"] != assigned:
        bad.append("sum(unique) + ambiguous = assigned")
    if not ((t["unique"] <= reads) & (reads <= t["candidates"])).all():
        bad.append("unique <= reads <= candidates")
    if "k" in t and int(t["candidates"].sum()) != sum(t["k"]):
        bad.append("sum(candidates) = sum(k)")
    if group_of is not None:
        if int(t["group_unique"].sum()) + t["group_ambiguous"] != assigned:
            bad.append("sum(group_unique) + group_ambiguous = assigned")
        per = np.bincount(np.asarray(group_of), weights=t["unique"], minlength=len(t["group_unique"])).astype(np.int64)
        if not (t["group_unique"] >= per).all():
            bad.append("group_unique[g] >= sum of unique over g")
    if depth is not None and not (np.asarray(depth) <= t["depth_any"]).all():
        bad.append("depth <= any-depth")
    return bad
