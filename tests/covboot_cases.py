"""The cases of the coverage bootstrap's unit tests, built in one place: tests/test_gpu_covboot_units.py runs them on the device
(tests/emul/device_covboot.hip) and tests/test_covboot_host.py on the CPU (tests/emul/covboot.cpp: the rules of csrc/mc_covboot.h under
g++).  Both read the same files of sections (order_cases.write_sections) and are compared with tests/covboot_restated.py, whose answer is
computed once per case.

A case: name, lengths (every gene's residues), rows (an mc_row array), cuts (the row index behind each launch's last row), cut (the
cut-offs), B, seed, F (need = max(1, ceil(F x length)); None: no need is handed over), capacity (None: exactly the number of entries - the
list is full to its last slot and nothing is dropped), launch (False: the launches are handed no list) and idmap (None, or (perm, base): a
row's query is a position, the read's id base + perm[query])."""
import numpy as np

import abundance_restated as R
import coverage_restated as V
import covboot_restated as CR
import curve_cases as cc
import geneboot_cases as gc
import geneboot_restated as GR
import tieboot_cases as tbc

BS = gc.BS                              # (1, 63, 64, 65, 257, 4096)
W = CR.WINDOW


def _case(name, lengths, spec, B, cuts=None, cut=None, seed=20240917, F=0.5, capacity=None, launch=True, idmap=None):
    rows = spec if isinstance(spec, np.ndarray) else cc.rows_of(spec)
    return {"name": name, "lengths": [int(x) for x in lengths], "nseq": len(lengths), "rows": rows, "cuts": list(cuts) if cuts else [len(rows)], "cut": cut or {}, "B": int(B),
            "seed": int(seed), "F": F, "capacity": capacity, "launch": launch, "idmap": idmap}


SPAN_LENGTHS = [200, 64, 130, 1, 300, 70, 9]


def _spans():
    """gene 0 (200 residues): a single residue, a span from 0, one to len - 1, two that abut (e + 1 == s'), one that overlaps them, one that
    nests, two that are identical, one crossing word 64 and one crossing word 128; gene 1 (64): the whole gene; gene 2 (130): send == len (the
    empty entry), sstart > send (empty too) and a valid span; gene 3 (1 residue); gene 4: no read; gene 5: ONE read; gene 6, the last: no read.
    Some reads carry a second, weaker row of another gene; read 9's first row fails min_ident 60 when the cut-offs are set."""
    return [(0, 0, 5, 5), (1, 0, 0, 9), (2, 0, 190, 199), (3, 0, 20, 29), (3, 4, 0, 299, 30.0), (4, 0, 30, 39), (5, 0, 35, 50), (6, 0, 40, 45), (7, 0, 40, 45), (8, 0, 60, 70),
            (9, 4, 0, 100, 80.0, 10, 30), (9, 0, 120, 140, 40.0), (10, 1, 0, 63), (11, 2, 100, 130), (12, 2, 10, 20), (12, 6, 0, 8, 20.0), (13, 2, 30, 25), (14, 3, 0, 0), (15, 5, 3, 66)]


def _window():
    """gene 1 is MC_CB_WINDOW + 100 residues long: spans on both sides of the window's edge, one across it, one ending on its last word, one
    starting on the next window's first word, one to len - 1, one over the whole gene's middle; genes 0 and 2 are short"""
    L = W + 100
    return [50, L, 64], [(0, 0, 3, 40), (1, 1, 0, 10), (2, 1, W - 50, W - 10), (3, 1, W - 5, W + 5), (4, 1, W - 20, W - 1), (5, 1, W, W + 30), (6, 1, W + 90, W + 99),
                         (7, 1, W - 300, W + 60), (8, 2, 10, 63), (9, 1, W + 40, W + 100), (11, 1, 1000, 1100)]


def _one_gene():
    """gene 1 holds 200 entries: four reads at each of 50 places ten residues apart, every span twelve residues (it overlaps the next
    place's by two; the last ends at len - 1).  A place is absent from a replicate with probability 0.37^4: about four replicates in ten
    cover all 500 residues, and need is 500"""
    return [30, 500, 30], [(7 * k, 1, (k % 50) * 10, min((k % 50) * 10 + 11, 499)) for k in range(200)]


def _workgroups():
    """tieboot_cases._workgroups' layout - more than 256 reads over four workgroups, a read beginning at thread 255, a workgroup that
    assigns nothing - with spans that differ from read to read; the genes are 40 residues long"""
    nseq, spec = tbc._workgroups()
    return [40] * nseq, [(r[0], r[1], r[0] % 30, r[0] % 30 + 2 + r[0] % 8) + tuple(r[4:]) for r in spec]


def cases():
    out = []
    for B in BS:
        out.append(_case("b%d" % B, SPAN_LENGTHS, _spans(), B, cut=dict(min_ident=60) if B >= 64 else None, F=0.25))
    lengths, spec = _window()
    out.append(_case("window", lengths, spec, 65))
    lengths, spec = _one_gene()
    out.append(_case("one_gene", lengths, spec, 64, F=1.0))
    lengths, spec = _workgroups()
    out.append(_case("workgroups", lengths, spec, 65))
    rows = cc.rows_of(_spans())
    cuts = [int(np.searchsorted(rows["query"], 5)), int(np.searchsorted(rows["query"], 10)), len(rows)]
    out.append(_case("launches", SPAN_LENGTHS, rows, 63, cuts=cuts))
    out.append(_case("no_need", SPAN_LENGTHS, _spans(), 64, F=None))
    # read ids up to 2^31 - 1
    top = 2 ** 31 - 1
    out.append(_case("big_ids", [100, 80], [(5, 0, 0, 30), (top - 2, 1, 10, 40), (top - 1, 0, 20, 60), (top, 1, 30, 79)], 64))
    # capacity: one entry short; the switch off (the launch is handed no list and must leave list memory as it was)
    short = _case("short", SPAN_LENGTHS, _spans(), 64)
    short["capacity"] = len(expect(short)["q"]) - 1
    out.append(short)
    out.append(_case("off", SPAN_LENGTHS, _spans(), 64, launch=False))
    # a class run's ids: the rows carry positions 0 .. 15, the ids are base + perm[position]
    perm = np.random.default_rng(5).permutation(40).astype(np.uint32)
    out.append(_case("idmap", SPAN_LENGTHS, _spans(), 64, idmap=(perm, 123456)))
    return out


_EXPECT = {}


def offsets(c):
    return np.r_[0, np.cumsum(c["lengths"])].astype(np.uint32)


def expect(c):
    """the restatement's answer of a case, computed once and shared: q, g, s, e (the entries), cov [nseq, B], stats [nseq, 6], need and det
    (None without F), counts: the gene bootstrap's replicate counts of the same rows; ab, cv: abundance_restated's and coverage_restated's;
    diff: the difference array k_abundance_cov leaves (uint32, every gene's len + 1 slots)"""
    if c["name"] not in _EXPECT:
        rows8, rows6, nseq, lengths = V.rows_from_array(c["rows"]), R.rows_from_array(c["rows"]), c["nseq"], c["lengths"]
        ids = None if c["idmap"] is None else (lambda pos, perm=c["idmap"][0], base=c["idmap"][1]: base + int(perm[pos]))
        q, g, s, e = CR.entries(rows8, lengths, ids=ids, **c["cut"])
        cov = CR.cover(q, g, s, e, lengths, c["B"], c["seed"])
        need = None if c["F"] is None else CR.need(lengths, c["F"])
        cv = V.coverage(rows8, lengths, **c["cut"])
        diff = np.zeros(sum(lengths) + nseq, np.int64)
        first = np.r_[0, np.cumsum(np.asarray(lengths) + 1)]
        for sub, a, b in cv["best"]:
            if 0 <= a <= b <= lengths[sub] - 1:
                diff[first[sub] + a] += 1
                diff[first[sub] + b + 1] -= 1
        _EXPECT[c["name"]] = {"q": q, "g": g, "s": s, "e": e, "cov": cov, "stats": CR.stats(cov), "need": need, "det": None if need is None else CR.detected(cov, need),
                              "counts": GR.counts(q, g, nseq, c["B"], c["seed"]), "cv": cv, "diff": (diff & 0xFFFFFFFF).astype(np.uint32),
                              "ab": R.abundance(rows6, max(nseq, int(c["rows"]["subject"].max()) + 1), **c["cut"])}
    return _EXPECT[c["name"]]


def capacity(c):
    return len(expect(c)["q"]) if c["capacity"] is None else c["capacity"]


def sections_in(c):
    pars = np.zeros(1, cc.PARS)
    cut = c["cut"]
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    meta = np.int32([c["nseq"], c["B"], capacity(c), 1 if c["launch"] else 0])
    perm, base = c["idmap"] if c["idmap"] is not None else (np.zeros(0, np.uint32), 0)
    need = np.zeros(0, np.uint32) if c["F"] is None else CR.need(c["lengths"], c["F"]).astype(np.uint32)
    return [pars, meta, offsets(c), c["rows"], np.array(c["cuts"], np.uint32), np.array([c["seed"]], np.uint64), np.asarray(perm, np.uint32), np.array([base], np.int64), need]


def entry_set(q, g, s, e):
    """the entries as a sorted list of (q, gene, s, e): a multiset"""
    return sorted(zip(*(np.asarray(x).tolist() for x in (q, g, s, e))))


def compare(c, cov, stats, det):
    """cov [nseq x B], stats [nseq x 6] and det [nseq] (or None) of a run of case c - from the device or the CPU build - against the
    restatement: the integers exactly, the doubles bit for bit; then the statement's invariants"""
    x = expect(c)
    cov = np.asarray(cov).astype(np.int64).reshape(c["nseq"], c["B"])
    stats = np.asarray(stats, np.float64).reshape(c["nseq"], 6)
    assert np.array_equal(cov, x["cov"]), "covered residues: first difference at %s" % (np.argwhere(cov != x["cov"])[:1].tolist(),)
    assert GR.same_bits(stats, x["stats"]), "the six doubles: first difference at %s" % (np.argwhere(stats.view(np.uint64) != x["stats"].view(np.uint64))[:1].tolist(),)
    if x["det"] is not None:
        assert np.array_equal(np.asarray(det).astype(np.int64), x["det"]), "detected: %s against %s" % (np.asarray(det).tolist(), x["det"].tolist())
    invariants(c, cov, x["cv"]["covered"], x["counts"])
    return x


def invariants(c, cov, covered, counts):
    """the statement's three invariants: cov[b][g] <= covered[g] of the whole sample; cov > 0 implies the gene bootstrap's count > 0, and the
    converse for a gene all of whose spans are valid; a gene with one read has cov in {0, e - s + 1}.  cov: [nseq, B]; covered: [nseq];
    counts: the gene bootstrap's [nseq, B] under the same seed"""
    x = expect(c)
    cov, counts = np.asarray(cov, np.int64), np.asarray(counts, np.int64)
    assert (cov <= np.asarray(covered, np.int64)[:, None]).all(), "a replicate covers more than the sample"
    assert (counts[cov > 0] > 0).all(), "covered residues in a replicate without a read of the gene"
    for gene in range(c["nseq"]):
        mine = x["g"] == gene
        if mine.any() and (x["s"][mine] <= x["e"][mine]).all():
            assert np.array_equal(cov[gene] > 0, counts[gene] > 0), "gene %d: every span is valid, and a replicate with a read covers nothing" % gene
        if mine.sum() == 1:
            i = int(np.flatnonzero(mine)[0])
            width = int(x["e"][i]) - int(x["s"][i]) + 1 if x["s"][i] <= x["e"][i] else 0
            assert set(cov[gene].tolist()) <= {0, width}, "gene %d has one read and a replicate covers neither 0 nor %d residues" % (gene, width)
