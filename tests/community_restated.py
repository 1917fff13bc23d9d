"""The community library's formula (csrc/mc_simlib.h: the member table, the draw, the walk) restated in numpy, vectorised over reads:
where every read is placed (member, contig, start) and the bytes of any library kind.  Shared by the CPU and GPU tests of
mc_community_*; written from the header's comment, with Python integers for the table, independent of the C++ code."""
import numpy as np

import simlib_restated as sr


def member_table(off, mfirst, copies, span):
    """(vstart per contig, counted from 0 inside every member; total per member; cum of M + 1 Python integers)."""
    off = [int(x) for x in off]
    vstart, total, cum = [0] * (len(off) - 1), [], [0]
    for m in range(len(copies)):
        t = 0
        for c in range(int(mfirst[m]), int(mfirst[m + 1])):
            vstart[c] = t
            t += max(0, off[c + 1] - off[c] - span + 1)
        total.append(t)
        cum.append(cum[-1] + int(copies[m]) * t)
    return vstart, total, cum


def place(off, mfirst, copies, span, x):
    """x: uint64 array, mix(key + frag) of every read.  (member, contig, start) as int64 arrays."""
    vstart, total, cum = member_table(off, mfirst, copies, span)
    assert 0 < cum[-1] < 1 << 62
    off = np.asarray(off, dtype=np.int64)
    mfirst = np.asarray(mfirst, dtype=np.int64)
    u = np.asarray(x, dtype=np.uint64) % np.uint64(cum[-1])
    m = np.searchsorted(np.array(cum, dtype=np.uint64), u, side="right").astype(np.int64) - 1
    v = ((u - np.array(cum, dtype=np.uint64)[m]) % np.array(total, dtype=np.uint64)[m]).astype(np.int64)
    vs = np.array(vstart, dtype=np.int64)
    width = np.maximum(0, np.diff(off) - span + 1)
    c = np.empty(len(u), dtype=np.int64)
    for k in np.unique(m):                         # member by member: the contig whose starts hold v
        sel = m == k
        lo, hi = int(mfirst[k]), int(mfirst[k + 1])
        ends = vs[lo:hi] + width[lo:hi]            # contig lo + j holds v in [vs, ends)
        c[sel] = lo + np.searchsorted(ends, v[sel], side="right")
    assert np.all(v >= vs[c]) and np.all(v < vs[c] + width[c])
    return m, c, off[c] + v - vs[c]


def simulate(bases, off, mfirst, copies, L, first, n, seed, lib, error_model=None, error_rate=None, paired_end=False, insert=None, places_only=False):
    """Rows [first, first + n) of the community library (seed, lib) of the given kind: (reads uint8 (n, L), member, contig, start)."""
    off = np.asarray(off, dtype=np.int64)
    span = insert if paired_end else L
    key = sr.mix64(seed ^ sr.mix64(lib))
    ekey = sr.mix64(key ^ sr.EKEY)
    i = np.arange(first, first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        frag = i >> np.uint64(1) if paired_end else i
        x = sr.mix64_np(np.uint64(key) + frag)
        r = sr.mix64_np(np.uint64(ekey) + i)
    m, c, s = place(off, mfirst, copies, span, x)
    if places_only:
        return None, m, c, s
    bases = np.asarray(bases, dtype=np.uint8)
    cs, ce = off[c], off[c + 1]
    rev = (i & np.uint64(1)).astype(bool) if paired_end else np.zeros(n, dtype=bool)
    step = np.where(rev, -1, 1)
    p = np.where(rev, s + span - 1, s)
    thr = np.array(sr.thresholds(error_model, error_rate), dtype=np.uint64)
    errors = error_model is not None
    out = np.zeros((n, L), dtype=np.uint8)
    o = np.zeros(n, dtype=np.int64)
    j = 0
    while True:                                    # the walk of mc_simlib.h, a consumed base per turn over the reads still walking
        a = np.nonzero(o < L)[0]
        if len(a) == 0:
            break
        pa = p[a]
        assert np.all(pa >= cs[a]) and np.all(pa < ce[a]), "a walk left its contig"
        b = bases[pa]
        b = np.where(rev[a], sr.COMP[b], b)
        e = np.zeros(len(a), dtype=np.int64)
        x = np.zeros(len(a), dtype=np.uint8)
        if errors:
            with np.errstate(over="ignore"):
                d = sr.mix64_np(r[a] + np.uint64((j * sr.GAMMA) & sr.MASK))
            err = (d >> np.uint64(32)) < thr[min(j, sr.NTHR - 1)]
            kind = ((d >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
            x = sr.ACGT[(d & np.uint64(3)).astype(np.int64)]
            e = np.where(err, np.where(kind < sr.SUB, 1, np.where(kind < sr.INS, 2, 3)), 0)
            left = np.where(step[a] > 0, ce[a] - 1 - pa, pa - cs[a])
            e = np.where((e == 3) & (left < L - o[a]), 4, e)
        keep = (e == 0) | (e == 4)
        out[a[keep], o[a[keep]]] = b[keep]
        sub = e == 1
        out[a[sub], o[a[sub]]] = x[sub]
        ins = e == 2
        out[a[ins], o[a[ins]]] = x[ins]
        o[a[keep | sub | ins]] += 1
        ins2 = ins & (o[a] < L)
        out[a[ins2], o[a[ins2]]] = b[ins2]
        o[a[ins2]] += 1
        p[a] += step[a]
        j += 1
    return out, m, c, s


def join_members(members):
    """[(bases, contig_off)] -> (bases, contig_off, mfirst) of the members one after another."""
    offs, first, at = [np.zeros(1, np.int64)], [0], 0
    for b, off in members:
        off = np.asarray(off, dtype=np.int64)
        offs.append(off[1:] + at)
        at += int(off[-1])
        first.append(first[-1] + len(off) - 1)
    return np.concatenate([np.asarray(b, np.uint8) for b, _ in members]), np.concatenate(offs), np.array(first, dtype=np.int32)


def fixture_members(which=None):
    """[(name, bases, contig_off)] of the genomes of tests/golden/genomes/genomes30.npz (all 30, or the indices in `which`)."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genomes", "genomes30.npz"))
    packed, off = d["packed"], d["contig_off"]
    codes = np.stack([(packed >> (2 * k)) & 3 for k in range(4)], axis=1).reshape(-1)[: off[-1]]
    allb = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    allb[d["exc_pos"]] = d["exc_chr"]
    out = []
    for g in (range(int(d["genome_of"].max()) + 1) if which is None else which):
        idx = np.nonzero(d["genome_of"] == g)[0]
        lo, hi = off[idx[0]], off[idx[-1] + 1]
        out.append(("g%02d" % g, allb[lo:hi].copy(), (off[idx[0]: idx[-1] + 2] - lo).astype(np.int64)))
    return out
