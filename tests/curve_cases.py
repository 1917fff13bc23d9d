"""The cases of the curve's unit tests, built in one place: tests/test_gpu_curve_units.py runs them on the device (tests/emul/device_curve.hip)
and tests/test_curve_host.py on the CPU (tests/emul/curve.cpp: the rules of csrc/mc_curve.h under g++, plain and sanitized).  Both read the
same files of sections (order_cases.write_sections) and are compared with tests/curve_restated.py, whose answer is computed once per case.

A case: name, lengths (every gene's residues), rows (an mc_row array), points, cuts (the row index behind each launch's last row) and cut
(the cut-offs).  Every case runs with coverage on and once more with it off."""
import numpy as np

import abundance_restated as R
import coverage_restated as V
import curve_restated as CR
from microbecensus_amd import microbe_census
from microbecensus_amd._native import ROW_DTYPE

PARS = np.dtype([("min_ident", "<i4"), ("min_aln", "<i4"), ("min_bits", "<f8"), ("max_loge", "<f8")])   # McAbundPars
assert ROW_DTYPE.itemsize == 72 and PARS.itemsize == 24


def rows_of(spec):
    """mc_row array of (query, subject, sstart, send[, bits[, nmatch, alnlen]]): bits 50, 27 of 30 identical by default"""
    arr = np.zeros(len(spec), ROW_DTYPE)
    for i, r in enumerate(spec):
        q, s, a, b = r[:4]
        bits = r[4] if len(r) > 4 else 50.0
        nmatch, alnlen = r[5:7] if len(r) > 5 else (27, 30)
        arr[i] = (q, s, nmatch * 100.0 / alnlen, alnlen, alnlen - nmatch, 0, 1, 90, a, b, -5.0, bits, 100, nmatch)
    return arr


def _case(name, lengths, spec, points, cuts=None, cut=None):
    rows = spec if isinstance(spec, np.ndarray) else rows_of(spec)
    return {"name": name, "lengths": [int(x) for x in lengths], "rows": rows, "points": [int(p) for p in points], "cuts": list(cuts) if cuts else [len(rows)],
            "cut": cut or {}}


LENGTHS = [1, 63, 64, 65, 129, 2047]


def _lengths_case():
    """genes of 1, 63, 64, 65, 129 and 2,047 residues with genes without reads between them; on every gene the spans [0, 0], [len - 1,
    len - 1] and [0, len - 1] - each from a read of another bin, the widest span last: covered grows point by point.  A non-zero first id."""
    lengths, hit = [], []
    for n in LENGTHS:
        hit.append(len(lengths))
        lengths += [n, 70, 5]
    spec, q = [], 7000
    for g, n in zip(hit, LENGTHS):
        for a, b in ((0, 0), (n - 1, n - 1), (0, n - 1)):
            spec.append((q, g, a, b))
            q += 3                                                # (reads without rows between them)
    return _case("lengths", lengths, spec, [7001 + 3 * k for k in range(18)]), hit


def _straddle_case():
    """a read whose rows straddle a 256-thread workgroup boundary with its best row behind it; a read whose rows end exactly at nrows; a
    top row that fails a cut-off, a tie on bits, a read with no passing row; subjects not below nseq"""
    lengths = [100, 300, 64, 2047]
    spec = [(q, q % 3, q % 30, q % 30 + 30) for q in range(250)]
    spec += [(250, 0, 0, 40, 40.0 + k) for k in range(5)] + [(250, 3, 100, 2046, 90.0)] + [(250, 1, 5, 9, 50.0) for _ in range(4)]   # rows 250 .. 259: the best is row 255
    spec += [(251, 2, 0, 63, 80.0, 10, 30), (251, 1, 290, 299, 40.0)]                               # the top row fails min_ident 60
    spec += [(252, 1, 0, 0, 60.0), (252, 2, 1, 1, 60.0)]                                            # a tie: the first
    spec += [(253, 0, 0, 99, 70.0, 5, 30)]                                                          # no passing row under the cut-offs
    spec += [(254, 4, 0, 10, 70.0), (255, 32767, 0, 10, 70.0)]                                      # subjects not below nseq
    spec += [(q, 3, (q * 37) % 2000, (q * 37) % 2000 + 46) for q in range(256, 256 + 300)]
    spec += [(600, 1, 7, 8, 10.0), (600, 1, 100, 299, 20.0), (600, 0, 50, 60, 15.0)]                # the last read: its rows end at nrows
    rows = rows_of(spec)
    assert rows["query"][255] == rows["query"][256] == 250 and rows["bits"][255] == 90.0 and len(rows) % 256 not in (0, 1)
    return rows, lengths


def cases():
    out = []
    # K = 1: ids n - 1 and n, and reads behind the point: beyond > 0, nothing lost from the bin sums
    out.append(_case("k1", [40, 9], [(3, 0, 0, 9), (4, 0, 5, 20), (5, 1, 0, 8), (6, 0, 30, 39), (9, 1, 2, 3)], [5]))
    # K = 64, a non-zero first id: for every point one read at n_k - 1 and one at n_k; the last of them lies behind the last point
    pts = [1000 + 5 * (k + 1) for k in range(64)]
    spec = []
    for k, n in enumerate(pts):
        spec += [(n - 1, k % 5, (3 * k) % 40, (3 * k) % 40 + 20), (n, (k + 1) % 5, k % 7, k % 7 + 25)]
    out.append(_case("k64", [130, 64, 70, 65, 200], spec, pts))
    # repeated points: sampled_reads 3, K 5
    pts = microbe_census.curve_points(3, 5)
    assert pts == [1, 2, 2, 3, 3]
    out.append(_case("repeats", [30, 20, 10], [(0, 0, 0, 9), (1, 1, 5, 19), (2, 0, 5, 29)], pts))
    lc, _ = _lengths_case()
    out.append(lc)
    for nseq in (1, 3, 4, 5):
        lengths = [130, 64, 7, 65, 200][:nseq]
        spec = sorted((3 * g + k, g, k, min(lengths[g] - 1, 20 * k + 5)) for g in range(nseq) for k in range(3))
        out.append(_case("genes%d" % nseq, lengths, spec, [2, 7, 11, 40]))
    rows, lengths = _straddle_case()
    for cut in ({}, dict(min_ident=60, min_aln=25)):
        out.append(_case("straddle_%d" % len(cut), lengths, rows, [100, 251, 252, 400, 601], cut=cut))
    # one residue range covered by two launches, the higher ids first and the lower ids first: the same first either way
    lo = [(10, 0, 5, 30), (11, 1, 0, 19), (12, 0, 20, 49)]
    hi = [(20, 0, 0, 40), (21, 1, 10, 19), (22, 0, 45, 49)]
    out.append(_case("hi_first", [50, 20], hi + lo, [11, 15, 21, 30], cuts=[3, 6]))
    out.append(_case("lo_first", [50, 20], lo + hi, [11, 15, 21, 30], cuts=[3, 6]))
    return out


def sections_in(c, coverage):
    pars = np.zeros(1, PARS)
    cut = c["cut"]
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    off = np.zeros(len(c["lengths"]) + 1, np.uint32)
    off[1:] = np.cumsum(c["lengths"])
    return [pars, off, c["rows"], np.array(c["points"], np.uint64), np.array(c["cuts"], np.uint32), np.int32([1 if coverage else 0])]


_EXPECT = {}


def expect(c, coverage):
    """the restatements' answer of a case, computed once and shared: (curve, abundance, coverage's covered)"""
    key = (c["name"], bool(coverage))
    if key not in _EXPECT:
        rows, nseq = c["rows"], len(c["lengths"])
        cv = CR.curve(V.rows_from_array(rows), c["lengths"], c["points"], coverage=coverage, **c["cut"])
        ab = R.abundance(R.rows_from_array(rows), max(nseq, int(rows["subject"].max()) + 1), **c["cut"])
        cov = V.coverage(V.rows_from_array(rows), c["lengths"], **c["cut"])
        _EXPECT[key] = (cv, ab, cov)
    return _EXPECT[key]


def compare(c, coverage, bins, first, out):
    """the bin table, first and the scan's output of a run of case c - from the device or from the CPU build - against the restatement,
    exactly; then the statement's invariants and the case's own conditions"""
    cv, ab, cov = expect(c, coverage)
    K, nseq = len(c["points"]), len(c["lengths"])
    bins = np.asarray(bins, np.uint64).reshape(K + 1, nseq, 2)
    assert np.array_equal(bins[:, :, 0], cv["bin_reads"].astype(np.uint64)) and np.array_equal(bins[:, :, 1], cv["bin_aligned"].astype(np.uint64)), "the bin table"
    want_first = CR.first_flat(cv)
    assert np.array_equal(first, want_first), "first: the first difference at residue %d" % int(np.flatnonzero(np.asarray(first) != want_first)[0])
    if not coverage:
        assert (want_first == 0xFFFFFFFF).all()
    out = np.asarray(out, np.uint64)
    fig, tot = out[:3 * K * nseq].reshape(K, nseq, 3), out[3 * K * nseq:]
    assert len(tot) == K + 1
    for j, name in enumerate(("reads", "aligned", "covered")):
        assert np.array_equal(fig[:, :, j], cv[name].astype(np.uint64)), name
    assert np.array_equal(tot[:K], cv["assigned"].astype(np.uint64)) and int(tot[K]) == cv["beyond"], "assigned_k / beyond"
    assert CR.invariants(cv, ab["reads"][:nseq], ab["aligned"][:nseq], cov["covered"], coverage) == []
    assert int(cv["bin_reads"].sum()) == len(cv["best"]) == int(cv["assigned"][-1]) + cv["beyond"], "nothing lost from the bin sums"
    return cv
