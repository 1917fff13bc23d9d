"""The coverage kernels (csrc/k_coverage.h) on synthetic rows at the smallest shapes that can go wrong: k_abundance_cov (the counting
kernel that also marks) and k_coverage_scan - and, the small cases once more with coverage off, k_abundance (csrc/k_abundance.h) -,
launched by tests/emul/device_coverage.hip through the library's launch function (csrc/mc_abund.h) - test_gpu_order_units.py's
idiom: the harness includes the library's headers and is built here with the library's flags, every case is one child process under a
time limit of its own, and every comparison is exact, against tests/coverage_restated.py (covered, spanned, max_depth and the depth of
every residue) and tests/abundance_restated.py (the reads / aligned / assigned counters of the same launch).

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
three unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import abundance_restated as R
import coverage_restated as V
import order_cases as oc
from microbecensus_amd._native import ROW_DTYPE

pytestmark = pytest.mark.gpu

PARS = np.dtype([("min_ident", "<i4"), ("min_aln", "<i4"), ("min_bits", "<f8"), ("max_loge", "<f8")])   # McAbundPars
assert ROW_DTYPE.itemsize == 72 and PARS.itemsize == 24


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_coverage", tmp_path_factory)


def _run(exe, case, arrays, tmp, limit):
    return oc.run_child(exe, case, arrays, tmp, limit, "run")


def _rows(spec):
    """mc_row array of (query, subject, sstart, send[, bits[, nmatch, alnlen]]): bits 50, 27 of 30 identical by default"""
    arr = np.zeros(len(spec), ROW_DTYPE)
    for i, r in enumerate(spec):
        q, s, a, b = r[:4]
        bits = r[4] if len(r) > 4 else 50.0
        nmatch, alnlen = r[5:7] if len(r) > 5 else (27, 30)
        arr[i] = (q, s, nmatch * 100.0 / alnlen, alnlen, alnlen - nmatch, 0, 1, 90, a, b, -5.0, bits, 100, nmatch)
    return arr


def _padding_untouched(out):
    """nothing was written behind any array: tab's and the difference array's padding still zero, the figures' and the depth's still 0xFF"""
    assert len(out) == 11 and len(out[8]) == len(out[9]) == 64
    assert not np.frombuffer(out[5], "<u8").any() and not np.frombuffer(out[10], "<u4").any(), "a write behind tab or the difference array"
    assert all(np.all(np.frombuffer(out[k], "u1") == 0xFF) for k in (6, 7, 8, 9)), "a write behind the figures or the depth"


def _counters(tab, ab, nseq, assigned):
    assert np.array_equal(tab[0:2 * nseq:2], ab["reads"][:nseq].astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == int(ab["reads"][:nseq].sum()) == assigned and int(tab[2 * nseq + 1]) == 0, "assigned"


def _check(exe, case, tmp, lengths, rows, cut=None, without=True):
    """Runs the case and compares everything with the restatements; returns the restated coverage (for the case's own conditions).
    without: the case once more with the harness's coverage switch off - k_abundance instead of k_abundance_cov through the same launch
    function: the counters are abundance_restated's, the padding is untouched and the difference array, which no kernel was handed,
    holds nothing."""
    cut = cut or {}
    pars = np.zeros(1, PARS)
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    off = np.zeros(len(lengths) + 1, np.uint32)
    off[1:] = np.cumsum(lengths)
    out = _run(exe, case, [pars, off, rows, np.int32([1])], tmp, 60)
    nseq = len(lengths)
    tab, fig, depth, fig2, diff = (np.frombuffer(out[0], "<u8"), np.frombuffer(out[1], "<u8").reshape(nseq, 3), np.frombuffer(out[2], "<u4"),
                                   np.frombuffer(out[3], "<u8").reshape(nseq, 3), np.frombuffer(out[4], "<u4"))
    _padding_untouched(out)
    inside = rows[(rows["subject"] >= 0) & (rows["subject"] < nseq)]     # (the restatements index by subject: what the kernel ignores is left out below)
    want = V.coverage(V.rows_from_array(rows), lengths, **cut)
    ab = R.abundance([r for r in R.rows_from_array(rows)], nseq + int(max(0, rows["subject"].max() - nseq + 1)) if len(rows) else nseq, **cut)
    print("%s: %d genes, %d rows (%d with a subject of the database), %d best rows, covered %d, spanned %d, max depth %d" % (
        case, nseq, len(rows), len(inside), len(want["best"]), int(want["covered"].sum()), int(want["spanned"].sum()), int(want["max_depth"].max())))
    _counters(tab, ab, nseq, len(want["best"]))
    assert np.array_equal(depth, want["depth"]), "depth: first difference at residue %d" % int(np.flatnonzero(depth != want["depth"])[0])
    for k, name in enumerate(("covered", "spanned", "max_depth")):
        assert np.array_equal(fig[:, k], want[name].astype(np.uint64)), name
    assert np.array_equal(fig, fig2), "the scan without the depth buffer"
    # the layout: every gene's slots sum to zero (its +1s and -1s), and the sentinel holds what ended at len - 1
    first = off[:-1].astype(np.int64) + np.arange(nseq)
    ends_at_last = np.bincount([s for s, a, b in want["best"] if b == lengths[s] - 1], minlength=nseq)
    assert np.array_equal(diff[first + np.asarray(lengths)], (-ends_at_last).astype(np.uint32)), "sentinels"
    assert V.invariants(want, ab["reads"][:nseq], lengths) == []
    if without:
        out = _run(exe, case + "_without", [pars, off, rows, np.int32([0])], tmp, 60)
        _padding_untouched(out)
        _counters(np.frombuffer(out[0], "<u8"), ab, nseq, len(want["best"]))
        assert len(out[1]) == len(out[2]) == len(out[3]) == 0 and len(out[4]) == 4 * (sum(lengths) + nseq) and not np.frombuffer(out[4], "<u4").any(), "the difference array"
    return want


LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 2047]


def test_gene_lengths_and_spans(harness, tmp_path):
    """Genes of 1, 2, 63, 64, 65, 127, 128, 129 and 2,047 residues in one database - with genes without reads lying between them (the skip
    path) - and on every gene the spans [0, 0], [0, len - 1], [len - 1, len - 1], and where they fit [10, 63] (its -1 lands in the next
    chunk's first lane), [63, 64] and one span over all 2,047 residues.  Time limit 60 s."""
    lengths, hit = [], []
    for n in LENGTHS:
        hit.append(len(lengths))
        lengths += [n, 70, 5]                                     # two genes without reads behind every gene with reads
    spec, q = [], 0
    for g, n in zip(hit, LENGTHS):
        spans = [(0, 0), (0, n - 1), (n - 1, n - 1)] + ([(10, 63)] if n >= 64 else []) + ([(63, 64)] if n >= 65 else []) + ([(0, 2046)] if n == 2047 else [])
        for a, b in spans:
            spec.append((q, g, a, b))
            q += 3                                                # (reads without rows between them)
    want = _check(harness, "lengths", tmp_path, lengths, _rows(spec))
    assert (want["covered"] > 0).sum() == len(LENGTHS) and want["covered"][hit].tolist() == LENGTHS and int(want["max_depth"][hit[-1]]) == 4


@pytest.mark.parametrize("nseq", [1, 3, 4, 5])
def test_gene_counts(harness, tmp_path, nseq):
    """1, 3, 4 and 5 genes: not a multiple of the four waves of a workgroup.  Every gene has reads.  Time limit 60 s."""
    lengths = [130, 64, 7, 65, 200][:nseq]
    spec = [(3 * g + k, g, k, min(lengths[g] - 1, 20 * k + 5)) for g in range(nseq) for k in range(3)]
    want = _check(harness, "genes%d" % nseq, tmp_path, lengths, _rows(sorted(spec)))
    assert (want["covered"] > 0).all()


@pytest.mark.parametrize("nrows", [1, 256, 257])
def test_row_counts(harness, tmp_path, nrows):
    """1, 256 and 257 rows, one read each: one thread, exactly one workgroup, one row into the second.  Time limit 60 s."""
    lengths = [40, 64, 9]
    want = _check(harness, "rows%d" % nrows, tmp_path, lengths, _rows([(q, q % 3, q % 9, q % 9) for q in range(nrows)]))
    assert len(want["best"]) == nrows and int(want["spanned"].sum()) == nrows


def test_sentinel_isolation(harness, tmp_path):
    """A gene whose only span ends at len - 1, directly followed by a gene whose only span starts at 0 - and the same at a chunk's
    end (64 residues).  Time limit 60 s."""
    lengths = [40, 30, 64, 64, 9]
    want = _check(harness, "sentinel", tmp_path, lengths, _rows([(0, 0, 35, 39), (1, 1, 0, 4), (2, 2, 60, 63), (3, 3, 0, 0)]))
    assert want["covered"].tolist() == [5, 5, 4, 1, 0] and want["max_depth"].tolist() == [1, 1, 1, 1, 0]


def test_depth_past_16_bits(harness, tmp_path):
    """70,000 identical best rows on one gene, a few on its neighbours.  Time limit 60 s."""
    n = 70000
    rows = np.zeros(n + 2, ROW_DTYPE)
    rows[:] = _rows([(0, 1, 3, 70)])[0]
    rows["query"] = np.arange(n + 2)
    rows["subject"][n:] = (0, 2)
    want = _check(harness, "deep", tmp_path, [80, 100, 90], rows, without=False)
    assert want["max_depth"].tolist() == [1, n, 1] and want["spanned"].tolist() == [68, 68 * n, 68] and want["covered"].tolist() == [68, 68, 68]


def test_read_boundaries_cuts_and_the_subject_guard(harness, tmp_path):
    """A read whose rows straddle a 256-thread workgroup boundary with its best row behind it; a read whose rows end exactly at nrows; a top
    row that fails a cut-off, a tie on bits, a read with no passing row; a row whose subject is not below nseq is ignored.  Time limit
    60 s."""
    lengths = [100, 300, 64, 2047]
    spec = [(q, q % 3, q % 30, q % 30 + 30) for q in range(250)]                                    # rows 0 .. 249: one per read
    spec += [(250, 0, 0, 40, 40.0 + k) for k in range(5)] + [(250, 3, 100, 2046, 90.0)] + [(250, 1, 5, 9, 50.0) for _ in range(4)]   # rows 250 .. 259: the best is row 255
    spec += [(251, 2, 0, 63, 80.0, 10, 30), (251, 1, 290, 299, 40.0)]                               # the top row fails min_ident 60
    spec += [(252, 1, 0, 0, 60.0), (252, 2, 1, 1, 60.0)]                                            # a tie: the first
    spec += [(253, 0, 0, 99, 70.0, 5, 30)]                                                          # no passing row
    spec += [(254, 4, 0, 10, 70.0), (255, 32767, 0, 10, 70.0)]                                      # subjects not below nseq
    spec += [(q, 3, (q * 37) % 2000, (q * 37) % 2000 + 46) for q in range(256, 256 + 300)]
    spec += [(600, 1, 7, 8, 10.0), (600, 1, 100, 299, 20.0), (600, 0, 50, 60, 15.0)]                # the last read: its rows end at nrows
    rows = _rows(spec)
    assert rows["query"][255] == rows["query"][256] == 250 and rows["bits"][255] == 90.0 and len(rows) % 256 not in (0, 1)
    for cut in ({}, dict(min_ident=60, min_aln=25)):
        want = _check(harness, "boundaries_%d" % len(cut), tmp_path, lengths, rows, cut)
        best = set(want["best"])
        assert (3, 100, 2046) in best and (1, 100, 299) in best and (1, 0, 0) in best and (2, 1, 1) not in best
        assert ((2, 0, 63) in best) == (not cut) and ((1, 290, 299) in best) == bool(cut) and ((0, 0, 99) in best) == (not cut)
