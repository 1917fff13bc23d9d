"""The curve kernels (csrc/k_curve.h) on synthetic rows at the smallest shapes that can go wrong: k_curve, launched behind the counting
kernel by the library's launch function (csrc/mc_abund.h), and k_curve_scan, run by tests/emul/device_curve.hip - test_gpu_coverage_units.py's
idiom: the harness includes the library's headers and is built here with the library's flags, every case is one child process under a
time limit of its own, and every comparison is exact, against tests/curve_restated.py (the bin table, every residue's first id, reads_k,
aligned_k, covered_k, assigned_k and beyond) and tests/abundance_restated.py (the reads / aligned / assigned counters that k_abundance or
k_abundance_cov left in the same launches).  The cases are tests/curve_cases.py's, which tests/test_curve_host.py runs on the CPU.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import curve_cases as cc
import order_cases as oc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in cc.cases()}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_curve", tmp_path_factory)


def _padding_untouched(out):
    """nothing was written behind any array: the padding of tab, the bin table and the points still zero, that of first and the scan's
    output still 0xFF"""
    assert len(out) == 9 and len(out[4]) == len(out[5]) == len(out[7]) == len(out[8]) == 128 and len(out[6]) == 64
    assert not any(np.frombuffer(out[k], "u1").any() for k in (4, 5, 8)), "a write behind tab, the bin table or the points"
    assert all(np.all(np.frombuffer(out[k], "u1") == 0xFF) for k in (6, 7)), "a write behind first or the scan's output"


def _check(exe, c, tmp, coverage):
    out = oc.run_child(exe, "%s_%d" % (c["name"], coverage), cc.sections_in(c, coverage), tmp, 60, "run")
    _padding_untouched(out)
    tab, bins, first, res = np.frombuffer(out[0], "<u8"), np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<u4"), np.frombuffer(out[3], "<u8")
    cv = cc.compare(c, coverage, bins, first, res)
    _, ab, _ = cc.expect(c, coverage)
    nseq = len(c["lengths"])
    # the counting kernel of the same launches - k_abundance_cov with coverage, k_abundance without - still counts what it counted
    assert np.array_equal(tab[0:2 * nseq:2], ab["reads"][:nseq].astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == int(ab["reads"][:nseq].sum()) == len(cv["best"]) and int(tab[2 * nseq + 1]) == 0, "assigned"
    print("%s, coverage %d: %d genes, %d rows in %d launches, K %d, %d best rows, assigned_k %s, beyond %d, covered_k %s" % (
        c["name"], coverage, nseq, len(c["rows"]), len(c["cuts"]), len(c["points"]), len(cv["best"]), cv["assigned"].tolist(), cv["beyond"], cv["covered"].sum(axis=1).tolist()))
    return cv


def _both(exe, name, tmp):
    """the case with coverage on and once more with it off: no first array is handed to a kernel, covered_k is zero, the rest is the same"""
    on = _check(exe, CASES[name], tmp, 1)
    off = _check(exe, CASES[name], tmp, 0)
    assert np.array_equal(on["reads"], off["reads"]) and not off["covered"].any()
    return on


def test_one_point_and_reads_behind_it(harness, tmp_path):
    """K = 1: ids n - 1 and n, and reads behind the point - beyond > 0 and nothing is lost from the bin sums.  Time limit 60 s."""
    cv = _both(harness, "k1", tmp_path)
    assert cv["assigned"].tolist() == [2] and cv["beyond"] == 3 and cv["covered"].tolist() == [[21, 0]]


def test_sixty_four_points_and_ids_at_every_point(harness, tmp_path):
    """K = 64 with a non-zero first id: one read at n_k - 1 and one at n_k for every k.  Time limit 60 s."""
    cv = _both(harness, "k64", tmp_path)
    assert cv["assigned"].tolist() == [2 * k + 1 for k in range(64)] and cv["beyond"] == 1


def test_repeated_points(harness, tmp_path):
    """sampled_reads 3, K 5: the points 1, 2, 2, 3, 3.  Time limit 60 s."""
    cv = _both(harness, "repeats", tmp_path)
    assert cv["assigned"].tolist() == [1, 2, 2, 3, 3] and cv["covered"][:, 0].tolist() == [10, 10, 10, 30, 30] and cv["beyond"] == 0


def test_gene_lengths_and_spans(harness, tmp_path):
    """Genes of 1, 63, 64, 65, 129 and 2,047 residues with genes without reads between them; the spans [0, 0], [len - 1, len - 1] and
    [0, len - 1], each in a bin of its own.  Time limit 60 s."""
    cv = _both(harness, "lengths", tmp_path)
    hit = [0, 3, 6, 9, 12, 15]
    assert cv["covered"][-1][hit].tolist() == cc.LENGTHS and (cv["covered"][-1] > 0).sum() == len(hit)
    assert cv["covered"][0][hit].tolist() == [1, 0, 0, 0, 0, 0] and cv["covered"][4][hit].tolist() == [1, 2, 0, 0, 0, 0] and cv["covered"][5][hit].tolist() == [1, 63, 0, 0, 0, 0]


@pytest.mark.parametrize("nseq", [1, 3, 4, 5])
def test_gene_counts(harness, tmp_path, nseq):
    """1, 3, 4 and 5 genes: not a multiple of the four waves of a workgroup.  Time limit 60 s."""
    cv = _both(harness, "genes%d" % nseq, tmp_path)
    assert (cv["covered"][-1] > 0).all() and cv["beyond"] == 0


@pytest.mark.parametrize("ncut", [0, 2])
def test_read_boundaries_cuts_and_the_subject_guard(harness, tmp_path, ncut):
    """A read whose rows straddle a 256-thread workgroup boundary with its best row behind it (and an id exactly at a point), a read
    whose rows end at nrows, a top row that fails a cut-off, a tie, a read with no passing row, subjects not below nseq.  Time limit 60 s."""
    cv = _both(harness, "straddle_%d" % ncut, tmp_path)
    best = {q: (s, a, b) for q, s, _, a, b in cv["best"]}
    assert best[250] == (3, 100, 2046) and best[600] == (1, 100, 299) and best[252] == (1, 0, 0) and 254 not in best and 255 not in best
    assert (best[251] == (2, 0, 63)) == (not ncut) and (253 in best) == (not ncut) and cv["beyond"] == 0
    assert cv["assigned"][2] - cv["assigned"][1] == 1                 # (read 251 alone lies between the points 251 and 252: read 250 is in the bin before)


def test_two_launches_in_either_order(harness, tmp_path):
    """The same residues covered by two launches, once with the higher ids first and once with the lower ids first: the same first, the
    same curve.  Time limit 60 s."""
    hi = _both(harness, "hi_first", tmp_path)
    lo = _both(harness, "lo_first", tmp_path)
    assert hi["first"] == lo["first"] and all(np.array_equal(hi[k], lo[k]) for k in ("reads", "aligned", "covered", "bin_reads"))
    assert hi["first"][0][5] == 10 and hi["first"][0][0] == 20 and hi["first"][0][45] == 12 and hi["first"][1][10] == 11
