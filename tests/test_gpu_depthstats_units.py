"""The selection kernel of the depth statistics (csrc/k_depthstats.h: k_depth_select) at the smallest shapes that can go wrong, on depths the
library's own counting kernels mark from synthetic rows - launched by tests/emul/device_depthstats.hip through the library's launch
functions (csrc/mc_abund.h: mc_abund_launch marks, mc_depthstats_launch reads) - test_gpu_coverage_units.py's idiom: the harness includes the
library's headers and is built here with the library's flags, every case is one child process under a time limit of its own, and every
comparison is exact, against tests/depthstats_restated.py applied to the depth that tests/coverage_restated.py's best rows (and, for the
any-depth, tests/ties_restated.py) give.  Every case reads at P = 1, 50, 80, 99 and 100, and at P = 100 its trimmed sum is held to the spanned
figure k_coverage_scan made in the same process.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the unit
modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import coverage_restated as V
import depthstats_restated as D
import order_cases as oc
import ties_restated as T
from microbecensus_amd._native import ROW_DTYPE

pytestmark = pytest.mark.gpu

PARS = np.dtype([("min_ident", "<i4"), ("min_aln", "<i4"), ("min_bits", "<f8"), ("max_loge", "<f8")])   # McAbundPars
assert ROW_DTYPE.itemsize == 72 and PARS.itemsize == 24
KEEPS = [1, 50, 80, 99, 100]
LDS_LEN = oc.define("MC_DS_LDS_LEN", "k_depthstats.h")            # 4096: up to here a gene's depths stay in LDS, above it every walk scans again


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_depthstats", tmp_path_factory)


def _rows(spec):
    """mc_row array of (query, subject, sstart, send[, bits]): bits 50 by default, 27 of 30 identical"""
    arr = np.zeros(len(spec), ROW_DTYPE)
    for i, r in enumerate(spec):
        q, s, a, b = r[:4]
        arr[i] = (q, s, 90.0, 30, 3, 0, 1, 90, a, b, -5.0, r[4] if len(r) > 4 else 50.0, 100, 27)
    return arr


def _one_depth(case, out, at, tab_has, depth_want, lengths):
    """the six sections of one depth, from out[at]: the scan's figures and depth, the difference array before and behind the reads, the reads"""
    nseq = len(lengths)
    fig, depth, before, after = np.frombuffer(out[at], "<u8").reshape(nseq, 3), np.frombuffer(out[at + 1], "<u4"), np.frombuffer(out[at + 2], "<u4"), np.frombuffer(out[at + 3], "<u4")
    got = np.frombuffer(out[at + 4], "<u8").reshape(len(KEEPS), nseq, 4)
    assert np.array_equal(depth, depth_want), "the depth the marks give: first difference at residue %d" % int(np.flatnonzero(depth != depth_want)[0])
    assert np.array_equal(D.depth_of_diff(before, lengths), depth_want), "the difference array"
    assert np.array_equal(before, after), "the reads changed the difference array"
    stats = {}
    for k, P in enumerate(KEEPS):
        want = D.depth_stats(depth_want, lengths, tab_has, P)
        for j, name in enumerate(D.FIGURES):
            bad = np.flatnonzero(got[k, :, j] != want[name].astype(np.uint64))
            assert not len(bad), "%s, P = %d, %s: gene %d (%d residues) gives %d, the restatement %d" % (
                case, P, name, bad[0], lengths[bad[0]], got[k, bad[0], j], want[name][bad[0]])
        assert D.invariants(want, fig[:, 1].astype(np.int64), fig[:, 2].astype(np.int64)) == [], "P = %d" % P
        stats[P] = want
    assert np.array_equal(got[KEEPS.index(100), :, 1], fig[:, 1]), "P = 100: trimmed_sum is k_coverage_scan's spanned"
    return stats, fig


def _check(exe, case, tmp, lengths, rows, ties=False):
    """Runs the case and compares everything with the restatements; returns ({P: the restated figures}, the scan's figures) of the depth and,
    with ties, of the any-depth."""
    pars = np.zeros(1, PARS)
    pars[0] = (0, 0, 0.0, 1.0)
    off = np.zeros(len(lengths) + 1, np.uint32)
    off[1:] = np.cumsum(lengths)
    out = oc.run_child(exe, case, [pars, off, rows, np.int32(KEEPS), np.int32([1 if ties else 0])], tmp, 60, "run")
    nseq = len(lengths)
    assert len(out) == 16
    assert not np.frombuffer(out[12], "<u8").any() and not np.frombuffer(out[13], "<u8").any() and not np.frombuffer(out[14], "<u4").any(), "a write behind a table or a difference array"
    assert len(out[15]) == 2 * 16 * 8 and np.all(np.frombuffer(out[15], "u1") == 0xFF), "a write behind the reads' figures"
    tab = np.frombuffer(out[0], "<u8")
    restated = V.rows_from_array(rows)
    best = V.best_rows(restated, nseq)
    reads = np.bincount([s for s, _, _ in best], minlength=nseq)
    assert np.array_equal(tab[0:2 * nseq:2], reads.astype(np.uint64)) and int(tab[2 * nseq]) == len(best), "the count table"
    own = _one_depth(case, out, 1, reads > 0, D.depth_of_spans(best, lengths), lengths)
    print("%s: %d genes (%d with reads, the longest %d), %d rows, max depth %d" % (case, nseq, int((reads > 0).sum()), max(lengths), len(rows), int(own[1][:, 2].max())))
    if not ties:
        assert all(len(out[k]) == 0 for k in range(6, 12))
        return own
    t = T.ties(restated, lengths)
    assert np.array_equal(np.frombuffer(out[6], "<u8")[0:2 * nseq:2], t["candidates"].astype(np.uint64)), "the head of the tie table"
    return own, _one_depth(case + " (any)", out, 7, t["candidates"] > 0, t["depth_any"], lengths)


def _spans(n, rng, more):
    """spans that leave a gene of n residues with several depths: its ends, its whole, its middle, its second half and `more` random ones"""
    fixed = [(0, 0), (0, n - 1), (n - 1, n - 1), (n // 3, 2 * n // 3), (n // 2, n - 1)]
    a = rng.integers(0, n, more)
    return fixed + [(int(x), int(min(n - 1, x + rng.integers(0, max(1, n // 4) + 1)))) for x in a]


LENGTHS = [1, 2, 3, 63, 64, 65, 199, 200, 201, 255, 256, 257, 2047, LDS_LEN - 1, LDS_LEN, LDS_LEN + 1, 65535]


def test_gene_lengths(harness, tmp_path):
    """Genes of 1 .. 65,535 residues in one database, genes without reads between them (the skip path): both sides of a wave, of the block's
    256 threads, of cut 0 / 1 at P = 99 (199, 200, 201), and of MC_DS_LDS_LEN - the depths in LDS and the scan repeated in every walk.  Time limit 60 s."""
    rng = np.random.default_rng(4096)
    lengths, hit = [], []
    for n in LENGTHS:
        hit.append(len(lengths))
        lengths += [n, 70, 5]
    spec, q = [], 0
    for g, n in zip(hit, LENGTHS):
        for a, b in _spans(n, rng, 12):
            spec.append((q, g, a, b))
            q += 2
    (stats, fig) = _check(harness, "lengths", tmp_path, lengths, _rows(spec))
    assert (fig[hit, 2] >= 3).all() and not np.delete(fig[:, 2], hit).any()
    assert (stats[100]["high"][hit] == fig[hit, 2].astype(np.int64)).all() and (stats[80]["trimmed_sum"][hit] > 0).all()
    assert [D.cut_lo_hi(n, 99)[0] for n in (199, 200, 201)] == [0, 1, 1] and LDS_LEN == 4096


def test_depth_shapes(harness, tmp_path):
    """All residues equal (low == high); a pile of 300 reads on 30 residues of a 400-residue gene; a staircase whose plateaus straddle the ranks
    lo and hi - 1; two values only; depths of 255 and 256; depths of 65,535, 65,536 and 65,537 from 65,537 rows (the second and third radix
    digit) - each gene with genes without reads around it.  Time limit 60 s."""
    lengths = [50, 9, 400, 9, 100, 9, 64, 9, 40, 9, 40]
    spec = [(0, 0, 0, 49)] * 3                                                                      # 0: equal
    spec += [(0, 2, 100, 129)] * 300                                                                # 2: the pile
    spec += [(0, 4, 5, 99), (0, 4, 20, 99), (0, 4, 80, 99), (0, 4, 95, 99)]                         # 4: the staircase: 5 zeros, 15 ones, 60 twos, 15 threes, 5 fours
    spec += [(0, 6, 10, 40)]                                                                        # 6: two values
    spec += [(0, 8, 0, 39)] * 255 + [(0, 8, 20, 39)]                                                # 8: 255 and 256
    spec += [(0, 10, 0, 29)] * 65535 + [(0, 10, 10, 29), (0, 10, 20, 29)]                           # 10: 65,535 .. 65,537 and ten zeros
    rows = _rows(spec[:1])[0]
    arr = np.zeros(len(spec), ROW_DTYPE)
    arr[:] = rows
    arr["query"] = np.arange(len(spec))
    arr["subject"], arr["sstart"], arr["send"] = (np.array([r[k] for r in spec], np.int32) for k in (1, 2, 3))
    stats, fig = _check(harness, "shapes", tmp_path, lengths, arr)
    st = stats[80]
    at = lambda s, P=80: tuple(int(stats[P][k][s]) for k in D.FIGURES)
    assert at(0) == (3, 3 * 40, 3, 3) and at(0, 1) == (3, 3 * 2, 3, 3)
    assert at(2) == (0, 0, 0, 0) and int(fig[2, 2]) == 300 and at(2, 100) == (0, 9000, 0, 300), "the pile moves neither the median nor tad80"
    assert at(4) == (2, 10 + 120 + 30, 1, 3) and D.cut_lo_hi(100, 80) == (10, 10, 90), "ties at both boundaries"
    assert at(6) == (0, 25, 0, 1) and at(6, 1) == (0, 0, 0, 0) and at(6, 100) == (0, 31, 0, 1)
    assert at(8) == (255, 16 * 255 + 16 * 256, 255, 256)
    assert at(10) == (65535, 10 * 65535 + 10 * 65536 + 6 * 65537, 0, 65537) and at(10, 1) == (65535, 65535 + 65536, 65535, 65536)
    assert not st["trimmed_sum"][1::2].any()


@pytest.mark.parametrize("nseq", [1, 3, 4, 5])
def test_gene_counts(harness, tmp_path, nseq):
    """1, 3, 4 and 5 genes, all with reads: a workgroup per gene, the last one's output ends the buffer.  Time limit 60 s."""
    lengths = [130, 64, 7, 65, 300][:nseq]
    rng = np.random.default_rng(nseq)
    spec = [(q, g, a, b) for g in range(nseq) for q, (a, b) in enumerate(_spans(lengths[g], rng, 4), 10 * g)]
    stats, fig = _check(harness, "genes%d" % nseq, tmp_path, lengths, _rows(spec))
    assert (fig[:, 0] > 0).all() and (stats[100]["trimmed_sum"] > 0).all()


def test_the_any_depth(harness, tmp_path):
    """Reads that tie across two genes: the any-depth holds the spans of both, the depth those of the first - the same read on the other pair
    of tables, the head of the tie table saying which genes are walked (gene 1 has candidates and no reads).  Time limit 60 s."""
    lengths = [120, 90, 30, 300]
    spec = []
    for q in range(40):
        spec += [(q, 0, q, q + 60, 70.0), (q, 1, q, q + 40, 70.0)]                                  # tie: gene 0 is assigned, gene 1 a candidate
    spec += [(40 + q, 3, 5 * q, 5 * q + 100, 60.0) for q in range(30)] + [(70, 3, 0, 299, 50.0), (70, 0, 0, 119, 50.0), (70, 2, 3, 9, 40.0)]
    (stats, fig), (stats_any, fig_any) = _check(harness, "any", tmp_path, lengths, _rows(spec), ties=True)
    assert int(fig[1, 1]) == 0 and int(fig_any[1, 1]) == 40 * 41 and not stats[100]["trimmed_sum"][1] and int(stats_any[100]["trimmed_sum"][1]) == 40 * 41
    assert int(stats_any[80]["median"][1]) > 0 and int(stats_any[80]["median"][0]) > int(stats[80]["median"][0]) and not fig_any[2].any()
