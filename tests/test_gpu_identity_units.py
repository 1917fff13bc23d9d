"""The identity kernels (csrc/k_identity.h) on synthetic rows at the smallest shapes that can go wrong: k_identity (the third walk, behind
the counting kernel) and k_identity_scan, launched by tests/emul/device_identity.hip through the library's launch functions
(csrc/mc_abund.h: mc_abund_launch and mc_identity_launch) - test_gpu_coverage_units.py's idiom: the harness includes the library's headers
and is built here with the library's flags, every case is one child process under a time limit of its own, and every comparison is exact,
against tests/identity_restated.py (the histogram, the three sums, min / median / max and the levels) and tests/abundance_restated.py (the
reads / aligned / assigned counters of the same launch).  The padding behind every buffer must be untouched, and so must the 27 slots
behind bin 100 of every gene.

Every case runs once more with the identity pointer null: the counters are abundance_restated's and the identity buffers, handed to
nobody, hold what they held.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the unit
modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import abundance_restated as R
import identity_restated as I
import order_cases as oc
from microbecensus_amd._native import ROW_DTYPE

pytestmark = pytest.mark.gpu

PARS = np.dtype([("min_ident", "<i4"), ("min_aln", "<i4"), ("min_bits", "<f8"), ("max_loge", "<f8")])   # McAbundPars
STRIDE = oc.define("MC_ID_STRIDE", "mc_identity.h")
assert ROW_DTYPE.itemsize == 72 and PARS.itemsize == 24 and STRIDE == 128 and oc.define("MC_ID_BINS", "mc_identity.h") == I.BINS
LEVELS8 = [0, 1, 50, 63, 64, 65, 99, 100]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_identity", tmp_path_factory)


def _rows(spec):
    """mc_row array of (query, subject, nmatch, alnlen[, bits[, mismatch, gapopen[, loge]]]): bits 50, mismatch alnlen - nmatch, no gap, loge -5"""
    arr = np.zeros(len(spec), ROW_DTYPE)
    for i, r in enumerate(spec):
        q, s, nmatch, alnlen = r[:4]
        bits = r[4] if len(r) > 4 else 50.0
        mis, gap = r[5:7] if len(r) > 5 else (max(alnlen - nmatch, 0), 0)
        loge = r[7] if len(r) > 7 else -5.0
        arr[i] = (q, s, nmatch * 100.0 / max(alnlen, 1), alnlen, mis, gap, 1, 90, 0, max(alnlen - 1, 0), loge, bits, 100, nmatch)
    return arr


def _counters(tab, ab, nseq, assigned):
    assert np.array_equal(tab[0:2 * nseq:2], ab["reads"][:nseq].astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == int(ab["reads"][:nseq].sum()) == assigned and int(tab[2 * nseq + 1]) == 0, "assigned"


def _check(exe, case, tmp, nseq, rows, levels=(), cut=None):
    """Runs the case with the identity on and once more with it off, and compares everything with the restatements; returns the restated
    identity (for the case's own conditions)."""
    cut = cut or {}
    pars = np.zeros(1, PARS)
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    lv, nout = np.int32(list(levels)), 3 + len(levels)
    out = oc.run_child(exe, case, [pars, np.int32([nseq, 1]), rows, lv], tmp, 60, "run")
    assert len(out) == 8
    tab, hist, sums, fig = (np.frombuffer(out[0], "<u8"), np.frombuffer(out[1], "<u4").reshape(nseq, STRIDE), np.frombuffer(out[2], "<u8").reshape(nseq, 4),
                            np.frombuffer(out[3], "<i8").reshape(nseq, nout))
    assert not np.frombuffer(out[4], "<u8").any() and not np.frombuffer(out[5], "<u4").any() and not np.frombuffer(out[6], "<u8").any(), "a write behind tab, hist or sums"
    assert np.all(np.frombuffer(out[7], "u1") == 0xFF), "a write behind the scan's output"
    want = I.identity(I.rows_from_array(rows), nseq, levels, **cut)
    top = int(rows["subject"].max()) if len(rows) else 0
    ab = R.abundance(R.rows_from_array(rows[rows["subject"] >= 0]), max(nseq, top + 1), **cut)      # (indexed by subject: a negative one is left out, as the kernel ignores it)
    print("%s: %d genes, %d rows, %d best rows, %d bins in use, levels %s" % (case, nseq, len(rows), len(want["best"]), int((want["hist"].sum(axis=0) > 0).sum()), list(levels)))
    _counters(tab, ab, nseq, len(want["best"]))
    assert np.array_equal(hist[:, :I.BINS], want["hist"]), "hist: first difference in gene %d" % int(np.flatnonzero((hist[:, :I.BINS] != want["hist"]).any(axis=1))[0])
    assert not hist[:, I.BINS:].any(), "a write behind bin 100 of a gene"
    for k, name in enumerate(("matched", "mismatched", "gap_opens")):
        assert np.array_equal(sums[:, k].view(np.int64), want[name]), name
    assert not sums[:, 3].any(), "the unused word of a sum record"
    for k, name in enumerate(("ident_min", "ident_median", "ident_max")):
        assert np.array_equal(fig[:, k], want[name].astype(np.int64)), name
    assert np.array_equal(fig[:, 3:], want["ge"]), "ge"
    assert np.array_equal(hist[:, :I.BINS].astype(np.int64).sum(axis=1), ab["reads"][:nseq]), "sum(hist) == reads of the counting kernel"
    if not any(r[1] > r[2] or r[1] < 0 for r in want["best"]):       # (the invariants are those of rows with 0 <= nmatch <= alnlen)
        assert I.invariants(want, ab["reads"][:nseq], ab["aligned"][:nseq], list(levels)) == []
    # the identity pointer null: k_identity is not issued, and nobody is handed its buffers
    out = oc.run_child(exe, case + "_without", [pars, np.int32([nseq, 0]), rows, lv], tmp, 60, "run")
    _counters(np.frombuffer(out[0], "<u8"), ab, nseq, len(want["best"]))
    assert not np.frombuffer(out[4], "<u8").any(), "a write behind tab"
    assert all(np.all(np.frombuffer(out[k], "u1") == 0x5A) for k in (1, 2, 3, 5, 6, 7)), "an identity buffer changed with the identity off"
    return want


def test_one_gene_one_read(harness, tmp_path):
    """nseq = 1 with one read of one row: one thread, one wave of the scan.  Time limit 60 s."""
    want = _check(harness, "one", tmp_path, 1, _rows([(0, 0, 27, 30)]), [90])
    assert want["hist"][0, 90] == 1 and want["ident_median"].tolist() == [90] and want["ge"].tolist() == [[1]]


@pytest.mark.parametrize("nlevels", [0, 1, 8])
def test_read_counts_per_gene_and_levels(harness, tmp_path, nlevels):
    """Genes with exactly 1, 2, 3 and 64 reads (n odd and even: the lower median), genes without reads between them, and 5 genes: not a
    multiple of the four waves of a workgroup; under 0, 1 and 8 levels, 0 and 100 among them.  Time limit 60 s."""
    spec, q = [], 0
    for g, n in ((0, 1), (2, 2), (3, 3), (4, 64)):                # (gene 1 has no read)
        for k in range(n):
            spec.append((q, g, 30 + (k * 7) % 31, 60))            # identities 50 % .. 100 %
            q += 2                                                # (reads without rows between them)
    levels = {0: [], 1: [75], 8: LEVELS8}[nlevels]
    want = _check(harness, "counts_%d" % nlevels, tmp_path, 5, _rows(spec), levels)
    assert want["hist"].sum(axis=1).tolist() == [1, 0, 2, 3, 64] and want["ident_min"][1] == want["ident_median"][1] == want["ident_max"][1] == -1
    assert want["ident_median"][2] == want["ident_min"][2] != want["ident_max"][2], "two reads: the lower median is the lower one"
    if nlevels == 8:
        assert want["ge"][:, 0].tolist() == [1, 0, 2, 3, 64] and want["ge"][4, 7] == 2 and (want["ge"][1] == 0).all()      # (60 of 60 at k = 22 and 53: 7 k = 30 mod 31)


def test_bins_at_the_ends_and_at_the_word_boundary(harness, tmp_path):
    """All reads of a gene in bin 0; all in bin 100; reads only in bins 63, 64 and 65 - the last bin of a lane's first word and the first
    two of its second - in every split of the median between them; a row with alnlen 0 (bin 0).  Time limit 60 s."""
    spec, q = [], 0
    def add(g, nmatch, alnlen, n=1):
        nonlocal q
        for _ in range(n):
            spec.append((q, g, nmatch, alnlen))
            q += 1
    add(0, 0, 40, 5)                                               # bin 0
    add(1, 40, 40, 4)                                              # bin 100
    add(2, 63, 100, 2); add(2, 64, 100, 1); add(2, 65, 100, 2)     # median 64
    add(3, 63, 100, 3); add(3, 64, 100, 2); add(3, 65, 100, 1)     # n = 6: the lower median is the 3rd, bin 63
    add(4, 63, 100, 1); add(4, 65, 100, 3)                         # n = 4: the lower median is the 2nd, bin 65
    add(5, 63, 100, 1); add(5, 64, 100, 1)                         # n = 2: bin 63
    add(6, 0, 0, 1); add(6, 199, 200, 1)                           # alnlen 0: bin 0; 199 of 200: bin 99
    want = _check(harness, "ends", tmp_path, 8, _rows(spec), LEVELS8)
    assert want["ident_median"].tolist() == [0, 100, 64, 63, 65, 63, 0, -1]
    assert want["ident_min"].tolist() == [0, 100, 63, 63, 63, 63, 0, -1] and want["ident_max"].tolist() == [0, 100, 65, 65, 65, 64, 99, -1]
    assert want["ge"][2].tolist() == [5, 5, 5, 5, 3, 2, 0, 0] and want["ge"][0].tolist() == [5, 0, 0, 0, 0, 0, 0, 0] and want["ge"][1].tolist() == [4] * 8


def test_row_counts_and_a_read_across_workgroups(harness, tmp_path):
    """257 reads of one row each - one more than a workgroup - then a read whose ten rows straddle rows 511 / 512 with its best row behind
    the boundary, and a last read whose rows end exactly at nrows.  Time limit 60 s."""
    spec = [(q, q % 3, 20 + q % 41, 60) for q in range(257)]
    spec += [(q, 3, 59, 60) for q in range(257, 506)]                                     # rows 257 .. 505
    spec += [(506, 0, 30, 60, 40.0 + k) for k in range(6)] + [(506, 4, 58, 60, 90.0, 1, 1)] + [(506, 1, 45, 60, 50.0) for _ in range(3)]   # rows 506 .. 515: the best is row 512
    spec += [(600, 1, 33, 60, 10.0), (600, 1, 44, 60, 20.0), (600, 0, 55, 60, 15.0)]
    rows = _rows(spec)
    assert rows["query"][255] != rows["query"][256] and rows["query"][511] == rows["query"][512] == 506 and rows["bits"][512] == 90.0
    want = _check(harness, "rows", tmp_path, 5, rows, [50, 90])
    assert (4, 58, 60, 1, 1) in want["best"] and (1, 44, 60, 16, 0) in want["best"] and len(want["best"]) == 508
    assert want["gap_opens"].tolist() == [0, 0, 0, 0, 1]


def test_contention_on_one_gene(harness, tmp_path):
    """5,000 reads on one gene - every atomic of the sums on one line, the histogram's on four - with genes without reads around it and a few
    reads on the others.  Time limit 60 s."""
    n = 5000
    spec = [(q, 2, 25 + q % 36, 60, 50.0, q % 5, q % 2) for q in range(n)] + [(n, 0, 60, 60), (n + 1, 5, 1, 60)]
    want = _check(harness, "contention", tmp_path, 7, _rows(spec), LEVELS8)
    assert want["hist"].sum(axis=1).tolist() == [1, 0, n, 0, 0, 1, 0] and int(want["mismatched"][2]) == sum(q % 5 for q in range(n)) and int(want["gap_opens"][2]) == n // 2


def test_ties_cut_offs_and_the_subject_guard(harness, tmp_path):
    """A read whose two top rows tie in bits with different identities: the first is taken.  Rows that fail each of the four cut-offs, so that
    a lower row of another identity wins; a read with no passing row; a row with alnlen 0 (under min_aln it fails); a subject >= nseq and a
    negative one, both ignored.  Without cut-offs and with all four.  Time limit 60 s."""
    spec = [(0, 1, 54, 60, 60.0), (0, 2, 30, 60, 60.0)]                                    # a tie: the first, 90 %
    spec += [(1, 0, 20, 60, 80.0), (1, 1, 57, 60, 40.0)]                                   # the top row fails min_ident 50
    spec += [(2, 0, 19, 20, 80.0), (2, 2, 48, 60, 40.0)]                                   # ... min_aln 25
    spec += [(3, 0, 60, 60, 25.0), (3, 1, 31, 60, 24.0)]                                   # both fail min_bits 30
    spec += [(4, 2, 60, 60, 80.0, 0, 0, -0.5), (4, 0, 42, 60, 40.0)]                       # the top row fails max_loge -1
    spec += [(5, 1, 0, 0, 70.0)]                                                           # alnlen 0
    spec += [(6, 3, 50, 60, 70.0), (7, 32767, 50, 60, 70.0), (7, 0, 36, 60, 60.0), (8, -1, 50, 60, 70.0)]   # read 7: its best row has no gene of the database, the read counts nowhere
    rows = _rows(spec)
    for cut in ({}, dict(min_ident=50, min_aln=25, min_bits=30.0, max_loge=-1.0)):
        want = _check(harness, "cuts_%d" % len(cut), tmp_path, 3, rows, [60, 95], cut)
        best = [b[:3] for b in want["best"]]
        assert (1, 54, 60) in best and (2, 30, 60) not in best
        assert ((0, 20, 60) in best) == (not cut) and ((1, 57, 60) in best) == bool(cut) and ((2, 48, 60) in best) == bool(cut) and ((0, 42, 60) in best) == bool(cut)
        assert ((0, 60, 60) in best) == (not cut) and ((1, 0, 0) in best) == (not cut) and len(best) == (6 if not cut else 4)


def test_no_rows(harness, tmp_path):
    """nr = 0: no kernel of the range is issued, the scan writes -1 and zeros for every gene.  Time limit 60 s."""
    want = _check(harness, "empty", tmp_path, 6, _rows([]), [0, 100])
    assert not want["hist"].any() and (want["ident_min"] == -1).all() and not want["ge"].any()
