"""The fold of long genes (csrc/k_fold.h, csrc/mc_fold.h) on synthetic rows at the smallest shapes that can go wrong, run by
tests/emul/device_fold.hip through the owner, McAbundance (csrc/mc_abund.h): set_fold, the switches, launch - the fold and then
mc_abund_launch, the library's one site - and the readers.  test_gpu_coverage_units.py's idiom: the harness includes the library's headers
and is built here with the library's flags, every case is one child process under a time limit of its own, no search runs, and every
comparison is exact: the folded rows and edge_rows against tests/fold_restated.py, and the counts, depth, ties, curve and gene-bootstrap
tables against the existing restatements (abundance_restated, coverage_restated, ties_restated, curve_restated, geneboot_restated)
applied to the numpy-folded rows.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the unit
modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import abundance_restated as R
import coverage_restated as CV
import curve_restated as CU
import fold_restated as FR
import geneboot_restated as GR
import order_cases as oc
import ties_restated as TR
from microbecensus_amd._native import ROW_DTYPE

pytestmark = pytest.mark.gpu

PARS = np.dtype([("min_ident", "<i4"), ("min_aln", "<i4"), ("min_bits", "<f8"), ("max_loge", "<f8")])   # McAbundPars
assert ROW_DTYPE.itemsize == 72 and PARS.itemsize == 24 and FR.SEG.itemsize == 16
S = FR.L - FR.V
# genes of 1, 64, 2047, 2048, 2049, 5,000 and 65,535 residues, and between them genes (300 residues, one of two segments) that get no read
LENS = [1, 300, 64, 2047, 300, 2048, 2049, FR.L + 5, 5000, 65535]
QUIET = (1, 4, 7)
B, SEED = 65, 7


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_fold", tmp_path_factory)


def _row(q, s, a, b, bits=50.0, nmatch=27, alnlen=30):
    return (q, s, nmatch * 100.0 / alnlen, alnlen, alnlen - nmatch, 0, 1, 90, a, b, -5.0, bits, 100, nmatch)


def _check(exe, name, tmp, lens, rows, cuts=None, tables=True, curve=True):
    rec, seg_gene, seg_off, seg_res = FR.records(lens)
    ng, nsegs, n = len(lens), len(rec), len(rows)
    goff = np.zeros(ng + 1, np.uint32)
    goff[1:] = np.cumsum(lens)
    cuts = np.uint32(cuts if cuts is not None else [n])
    nreads = int(rows["query"].max()) + 1 if n else 1
    points = np.uint64([max(1, nreads // 4), max(1, nreads // 2), nreads]) if curve else np.zeros(0, np.uint64)
    scale = np.where(np.arange(B) % 5 == 3, np.nan, 1.0 / (1.0 + np.arange(B)))
    pars = np.zeros(1, PARS)
    pars[0] = (0, 0, 0.0, 1.0)
    out = oc.run_child(exe, name, [pars, np.int32([nsegs, ng, len(points), B, max(n, 1)]), rec, goff, rows, cuts, points, scale, np.uint64([SEED])], tmp, 60, "run")
    assert len(out) == 22
    want = FR.fold(rows, rec)
    got = np.frombuffer(out[0], ROW_DTYPE)
    assert FR.same_rows(got, want), "the folded rows: first difference at row %d" % next(i for i in range(n) if not FR.same_rows(got[i:i + 1], want[i:i + 1]))
    edge = np.frombuffer(out[1], "<i8")
    assert int(edge[0]) == FR.edge_rows(rows, rec) and int(edge[1]) == ng, "edge_rows %d against %d" % (edge[0], FR.edge_rows(rows, rec))
    # everything behind the fold is in gene space: the existing statements on the numpy-folded rows (rows of a subject outside the
    # segments have the lowest bits of their read and are no gene's: left out, as the kernels ignore them)
    inside = want[(want["subject"] >= 0) & (want["subject"] < ng) & (rows["subject"] >= 0) & (rows["subject"] < nsegs)]
    ab = R.abundance(R.rows_from_array(inside), ng)
    i8 = lambda k: np.frombuffer(out[k], "<i8")
    assert np.array_equal(i8(2), ab["reads"]) and np.array_equal(i8(3), ab["aligned"]) and int(i8(4)[1]) == ab["assigned"], "reads / aligned / assigned"
    print("%s: %d genes in %d segments, %d rows in %d launches, %d edge rows, %d reads assigned" % (name, ng, nsegs, n, len(cuts), edge[0], ab["assigned"]))
    if not tables:
        return ab
    cov = CV.coverage(CV.rows_from_array(inside), lens)
    for k, key in ((5, "covered"), (6, "spanned"), (7, "max_depth")):
        assert np.array_equal(i8(k), cov[key]), key
    assert np.array_equal(np.frombuffer(out[8], "<u4"), cov["depth"]), "depth"
    ti = TR.ties(CV.rows_from_array(inside), lens)
    assert np.array_equal(i8(9), ti["candidates"]) and np.array_equal(i8(10), ti["unique"]) and np.array_equal(np.frombuffer(out[11], "<u8"), ti["share"]), "ties"
    assert int(i8(12)[0]) == ti["ambiguous"] and np.array_equal(i8(13), ti["covered_any"]), "ambiguous / covered_any"
    if curve:
        cu = CU.curve(CV.rows_from_array(inside), lens, points.tolist())
        for k, key in ((14, "reads"), (15, "aligned"), (16, "covered")):
            assert np.array_equal(i8(k).reshape(len(points), ng), cu[key]), "curve " + key
        assert np.array_equal(i8(17), cu["assigned"]) and int(i8(18)[0]) == cu["beyond"], "curve totals"
    q, s = GR.assignments(R.rows_from_array(inside), ng)
    cm = GR.counts(q, s, ng, B, SEED)
    assert np.array_equal(i8(19).reshape(ng, B), cm) and int(i8(21)[0]) == 0, "the replicate counts"
    assert GR.same_bits(np.frombuffer(out[20], "<f8").reshape(ng, 6), GR.stats(cm, scale)), "the six doubles"
    return ab


def test_spans_on_first_middle_and_last_segments_edges_and_subjects_out_of_range(harness, tmp_path):
    """Every gene that gets reads: [0, 0] on its first segment and [len - 1, len - 1] on its last; the genes of more than 2,048 residues a
    span across residue 2,047 of the gene, on the segment that holds it; the long ones rows on a middle segment, a span that starts on an
    interior edge and one that ends on one; a tie between two segments of ONE gene (one tied subject after the fold) and between two genes;
    subjects -1, nsegs and nsegs + 5 below a read's other rows.  Three launches with cuts between reads.  Time limit 60 s."""
    rec, seg_gene, seg_off, seg_res = FR.records(LENS)
    nsegs, first = len(rec), {g: int(np.flatnonzero(seg_gene == g)[0]) for g in range(len(LENS))}
    spec, q, edges = [], 0, 0
    for g, n in enumerate(LENS):
        if g in QUIET:
            continue
        f, l = first[g], first[g] + len(FR.segments(n)) - 1
        spec.append(_row(q, f, 0, 0)); q += 1
        spec.append(_row(q, l, int(seg_res[l]) - 1, int(seg_res[l]) - 1)); q += 1
        if n > 2048 + 8:
            j = FR.seg_of(2040, n)
            spec.append(_row(q, f + j, 2040 - j * S, 2055 - j * S)); q += 1
        if l - f >= 2:
            m = f + (l - f) // 2
            spec += [_row(q, m, 10, 200), _row(q + 1, m, 0, 99), _row(q + 2, m, FR.L - 100, FR.L - 1), _row(q + 3, f, 5, FR.L - 1), _row(q + 4, l, 0, 3)]
            q += 5; edges += 4
            # two segments of one gene tie (the overlap holds the span in both): one tied subject; then a tie with another gene
            spec += [_row(q, m, S + 20, S + 60, bits=77.0), _row(q, m + 1, 20, 60, bits=77.0)]; q += 1
            spec += [_row(q, m, 300, 340, bits=66.0), _row(q, first[2], 3, 43, bits=66.0)]; q += 1
        spec += [_row(q, l, 0, 0, bits=60.0), _row(q, -1, 0, 5, bits=1.0), _row(q, nsegs, 0, 5, bits=1.0), _row(q, nsegs + 5, 2, 9, bits=1.0)]
        edges += 1 if l > f else 0
        q += 1
    rows = np.zeros(len(spec), ROW_DTYPE)
    for i, r in enumerate(spec):
        rows[i] = r
    cut1 = int(np.searchsorted(rows["query"], q // 3)); cut2 = int(np.searchsorted(rows["query"], 2 * q // 3))
    ab = _check(harness, "spans", tmp_path, LENS, rows, cuts=[cut1, cut2, len(rows)])
    assert FR.edge_rows(rows, rec) >= edges > 8
    assert all(ab["reads"][g] == 0 for g in QUIET) and all(ab["reads"][g] > 0 for g in range(len(LENS)) if g not in QUIET)
    ti = TR.ties(CV.rows_from_array(FR.fold(rows[(rows["subject"] >= 0) & (rows["subject"] < nsegs)], rec)), LENS)
    assert ti["ambiguous"] == sum(1 for g, n in enumerate(LENS) if g not in QUIET and len(FR.segments(n)) >= 3) == 5, "only the ties between two GENES are ambiguous: two segments of one gene are one subject"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_row_counts_around_a_wave(harness, tmp_path, n):
    """0, 1, 63, 64 and 65 rows: no kernel at all, one lane, one short of a wave, a wave, one over.  Time limit 60 s."""
    rec, _, _, seg_res = FR.records(LENS)
    rows = FR.random_rows(np.random.default_rng(100 + n), n, len(rec), seg_res)
    _check(harness, "rows%d" % n, tmp_path, LENS, rows)


def test_a_hundred_thousand_rows_in_two_launches(harness, tmp_path):
    """100,003 rows, 391 workgroups, a second launch smaller than the first (the folded rows are not grown again): the folded rows,
    edge_rows and the counts; the other tables are compared on the small cases.  Time limit 60 s."""
    rec, _, _, seg_res = FR.records(LENS)
    rows = FR.random_rows(np.random.default_rng(9), 100003, len(rec), seg_res)
    cut = int(np.searchsorted(rows["query"], rows["query"][70000]))
    ab = _check(harness, "many", tmp_path, LENS, rows, cuts=[cut, len(rows)], tables=False, curve=False)
    assert ab["assigned"] > 40000 and FR.edge_rows(rows, rec) > 10000


def test_no_gene_is_split(harness, tmp_path):
    """a fold over genes that all fit one segment: the identity on subjects and coordinates, and no edge row.  Time limit 60 s."""
    lens = [5, 64, FR.L, 700]
    rec, _, _, seg_res = FR.records(lens)
    assert len(rec) == 4 and (rec["lo"] == -1).all() and (rec["hi"] == -1).all()
    rows = FR.random_rows(np.random.default_rng(3), 300, len(rec), seg_res)
    _check(harness, "unsplit", tmp_path, lens, rows)
    assert FR.edge_rows(rows, rec) == 0 and FR.same_rows(FR.fold(rows, rec), rows)
