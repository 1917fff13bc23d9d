"""The tie kernel (csrc/k_ties.h: k_ties) on synthetic rows at the smallest shapes that can go wrong, launched behind the counting kernel
by tests/emul/device_ties.hip as range_end launches it - test_gpu_coverage_units.py's idiom: the harness includes the library's headers
and is built here with the library's flags, every case is one child process under a time limit of its own, and every comparison is exact,
against tests/ties_restated.py (every counter, the any-depth of every residue and its three figures per gene), tests/abundance_restated.py
(the reads / aligned / assigned counters of the same launch) and tests/coverage_restated.py (the depth beside the any-depth).  The cases
are those of tests/ties_cases.py, which test_ties_host.py runs through the same walk on the CPU.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
three unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import order_cases as oc
import ties_cases as tc

pytestmark = pytest.mark.gpu

ONE = 1 << 32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_ties", tmp_path_factory)


def _run(exe, case, arrays, tmp, limit):
    return oc.run_child(exe, case, arrays, tmp, limit, "run")


def _check(exe, name, c, tmp):
    """Runs the case and compares everything with the restatements; returns the restated ties (for the case's own conditions)."""
    want = tc.expected(name, c)
    t, ab, cv = want
    out = _run(exe, name, tc.sections_in(c), tmp, 60)
    assert len(out) == 10
    nseq, nres = len(c["lengths"]), sum(c["lengths"])
    # nothing was written behind any array (the tie table is ONE array, as in the library: its parts are compared counter by counter below)
    assert all(len(out[k]) >= 128 and not np.frombuffer(out[k], "u1").any() for k in (7, 8, 9)), "a write behind the count table, the tie table or a difference array"
    tab = np.frombuffer(out[0], "<u8")
    reads = ab["reads"][:nseq]
    print("%s: %d genes, %d rows, %d reads assigned, %d ambiguous, %d across groups, largest tied set %d, sum of candidates %d" % (
        name, nseq, len(c["rows"]), int(reads.sum()), t["ambiguous"], t["group_ambiguous"], max(t["k"]) if t["k"] else 0, int(t["candidates"].sum())))
    # the counting kernel of the same launch: still abundance_restated's
    assert np.array_equal(tab[0:2 * nseq:2], reads.astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == int(reads.sum()) and int(tab[2 * nseq + 1]) == 0, "assigned"
    depth_any = np.frombuffer(out[5], "<u4") if c["cov"] else None
    got = tc.check_ties(c, want, np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<u8"), np.frombuffer(out[3], "<u8"), depth_any)
    if c["cov"]:
        fig = np.frombuffer(out[4], "<u8").reshape(nseq, 3)
        for k, key in enumerate(("covered_any", "spanned_any", "max_depth_any")):
            assert np.array_equal(fig[:, k], t[key].astype(np.uint64)), key
        depth = np.frombuffer(out[6], "<u4")
        assert len(depth) == nres and np.array_equal(depth, cv["depth"]) and (depth <= depth_any).all(), "the depth beside the any-depth"
    else:
        assert len(out[4]) == len(out[5]) == len(out[6]) == 0
    return got, t


@pytest.mark.parametrize("how", ["map_cov", "map_cov_cut", "no_map", "no_cov", "counts_only_cut"])
def test_small_shapes(harness, tmp_path, how):
    """One read of one row (share 2^32); k = 2, 3 (the remainder 1 to the first tied subject), 6 and 7; tied rows s0, s1, s0 (k = 2, s0 by its
    first row's span); lower-scoring rows in front of the top rows and tied rows that are not adjacent; a tied row that fails min_ident; a
    higher-scoring row that fails it and lowers T; a first-rule best row with a subject >= nseq (nothing anywhere); tied rows with subjects
    >= nseq behind an in-range first one (ignored); ties inside one group and across two; spans ending at len - 1; a gene of one residue; both
    tied genes marked; a span outside its gene - with and without the group map, the any-depth and the cut-offs.  Time limit 60 s."""
    c = {"map_cov": tc.basics(), "map_cov_cut": tc.basics(cut=tc.CUT), "no_map": tc.basics(groups=False), "no_cov": tc.basics(cov=False),
         "counts_only_cut": tc.basics(groups=False, cov=False, cut=tc.CUT)}[how]
    name = {"map_cov": "basics", "map_cov_cut": "basics_cut", "no_map": "basics_no_map", "no_cov": "basics_no_cov", "counts_only_cut": "basics_counts_only"}[how]
    got, t = _check(harness, name, c, tmp_path)
    cut = bool(c["cut"])
    assert int(got["share"][7]) == ONE // 7 + 4 + ONE // 2 and int(got["share"][1]) == ONE and got["ambiguous"] == 10
    assert got["unique"].tolist() == ([1, 0, 1, 0, 0, 0, 0, 0] if cut else [2, 0, 0, 0, 1, 0, 0, 0])
    if c["group_of"] is not None:
        assert got["group_unique"].tolist() == ([3, 1, 1, 1] if cut else [4, 1, 2, 1]) and got["group_ambiguous"] == (6 if cut else 5)
    else:
        assert len(got["group_unique"]) == 0 and got["group_ambiguous"] == 0
    if c["cov"]:
        assert int(got["depth_any"][30]) == 2 and int(got["depth_any"][29]) == 2                 # the gene of one residue; a span ending at len - 1


@pytest.mark.parametrize("nrows", [1, 256, 257])
def test_row_counts(harness, tmp_path, nrows):
    """1, 256 and 257 rows: one thread, exactly one workgroup, one row into the second.  Time limit 60 s."""
    got, t = _check(harness, "rows%d" % nrows, tc.row_counts(nrows), tmp_path)
    assert got["ambiguous"] == nrows // 2 and int(got["unique"].sum()) == nrows % 2


def test_read_boundaries(harness, tmp_path):
    """A read whose rows straddle a 256-thread workgroup boundary with tied rows on both sides of it (one of them a repeated subject), a
    read whose tied rows end exactly at nrows, and a read that begins at the last row.  Time limit 60 s."""
    got, t = _check(harness, "boundaries", tc.boundaries(), tmp_path)
    assert dict(t["sets"])[250] == [(0, 2, 22), (1, 5, 25), (3, 10, 30)] and dict(t["sets"])[501] == [(3, 39, 39)] and got["ambiguous"] == 2


def test_rows_at_the_top_far_apart(harness, tmp_path):
    """One read of 200 rows with its rows at the top at positions 3, 10, 63, 64, 65, 130 (a repeated subject) and 199, lower-scoring rows
    between them and a higher-scoring row that fails min_ident.  Time limit 60 s."""
    got, t = _check(harness, "long_span", tc.long_span(), tmp_path)
    assert t["k"] == [2, 6, 1] and got["candidates"].tolist() == [1, 1, 1, 1, 1, 1, 1, 2] and got["group_ambiguous"] == 1 and got["group_unique"].tolist() == [0, 0, 2]


def test_one_read_with_500_tied_rows_over_500_subjects(harness, tmp_path):
    """The largest tied set there is.  Time limit 60 s."""
    got, t = _check(harness, "wide_500", tc.wide(1, 500), tmp_path)
    assert t["k"] == [500] and int(got["share"][0]) == ONE // 500 + ONE % 500 and got["candidates"].tolist() == [1] * 500 and got["group_ambiguous"] == 1


def test_64_reads_with_500_tied_rows_over_250_subjects(harness, tmp_path):
    """Every subject twice, the second round behind the first: the duplicate check's worst case, in both walks.  Time limit 60 s."""
    got, t = _check(harness, "wide_250_twice", tc.wide(64, 250), tmp_path)
    assert t["k"] == [250] * 64 and got["candidates"].tolist() == [64] * 250 and int(got["share"][1]) == 64 * (ONE // 250)


def test_100000_reads_tied_on_the_same_two_subjects(harness, tmp_path):
    """200,000 atomics on each of two counters, sums of 2^48: exact.  Time limit 60 s."""
    got, t = _check(harness, "many_100000", tc.many(100_000), tmp_path)
    assert got["share"].tolist() == [0, 100_000 * (ONE // 2), 100_000 * (ONE // 2)] and got["candidates"].tolist() == [0, 100_000, 100_000]
    assert got["group_unique"].tolist() == [0, 100_000] and got["ambiguous"] == 100_000 and got["group_ambiguous"] == 0
