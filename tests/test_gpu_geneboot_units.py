"""The gene bootstrap's kernels (csrc/k_geneboot.h) on synthetic rows at the smallest shapes that can go wrong: k_geneboot_collect, launched
behind the counting kernel by the library's launch function, and the three kernels of a read, launched by mc_geneboot_launch
(csrc/mc_abund.h), run by tests/emul/device_geneboot.hip - test_gpu_curve_units.py's idiom: the harness includes the library's headers and
is built here with the library's flags, every case is one child process under a time limit of its own, and every comparison is exact,
against tests/geneboot_restated.py (the list, the grouped list, the integer matrix of replicate counts, the six doubles bit for bit) and
tests/abundance_restated.py (the reads / aligned / assigned counters that k_abundance left in the same launches).  The harness also runs
the owner, McAbundance, on the same launches: its counts, stats, dropped and refusal are compared too.  The cases are
tests/geneboot_cases.py's, which tests/test_geneboot_host.py runs on the CPU.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import geneboot_cases as gc
import geneboot_restated as GR
import order_cases as oc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in gc.cases()}
ENTRY = np.dtype([("q", "<u4"), ("gene", "<u4")])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_geneboot", tmp_path_factory)


def _padding_untouched(out, read):
    """nothing was written behind any array: the padding of tab, the cursor, mat, the genes' cursors, their indices and the scales still
    zero, that of the two lists still 0xEE, that of the output still 0xFF"""
    assert len(out[4]) == len(out[6]) == 128 and len(out[5]) == 128
    assert not any(np.frombuffer(out[k], "u1").any() for k in (4, 6)), "a write behind tab or the cursor"
    assert np.all(np.frombuffer(out[5], "u1") == 0xEE), "a write behind the list"
    if read:
        assert [len(out[k]) for k in range(10, 16)] == [128, 128, 128, 64, 64, 128]
        assert np.all(np.frombuffer(out[10], "u1") == 0xEE), "a write behind the grouped list"
        assert np.all(np.frombuffer(out[12], "u1") == 0xFF), "a write behind the output"
        assert not any(np.frombuffer(out[k], "u1").any() for k in (11, 13, 14, 15)), "a write behind mat, the genes' cursors, their indices or the scales"


def _check(exe, name, tmp):
    c = CASES[name]
    out = oc.run_child(exe, name, gc.sections_in(c), tmp, 60, "run")
    e = gc.expect(c)
    status = np.frombuffer(out[0], "<i4")
    nseq, B, cap, n = c["nseq"], c["B"], gc.capacity(c), len(e["q"])
    read = bool(status[3])
    assert len(out) == (20 if status[0] else 7) and read == (c["launch"] and cap >= n)
    _padding_untouched(out, read)
    tab, lst, cur = np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], ENTRY), np.frombuffer(out[3], "<u8")
    # the counting kernel of the same launches still counts what it counted
    ab = e["ab"]
    assert np.array_equal(tab[0:2 * nseq:2], ab["reads"][:nseq].astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == int(ab["reads"][:nseq].sum()) == n and int(tab[2 * nseq + 1]) == 0, "assigned"
    assert len(lst) == cap
    want = sorted(zip(e["q"].tolist(), e["s"].tolist()))
    if not c["launch"]:                                                                   # no list handed over: list memory is as it was
        assert np.all(np.frombuffer(out[2], "u1") == 0xEE) and not cur.any()
        return None
    # the cursor counts every assigned read; the list holds the first min(n, capacity) slots, each an assigned read, none twice
    assert int(cur[0]) == n and int(cur[1]) == max(0, n - cap), "cursor %d, dropped %d" % (cur[0], cur[1])
    got = sorted(zip(lst["q"][:min(n, cap)].tolist(), lst["gene"][:min(n, cap)].tolist()))
    assert len(set(got)) == len(got) and set(got) <= set(want) and (got == want or cap < n), "the list"
    assert np.all(np.frombuffer(out[2], "u1")[8 * min(n, cap):] == 0xEE), "a write behind the last entry"
    dropped, ocounts, ostats, err = int(np.frombuffer(out[16], "<i8")[0]), np.frombuffer(out[17], "<i8"), np.frombuffer(out[18], "<f8"), bytes(out[19]).decode()
    if not read:
        assert status[1] == -1 and dropped == n - cap and ("mc_gene_bootstrap: %d assigned reads did not fit the list of %d entries" % (n - cap, cap)) in err
        assert (ocounts == -1).all() and (ostats == -1.0).all()                           # the refusal computed nothing
        return None
    # the grouped list: gene by gene in the order of the compact index, each gene's slice holds exactly its reads
    ng = int(status[2])
    have = np.flatnonzero(np.bincount(e["s"], minlength=nseq))
    assert ng == len(have)
    srt = np.frombuffer(out[7], ENTRY)
    assert len(srt) == n and np.all(np.diff(srt["gene"].astype(np.int64)) >= 0)
    assert sorted(zip(srt["q"].tolist(), have[srt["gene"]].tolist())) == want, "the grouped list"
    mat, res = np.frombuffer(out[8], "<u8").reshape(ng, B), np.frombuffer(out[9], "<f8").reshape(ng, 6)
    assert np.array_equal(mat.astype(np.int64), e["counts"][have]), "the replicate counts of the genes with reads"
    assert GR.same_bits(res, e["stats"][have]), "the six doubles of the genes with reads: %s against %s" % (res.tolist(), e["stats"][have].tolist())
    # the owner on the same launches: every gene, the genes without reads among them
    assert status[1] == 0 and dropped == 0 and err == ""
    gc.compare(c, ocounts, ostats)
    print("%s: %d genes (%d with reads), %d rows in %d launches, B %d (m %d), %d entries, %d per tile" % (name, nseq, ng, len(c["rows"]), len(c["cuts"]), B, e["m"], n, GR.per_tile(n, B)))
    return e


@pytest.mark.parametrize("B", gc.BS)
def test_replicate_tiles_and_sort_padding(harness, tmp_path, B):
    """B = 1, 63, 64, 65, 257 and 4096: replicate tiles of 64 and one over, a sort padded from one over a power of two, the limits; from 63
    on every third scale is NaN, 0, negative or infinite, so that m < B.  Time limit 60 s."""
    e = _check(harness, "b%d" % B, tmp_path)
    assert e["m"] == (B if B < 63 else B - len(range(0, B, 3)))


@pytest.mark.parametrize("nseq", [1, 3, 4, 5])
def test_gene_counts(harness, tmp_path, nseq):
    """1, 3, 4 and 5 genes, genes without reads between genes with reads.  Time limit 60 s."""
    e = _check(harness, "genes%d" % nseq, tmp_path)
    assert e["counts"][0].any() and (nseq < 3 or not e["counts"][1].any())


def test_one_gene_holds_every_read(harness, tmp_path):
    """more entries than two tiles, all of one gene: every tile flushes into the same row of mat.  Time limit 60 s."""
    e = _check(harness, "one_gene", tmp_path)
    assert len(e["q"]) == 200 and GR.per_tile(200, 64) == 64


def test_tile_boundary_on_a_gene_boundary(harness, tmp_path):
    """64 reads of one gene, then 64 of another, then 7 of a third, 64 entries per tile, two replicate tiles.  Time limit 60 s."""
    e = _check(harness, "boundary", tmp_path)
    assert np.bincount(e["s"]).tolist() == [64, 0, 64, 7]


@pytest.mark.parametrize("ncut", [0, 2])
def test_three_launches_read_boundaries_and_the_largest_id(harness, tmp_path, ncut):
    """Three launches with cuts between reads: reads that straddle a workgroup boundary, a top row that fails a cut-off, a tie, subjects not
    below nseq; a non-zero first id; the id 2^31 - 1.  Time limit 60 s."""
    e = _check(harness, "launches_%d" % ncut, tmp_path)
    best = dict(zip(e["q"].tolist(), e["s"].tolist()))
    assert best[250] == 3 and best[600] == 1 and best[252] == 1 and 254 not in best and 255 not in best and best[2 ** 31 - 1] == 2 and best[5003] == 3
    assert (best[251] == 2) == (not ncut) and (253 in best) == (not ncut)


def test_one_used_replicate_and_none(harness, tmp_path):
    """m = 1: sum and all four order statistics are the one value, m2 is 0; m = 0: all six are NaN.  Time limit 60 s."""
    e = _check(harness, "m_one", tmp_path)
    assert e["m"] == 1 and (e["stats"][:, 1] == 0).all() and all((e["stats"][:, k] == e["stats"][:, 0]).all() for k in (2, 3, 4, 5))
    e = _check(harness, "m_none", tmp_path)
    assert e["m"] == 0 and np.isnan(e["stats"]).all()


def test_equal_values_across_replicates(harness, tmp_path):
    """a constant scale and tied counts.  Time limit 60 s."""
    e = _check(harness, "tied", tmp_path)
    assert e["stats"][0][2] == e["stats"][0][3] == 0.0 and e["stats"][0][4] <= e["stats"][0][5]


def test_capacity_one_short(harness, tmp_path):
    """dropped == 1, nothing is written behind the list, and the owner's read returns its error - an ordinary refusal.  Time limit 60 s."""
    assert _check(harness, "short", tmp_path) is None


def test_no_list_handed_over_leaves_list_memory_untouched(harness, tmp_path):
    """mc_abund_launch with G == nullptr: the counts are counted, list memory and the cursor stay as they were.  Time limit 60 s."""
    assert _check(harness, "off", tmp_path) is None
