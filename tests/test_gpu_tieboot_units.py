"""The tie bootstrap's kernels (csrc/k_tieboot.h) on synthetic rows at the smallest shapes that can go wrong: k_tieboot_collect, launched
behind the counting kernel and k_ties by the library's launch function, and the three kernels of a read - k_tieboot_scatter, k_tieboot_sums
and the gene bootstrap's k_geneboot_summary - launched by mc_tieboot_launch (csrc/mc_abund.h), run by tests/emul/device_tieboot.hip -
test_gpu_geneboot_units.py's idiom: the harness includes the library's headers and is built here with the library's flags, every case is
one child process under a time limit of its own, and every comparison is exact, against tests/tieboot_restated.py (the entry multiset, the
cursor and dropped, the grouped list's slices, the integer matrix of replicate shares, the six doubles bit for bit),
tests/abundance_restated.py and tests/ties_restated.py (what k_abundance and k_ties left in the same launches).  Every array is padded and
the padding is checked as untouched.  The harness also runs the owner, McAbundance, on the same launches: its shares, stats, dropped and
refusal are compared too.  The cases are tests/tieboot_cases.py's, which tests/test_tieboot_host.py runs on the CPU.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import geneboot_restated as GR
import order_cases as oc
import tieboot_cases as tbc
import tieboot_restated as TR

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in tbc.cases()}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_tieboot", tmp_path_factory)


def _padding_untouched(out, read):
    """nothing was written behind any array: the padding of the two tables, the cursor, mat, the genes' cursors, their indices and the
    scales still zero, that of the two lists still 0xEE, that of the output still 0xFF"""
    assert [len(out[k]) for k in (5, 6, 7, 8)] == [128, 128, 192, 128]
    assert not any(np.frombuffer(out[k], "u1").any() for k in (5, 6, 8)), "a write behind the count table, the tie table or the cursor"
    assert np.all(np.frombuffer(out[7], "u1") == 0xEE), "a write behind the list"
    if read:
        assert [len(out[k]) for k in range(12, 18)] == [192, 128, 128, 64, 64, 128]
        assert np.all(np.frombuffer(out[12], "u1") == 0xEE), "a write behind the grouped list"
        assert np.all(np.frombuffer(out[14], "u1") == 0xFF), "a write behind the output"
        assert not any(np.frombuffer(out[k], "u1").any() for k in (13, 15, 16, 17)), "a write behind mat, the genes' cursors, their indices or the scales"


def _check(exe, name, tmp):
    c = CASES[name]
    out = oc.run_child(exe, name, tbc.sections_in(c), tmp, 60, "run")
    e = tbc.expect(c)
    status = np.frombuffer(out[0], "<i4")
    nseq, B, cap, n = c["nseq"], c["B"], tbc.capacity(c), len(e["q"])
    read, owner = bool(status[3]), c["launch"] and cap > 0
    assert len(out) == (22 if owner else 18) and read == (c["launch"] and cap >= n)
    _padding_untouched(out, read)
    tab, ties, lst, cur = np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<u8"), np.frombuffer(out[3], TR.ENTRY), np.frombuffer(out[4], "<u8")
    # the counting kernel and k_ties of the same launches still count what they counted
    ab, t = e["ab"], e["ties"]
    assigned = int(ab["reads"][:nseq].sum())
    assert np.array_equal(tab[0:2 * nseq:2], ab["reads"][:nseq].astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == assigned == len(e["k"]) and int(tab[2 * nseq + 1]) == 0, "assigned"
    assert np.array_equal(ties[0:2 * nseq:2], t["candidates"].astype(np.uint64)) and np.array_equal(ties[1:2 * nseq:2], t["unique"].astype(np.uint64)), "candidates / unique"
    assert int(ties[2 * nseq]) == t["ambiguous"] and np.array_equal(ties[2 * nseq + 2:], t["share"]), "ambiguous / share"
    assert len(lst) == cap
    want = tbc.entry_set(e["q"], e["s"], e["share"])
    if not c["launch"]:                                                                   # no list handed over: list memory is as it was
        assert np.all(np.frombuffer(out[3], "u1") == 0xEE) and not cur.any()
        return None
    # the cursor counts every entry; the list holds the first min(n, capacity) slots, each an entry of the restatement, none twice
    assert int(cur[0]) == n == int(t["candidates"].sum()) and int(cur[1]) == max(0, n - cap), "cursor %d, dropped %d" % (cur[0], cur[1])
    fit = min(n, cap)
    got = tbc.entry_set(lst["q"][:fit], lst["gene"][:fit], lst["share_m1"][:fit].astype(np.uint64) + np.uint64(1))
    assert len(set(got)) == len(got) and set(got) <= set(want) and (got == want or cap < n), "the list"
    assert np.all(np.frombuffer(out[3], "u1")[12 * fit:] == 0xEE), "a write behind the last entry"
    if owner:
        dropped, oshares, ostats, err = int(np.frombuffer(out[18], "<i8")[0]), np.frombuffer(out[19], "<u8"), np.frombuffer(out[20], "<f8"), bytes(out[21]).decode()
    if not read:
        assert not any(len(out[k]) for k in range(9, 18))
        if owner:                                                                         # the owner's refusal names the number and computed nothing
            assert status[1] == -1 and dropped == n - cap and ("mc_tie_bootstrap: %d entries did not fit the list of %d entries" % (n - cap, cap)) in err
            assert (oshares == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (ostats == -1.0).all()
        return None
    # the grouped list: gene by gene in the order of the compact index, each gene's slice holds exactly its entries
    ng = int(status[2])
    have = np.flatnonzero(t["candidates"])
    assert ng == len(have)
    srt = np.frombuffer(out[9], TR.ENTRY)
    assert len(srt) == n and np.all(np.diff(srt["gene"].astype(np.int64)) >= 0)
    assert np.array_equal(np.bincount(srt["gene"], minlength=ng), t["candidates"][have]), "the slices"
    assert tbc.entry_set(srt["q"], have[srt["gene"]], srt["share_m1"].astype(np.uint64) + np.uint64(1)) == want, "the grouped list"
    mat, res = np.frombuffer(out[10], "<u8").reshape(ng, B), np.frombuffer(out[11], "<f8").reshape(ng, 6)
    assert np.array_equal(mat, e["shares"][have]), "the replicate shares of the genes with candidates"
    assert GR.same_bits(res, e["stats"][have]), "the six doubles of the genes with candidates: %s against %s" % (res.tolist(), e["stats"][have].tolist())
    # the owner on the same launches: every gene, the genes without candidates among them
    assert status[1] == 0 and dropped == 0 and err == ""
    tbc.compare(c, oshares, ostats)
    print("%s: %d genes (%d with candidates), %d rows in %d launches, B %d (m %d), %d entries of %d reads, %d per tile" % (
        name, nseq, ng, len(c["rows"]), len(c["cuts"]), B, e["m"], n, len(e["k"]), GR.per_tile(n, B)))
    return e


@pytest.mark.parametrize("B", tbc.BS)
def test_tied_sets_replicate_tiles_and_sort_padding(harness, tmp_path, B):
    """ties_cases' small shapes - k = 1, 2, 3, 6 and 7, a subject that ties twice, tied rows that are not adjacent, tied rows and a
    first-rule subject >= nseq, a top row that fails a cut-off - at B = 1, 63, 64, 65, 257 and 4096; from 63 on every third scale is NaN, 0,
    negative or infinite, so that m < B.  Time limit 60 s."""
    e = _check(harness, "b%d" % B, tmp_path)
    assert e["m"] == (B if B < 63 else B - len(range(0, B, 3))) and {1, 2, 3, 6, 7} <= set(e["k"])


def test_the_widest_tied_set(harness, tmp_path):
    """k = 500, the limit: 500 entries of one read, the remainder 296 on the first.  Time limit 60 s."""
    e = _check(harness, "k500", tmp_path)
    assert e["k"] == [500, 1] and int(e["share"][0]) == TR.ONE // 500 + 296


def test_genes_without_entries_between_genes_with_entries(harness, tmp_path):
    """Time limit 60 s."""
    e = _check(harness, "gaps", tmp_path)
    assert (e["ties"]["candidates"] > 0).tolist() == [True, False, True, True, False, False, True]


def test_one_gene_in_every_tied_set(harness, tmp_path):
    """more entries than two tiles in one gene's slice: every tile flushes into the same row of mat.  Time limit 60 s."""
    e = _check(harness, "one_gene", tmp_path)
    assert int(e["ties"]["candidates"][1]) == 200 > 2 * tbc.PER_TILE


def test_slot_reservation_across_workgroups(harness, tmp_path):
    """four workgroups, the second without a read that adds anything; a read that begins at thread 255 and one at thread 0.  Time limit 60 s."""
    e = _check(harness, "workgroups", tmp_path)
    assert len(e["k"]) > 256 and len(e["q"]) > len(e["k"])


def test_three_launches(harness, tmp_path):
    """the rows cut into three launches between reads: the cursor goes on where the launch before left it.  Time limit 60 s."""
    e = _check(harness, "launches", tmp_path)
    assert np.array_equal(e["shares"][:, :63], tbc.expect(CASES["b64"])["shares"][:, :63])       # (replicate b does not depend on B, nor on the launches)


def test_one_used_replicate_and_none(harness, tmp_path):
    """m = 1: sum and all four order statistics are the one value, m2 is 0; m = 0: all six are NaN.  Time limit 60 s."""
    e = _check(harness, "m_one", tmp_path)
    assert e["m"] == 1 and (e["stats"][:, 1] == 0).all() and all((e["stats"][:, k] == e["stats"][:, 0]).all() for k in (2, 3, 4, 5))
    e = _check(harness, "m_none", tmp_path)
    assert e["m"] == 0 and np.isnan(e["stats"]).all()


def test_no_read_ties_is_the_gene_bootstrap(harness, tmp_path):
    """cs = c x 2^32 and the six doubles are the gene bootstrap's, bit for bit (tieboot_cases.invariants).  Time limit 60 s."""
    e = _check(harness, "no_ties", tmp_path)
    assert max(e["k"]) == 1 and GR.same_bits(e["stats"], GR.stats(e["counts"], CASES["no_ties"]["scale"]))


def test_capacity_one_short_and_zero(harness, tmp_path):
    """dropped == 1, nothing is written behind the list, and the owner's read returns its error - an ordinary refusal; capacity 0: every
    entry is dropped and nothing is written at all.  Time limit 60 s."""
    assert _check(harness, "short", tmp_path) is None
    assert _check(harness, "zero", tmp_path) is None


def test_no_list_handed_over_leaves_list_memory_untouched(harness, tmp_path):
    """mc_abund_launch with T == nullptr: counts and ties are counted, list memory and the cursor stay as they were.  Time limit 60 s."""
    assert _check(harness, "off", tmp_path) is None


def test_ids_through_a_permuted_map_with_a_base(harness, tmp_path):
    """a class run's ids: base + perm[query] in every entry, the same tied sets.  Time limit 60 s."""
    e = _check(harness, "idmap", tmp_path)
    perm, base = CASES["idmap"]["idmap"]
    assert e["q"].min() >= base and not np.array_equal(e["shares"], tbc.expect(CASES["b64"])["shares"])
