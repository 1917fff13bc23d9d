"""The coverage bootstrap's kernels (csrc/k_covboot.h) on synthetic rows at the smallest shapes that can go wrong: k_covboot_collect,
launched behind the counting kernel k_abundance_cov by the library's launch function, and the three kernels of a read - k_covboot_scatter,
k_covboot_cover and the gene bootstrap's k_geneboot_summary - launched by mc_covboot_launch (csrc/mc_abund.h), run by
tests/emul/device_covboot.hip - test_gpu_tieboot_units.py's idiom: the harness includes the library's headers and is built here with the
library's flags, every case is one child process under a time limit of its own, and every comparison is exact, against
tests/covboot_restated.py (the entry multiset, the cursor and dropped, the grouped list's slices, the integer matrix of covered residues,
det, the six doubles bit for bit), tests/abundance_restated.py and tests/coverage_restated.py (what k_abundance_cov left in the same
launches: the count table and the difference array).  Every array is padded and the padding is checked as untouched.  The harness also runs
the owner, McAbundance, on the same launches: its covered residues, stats, detected, dropped and refusal are compared too, and its own
coverage scan bounds every replicate.  The cases are tests/covboot_cases.py's, which tests/test_covboot_host.py runs on the CPU.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import covboot_cases as cbc
import covboot_restated as CR
import geneboot_restated as GR
import order_cases as oc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in cbc.cases()}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_covboot", tmp_path_factory)


def _padding_untouched(out, read):
    """nothing was written behind any array: the padding of the count table, the difference array, the cursor, det, the genes' cursors, their
    indices, their records and the ones as it was uploaded (zeros), that of the two lists and of mat still 0xEE, that of the output still 0xFF"""
    assert [len(out[k]) for k in (5, 6, 7, 8)] == [128, 64, 192, 128]
    assert not any(np.frombuffer(out[k], "u1").any() for k in (5, 6, 8)), "a write behind the count table, the difference array or the cursor"
    assert np.all(np.frombuffer(out[7], "u1") == 0xEE), "a write behind the list"
    if read:
        assert [len(out[k]) for k in range(13, 21)] == [192, 128, 128, 128, 64, 64, 256, 128]
        assert np.all(np.frombuffer(out[13], "u1") == 0xEE) and np.all(np.frombuffer(out[14], "u1") == 0xEE), "a write behind the grouped list or mat"
        assert np.all(np.frombuffer(out[16], "u1") == 0xFF), "a write behind the output"
        assert not any(np.frombuffer(out[k], "u1").any() for k in (15, 17, 18, 19, 20)), "a write behind det, the genes' cursors, their indices, their records or the ones"


def _check(exe, name, tmp):
    c = CASES[name]
    out = oc.run_child(exe, name, cbc.sections_in(c), tmp, 60, "run")
    x = cbc.expect(c)
    status = np.frombuffer(out[0], "<i4")
    nseq, B, cap, n = c["nseq"], c["B"], cbc.capacity(c), len(x["q"])
    read, owner = bool(status[3]), c["launch"] and cap > 0
    assert len(out) == (27 if owner else 21) and read == (c["launch"] and cap >= n)
    _padding_untouched(out, read)
    tab, diff, lst, cur = np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<u4"), np.frombuffer(out[3], CR.ENTRY), np.frombuffer(out[4], "<u8")
    # the counting kernel of the same launches still counts and marks what it counted and marked
    ab = x["ab"]
    assert np.array_equal(tab[0:2 * nseq:2], ab["reads"][:nseq].astype(np.uint64)) and np.array_equal(tab[1:2 * nseq:2], ab["aligned"][:nseq].astype(np.uint64)), "reads / aligned"
    assert int(tab[2 * nseq]) == int(ab["reads"][:nseq].sum()) == n and int(tab[2 * nseq + 1]) == 0, "assigned"
    assert np.array_equal(diff, x["diff"]), "the difference array k_abundance_cov left"
    assert len(lst) == cap
    want = cbc.entry_set(x["q"], x["g"], x["s"], x["e"])
    if not c["launch"]:                                                                   # no list handed over: list memory is as it was
        assert np.all(np.frombuffer(out[3], "u1") == 0xEE) and not cur.any()
        return None
    # the cursor counts every assigned read; the list holds the first min(n, capacity) slots, each an entry of the restatement, none twice
    assert int(cur[0]) == n and int(cur[1]) == max(0, n - cap), "cursor %d, dropped %d" % (cur[0], cur[1])
    fit = min(n, cap)
    got = cbc.entry_set(lst["q"][:fit], lst["gene"][:fit], lst["s"][:fit], lst["e"][:fit])
    assert len({g[0] for g in got}) == len(got) and set(got) <= set(want) and (got == want or cap < n), "the list"
    assert np.all(np.frombuffer(out[3], "u1")[12 * fit:] == 0xEE), "a write behind the last entry"
    if owner:
        dropped, ocov, ostats, odet, err, scan = (int(np.frombuffer(out[21], "<i8")[0]), np.frombuffer(out[22], "<i8"), np.frombuffer(out[23], "<f8"), np.frombuffer(out[24], "<i8"),
                                                  bytes(out[25]).decode(), np.frombuffer(out[26], "<i8"))
        assert np.array_equal(scan, x["cv"]["covered"]), "the owner's coverage scan"
    if not read:
        assert not any(len(out[k]) for k in range(9, 21))
        if owner:                                                                         # the owner's refusal names the number and computed nothing
            assert status[1] == -1 and dropped == n - cap and ("mc_coverage_bootstrap: %d assigned reads did not fit the list of %d entries" % (n - cap, cap)) in err
            assert (ocov == -1).all() and (ostats == -1.0).all() and (odet == -1).all()
        return None
    # the grouped list: gene by gene in the order of the compact index, each gene's slice holds exactly its entries
    ng = int(status[2])
    have = np.flatnonzero(ab["reads"][:nseq])
    assert ng == len(have)
    srt = np.frombuffer(out[9], CR.ENTRY)
    assert len(srt) == n and np.all(np.diff(srt["gene"].astype(np.int64)) >= 0)
    assert np.array_equal(np.bincount(srt["gene"], minlength=ng), ab["reads"][:nseq][have]), "the slices"
    assert cbc.entry_set(srt["q"], have[srt["gene"]], srt["s"], srt["e"]) == want, "the grouped list"
    mat, det, res = np.frombuffer(out[10], "<u8").reshape(ng, B), np.frombuffer(out[11], "<u8"), np.frombuffer(out[12], "<f8").reshape(ng, 6)
    assert np.array_equal(mat.astype(np.int64), x["cov"][have]), "the covered residues of the genes with reads"
    assert np.array_equal(det.astype(np.int64), x["det"][have] if x["det"] is not None else np.zeros(ng, np.int64)), "det of the genes with reads"
    assert GR.same_bits(res, x["stats"][have]), "the six doubles of the genes with reads: %s against %s" % (res.tolist(), x["stats"][have].tolist())
    # the owner on the same launches: every gene, the genes without reads among them; its own scan bounds every replicate
    assert status[1] == 0 and dropped == 0 and err == "" and len(odet) == (0 if c["F"] is None else nseq)
    cbc.compare(c, ocov, ostats, odet)
    cbc.invariants(c, ocov.reshape(nseq, B), scan, x["counts"])
    print("%s: %d genes (%d with reads, the longest %d residues), %d rows in %d launches, B %d, %d entries" % (name, nseq, ng, max(c["lengths"]), len(c["rows"]), len(c["cuts"]), B, n))
    return x


@pytest.mark.parametrize("B", cbc.BS)
def test_spans_and_replicate_tiles(harness, tmp_path, B):
    """covboot_cases._spans - a single residue, from 0, to len - 1, spans that abut, overlap, nest and repeat, spans across words 64 and 128,
    the empty entry of an invalid span, a gene of one residue, a gene with one read, genes without reads between genes with reads and at the
    end - at B = 1, 63, 64, 65, 257 and 4096; from 64 on a cut-off moves read 9 to another gene.  Time limit 60 s."""
    x = _check(harness, "b%d" % B, tmp_path)
    assert (x["s"] > x["e"]).sum() == 2 and (np.bincount(x["g"], minlength=7) == 0).tolist()[-1] is True


def test_a_gene_longer_than_the_window(harness, tmp_path):
    """MC_CB_WINDOW + 100 residues: spans on both sides of the window's edge, across it, ending on its last word and starting on the next
    window's first.  Time limit 60 s."""
    x = _check(harness, "window", tmp_path)
    assert CASES["window"]["lengths"][1] == CR.WINDOW + 100 and int(x["cov"][1].max()) > 300


def test_one_gene_holds_every_read(harness, tmp_path):
    """200 entries in one slice, walked by one wave per replicate tile; about four replicates in ten cover the whole gene.  Time limit 60 s."""
    x = _check(harness, "one_gene", tmp_path)
    assert 0 < int(x["det"][1]) < 64


def test_slot_reservation_across_workgroups(harness, tmp_path):
    """four workgroups, the second without a read that adds anything; a read that begins at thread 255 and one at thread 0.  Time limit 60 s."""
    x = _check(harness, "workgroups", tmp_path)
    assert len(x["q"]) > 256


def test_three_launches(harness, tmp_path):
    """the rows cut into three launches between reads: the cursor goes on where the launch before left it.  Time limit 60 s."""
    x = _check(harness, "launches", tmp_path)
    assert np.array_equal(x["cov"], cbc.expect(CASES["b63"])["cov"])                     # (the launches change nothing)


def test_no_need_no_detection(harness, tmp_path):
    """need == NULL: det is not touched, the owner returns no detected.  Time limit 60 s."""
    x = _check(harness, "no_need", tmp_path)
    assert x["det"] is None


def test_read_ids_up_to_the_largest(harness, tmp_path):
    """ids 2^31 - 3 .. 2^31 - 1: 32 bits of an entry hold them, and the key is added in 64.  Time limit 60 s."""
    x = _check(harness, "big_ids", tmp_path)
    assert int(x["q"].max()) == 2 ** 31 - 1


def test_capacity_one_short(harness, tmp_path):
    """dropped == 1, nothing is written behind the list, and the owner's read returns its error - an ordinary refusal - and computes
    nothing.  Time limit 60 s."""
    assert _check(harness, "short", tmp_path) is None


def test_no_list_handed_over_leaves_list_memory_untouched(harness, tmp_path):
    """mc_abund_launch with V == nullptr: counts and depth are counted, list memory and the cursor stay as they were.  Time limit 60 s."""
    assert _check(harness, "off", tmp_path) is None


def test_ids_through_a_permuted_map_with_a_base(harness, tmp_path):
    """a class run's ids: base + perm[query] in every entry, the same spans.  Time limit 60 s."""
    x = _check(harness, "idmap", tmp_path)
    perm, base = CASES["idmap"]["idmap"]
    assert x["q"].min() >= base and not np.array_equal(x["cov"], cbc.expect(CASES["b64"])["cov"])
