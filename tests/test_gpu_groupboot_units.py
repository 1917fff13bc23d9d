"""The group bootstrap's kernels (csrc/k_groupboot.h) on synthetic rows and group maps at the smallest shapes that can go wrong:
k_groupboot_values and k_groupboot_summary, launched by mc_groupboot_launch (csrc/mc_abund.h) on the replicate counts the gene bootstrap's
read left on the device, run by tests/emul/device_groupboot.hip - test_gpu_geneboot_units.py's idiom: the harness includes the library's
headers and is built here with the library's flags, every case is one child process under a time limit of its own, and every comparison
is exact, against tests/groupboot_restated.py: the replicate values and the six doubles bit for bit, the replicate counts as integers, on
raw buffers with padding behind each.  The harness also runs the owner, McAbundance, on the same launches: a group read that has to make
the genes' replicate counts, a gene read, and a group read that takes them over - both orders give the same bits -, one of the two asking
for the counts and the other not.  The cases are tests/groupboot_cases.py's, which tests/test_groupboot_host.py runs on the CPU.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import geneboot_restated as GR
import groupboot_cases as grc
import order_cases as oc

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in grc.cases()}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_groupboot", tmp_path_factory)


def _padding_untouched(out):
    """nothing was written behind any array: the padding of val and the output still 0xFF, that of cnt still 0xEE, that of the CSR, the
    members' gene_kb, mat and the scales still zero"""
    assert [len(out[k]) for k in range(6, 14)] == [128, 128, 128, 64, 64, 128, 128, 128]
    assert all(np.all(np.frombuffer(out[k], "u1") == 0xFF) for k in (6, 8)), "a write behind val or the output"
    assert np.all(np.frombuffer(out[7], "u1") == 0xEE), "a write behind cnt"
    assert not any(np.frombuffer(out[k], "u1").any() for k in (9, 10, 11, 12, 13)), "a write behind the CSR, gene_kb, mat or the scales"


def _check(exe, name, tmp):
    c = CASES["grp_" + name]
    out = oc.run_child(exe, c["name"], grc.sections_in(c), tmp, 60, "run")
    e = grc.expect(c)
    status = np.frombuffer(out[0], "<i4")
    B, ngroups, live = c["B"], c["ngroups"], e["live"]
    assert len(out) == 20 and status.tolist() == [int((e["reads"] > 0).sum()), len(live), e["m"], 0, 0, 0], status.tolist()
    _padding_untouched(out)
    # raw buffers: the groups with reads, in ascending group number
    val, cnt, res = np.frombuffer(out[1], "<f8").reshape(len(live), B), np.frombuffer(out[2], "<u8").reshape(len(live), B), np.frombuffer(out[3], "<f8").reshape(len(live), 6)
    assert GR.same_bits(val, e["y"][live]), "val: first difference at %s" % (np.argwhere(val.view(np.uint64) != e["y"][live].view(np.uint64))[:1].tolist(),)
    assert np.array_equal(cnt.astype(np.int64), e["C"][live]), "cnt"
    assert GR.same_bits(res, e["gstats"][live]), "the six doubles of the groups with reads: %s against %s" % (res.tolist(), e["gstats"][live].tolist())
    assert bytes(out[4]) == bytes(out[1]) and bytes(out[5]) == bytes(out[3]), "a launch that asks for no counts gives other values"
    # the owner: every group, those without reads among them; one call with the counts and one without, in both calling orders
    s1, c1, s2, c2 = np.frombuffer(out[14], "<f8"), np.frombuffer(out[15], "<i8"), np.frombuffer(out[16], "<f8"), np.frombuffer(out[17], "<i8")
    ms, err = np.frombuffer(out[18], "<f4"), bytes(out[19]).decode()
    assert err == "" and (len(c1), len(c2)) == ((ngroups * B, 0) if c["counts_first"] else (0, ngroups * B))
    grc.compare(c, None, c1 if len(c1) else None, s1)
    grc.compare(c, None, c2 if len(c2) else None, s2)
    assert bytes(out[14]) == bytes(out[16]), "the group read behind a gene read gives other bits than the one that made its own replicate counts"
    assert ms[0] > 0.0 and ms[1] > ms[0] and ms[2] > 0.0
    print("%s: %d genes (%d with reads) in %d groups (%d with reads), B %d (m %d); group reads %.3f ms, then %.3f ms" % (name, c["nseq"], status[0], ngroups, len(live), B, e["m"], ms[0], ms[1] - ms[0]))
    return e


@pytest.mark.parametrize("B", grc.BS)
def test_replicate_tiles_and_sort_padding(harness, tmp_path, B):
    """B = 1, 63, 64, 65, 257 and 4096: replicate tiles of 64 and one over, a sort padded from one over a power of two, the limits; three
    groups whose members interleave, a gene without reads among them; from 63 on every third scale is NaN, 0, negative or infinite.  Time
    limit 60 s."""
    e = _check(harness, "b%d" % B, tmp_path)
    assert e["m"] == (B if B < 63 else B - len(range(0, B, 3)))


def test_one_group_holds_every_gene(harness, tmp_path):
    """ngroups == 1: the serial walk over all members.  Time limit 60 s."""
    e = _check(harness, "one_group", tmp_path)
    assert np.array_equal(e["C"][0], e["counts"].sum(axis=0))


def test_every_gene_its_own_group(harness, tmp_path):
    """ngroups == nseq: a singleton group's count is its gene's, its value the gene's divided by gene_kb.  Time limit 60 s."""
    e = _check(harness, "singletons", tmp_path)
    assert np.array_equal(e["C"], e["counts"])


def test_members_that_interleave_in_gene_order(harness, tmp_path):
    """two groups of three genes each, alternating.  Time limit 60 s."""
    e = _check(harness, "interleave", tmp_path)
    assert np.array_equal(e["C"][1], e["counts"][1::2].sum(axis=0))


def test_a_group_without_reads_between_two_with(harness, tmp_path):
    """Time limit 60 s."""
    e = _check(harness, "empty_between", tmp_path)
    assert e["live"].tolist() == [0, 2] and not e["gstats"][1].any()


def test_members_without_reads_are_skipped(harness, tmp_path):
    """a group of one member with reads and four without: the kernel sees the one.  Time limit 60 s."""
    e = _check(harness, "one_of_five", tmp_path)
    assert np.array_equal(e["C"][0], e["counts"][2])


def test_more_members_than_a_wave(harness, tmp_path):
    """a group of 70 members with reads, split by a group of five.  Time limit 60 s."""
    e = _check(harness, "seventy", tmp_path)
    assert np.diff(e["plan"][1]).tolist() == [70, 5]


def test_one_used_replicate_and_none(harness, tmp_path):
    """m = 1: sum and all four order statistics are the one value, m2 is 0; m = 0: all six are NaN.  Time limit 60 s."""
    e = _check(harness, "m_one", tmp_path)
    assert e["m"] == 1 and (e["gstats"][:, 1] == 0).all() and all((e["gstats"][:, k] == e["gstats"][:, 0]).all() for k in (2, 3, 4, 5))
    e = _check(harness, "m_none", tmp_path)
    assert e["m"] == 0 and np.isnan(e["gstats"]).all()


def test_gene_kb_of_very_different_magnitudes(harness, tmp_path):
    """gene_kb 0.003 and 196.605 in one group: the addition order shows in the bits (test_groupboot_host.py shows that it does).  Time limit 60 s."""
    _check(harness, "kb_mixed", tmp_path)
