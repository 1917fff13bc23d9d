"""The kernels of the counts on class runs on synthetic rows at the smallest shapes that can go wrong: k_geneboot_collect_mapped
(csrc/k_geneboot.h), which takes a read's id through the batch's id map, and k_abund_class_add (csrc/k_abund_classes.h), the per-class
table, both launched by the library's launch function mc_abund_launch (csrc/mc_abund.h) from tests/emul/device_abund_classes.hip -
test_gpu_geneboot_units.py's idiom: the harness includes the library's headers and is built here with the library's flags, every case is
one child process under a time limit of its own, and every comparison is exact, against tests/geneboot_restated.py (the assigned reads)
and tests/abundance_restated.py (the counters k_abundance left in the same launches).  The harness also runs the owner, McAbundance, on
the same launches: its list, cursor, table and `searched` are compared too.

A row's `query` is a position p of the sorted batch; the id of its read is base + perm[p].  perm is a seeded permutation and base is
2^31 - 1 - n, so the largest id is 2^31 - 1 and a sum taken in signed 32 bits would wrap.

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import abundance_restated as R
import curve_cases as cc
import geneboot_restated as GR
import order_cases as oc

pytestmark = pytest.mark.gpu

ENTRY = np.dtype([("q", "<u4"), ("gene", "<u4")])
NSEQ, K = 4, 3
SLOTS = 2 * (oc.define("MC_CLS_MAX", "mc_classes.h") + 1) + 1                     # MC_AC_SLOTS (csrc/k_abund_classes.h)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_abund_classes", tmp_path_factory)


def _rows(nr):
    """nr rows by ascending position: one row per read, but the read at position 254 has three rows (254, 255, 256 - they straddle the
    first workgroup boundary, and its best row is the last) where nr allows; every fifth read's subject is not below nseq"""
    spec, p = [], 0
    while len(spec) < nr:
        if p == 254 and nr >= 257:
            spec += [(p, 0, 0, 30, 40.0), (p, 1, 0, 30, 41.0), (p, 2, 0, 30, 90.0)]
        else:
            spec.append((p, NSEQ if p % 5 == 4 else p % NSEQ, p % 20, p % 20 + 29, 50.0 + p % 7))
        p += 1
    return cc.rows_of(spec[:nr])


def _run(exe, tmp, name, rows, cuts, cls, reads, mapped=True, capacity=None, below=0):
    n = int(rows["query"].max()) + 1 if len(rows) else 1
    perm = np.random.default_rng(len(rows) + 17).permutation(n).astype(np.uint32)
    base = 2 ** 31 - 1 - (n - 1)
    per_launch = [GR.assignments(R.rows_from_array(rows[a:b]), NSEQ) for a, b in zip([0] + list(cuts[:-1]), cuts)]
    q = np.concatenate([x[0] for x in per_launch]).astype(np.int64)
    s = np.concatenate([x[1] for x in per_launch]).astype(np.int64)
    cap = max(1, len(q)) if capacity is None else capacity
    pars = np.zeros(1, cc.PARS)
    pars[0] = (0, 0, 0.0, 1.0)
    out = oc.run_child(exe, name, [pars, np.int32([NSEQ, cap, 1 if mapped else 0, K, below]), np.int64([base]), rows, np.uint32(cuts), np.int32(cls), np.uint64(reads), perm],
                       tmp, 60, "run")
    assert len(out) == 13
    status = np.frombuffer(out[0], "<i4")
    tab, lst, cur, ctab = np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], ENTRY), np.frombuffer(out[3], "<u8"), np.frombuffer(out[4], "<u8")
    # nothing was written behind any array
    assert not any(np.frombuffer(out[k], "u1").any() for k in (5, 7, 8)) and np.all(np.frombuffer(out[6], "u1") == 0xEE)
    # the counting kernel of the same launches counts what it counts without a map
    ab = R.abundance(R.rows_from_array(rows), NSEQ + 1) if len(rows) else {"reads": np.zeros(NSEQ + 1, np.int64), "aligned": np.zeros(NSEQ + 1, np.int64)}
    assert np.array_equal(tab[0:2 * NSEQ:2], ab["reads"][:NSEQ].astype(np.uint64)) and np.array_equal(tab[1:2 * NSEQ:2], ab["aligned"][:NSEQ].astype(np.uint64))
    assert int(tab[2 * NSEQ]) == len(q)
    # the list: the cursor counts every assigned read, the first min(n, capacity) slots hold assigned reads under their GLOBAL ids, none twice
    ids = base + perm[q].astype(np.int64) if mapped else q
    want = sorted(zip(ids.tolist(), s.tolist()))
    assert len(set(ids.tolist())) == len(ids) and (not mapped or not len(ids) or ids.max() <= 2 ** 31 - 1)
    for which, (l, c) in (("launch", (lst, cur)), ("owner", (np.frombuffer(out[9], ENTRY), np.frombuffer(out[10], "<u8")))):
        assert int(c[0]) == len(q) and int(c[1]) == max(0, len(q) - cap), "%s: cursor %d, dropped %d" % (which, c[0], c[1])
        got = sorted(zip(l["q"][:min(len(q), cap)].tolist(), l["gene"][:min(len(q), cap)].tolist()))
        assert len(set(got)) == len(got) and set(got) <= set(want) and (got == want or cap < len(q)), "%s: the list" % which
    assert np.all(np.frombuffer(out[2], "u1")[8 * min(len(q), cap):] == 0xEE), "a write behind the last entry"
    # the per-class table: every launch's reads and assigned reads in its class, the rows below the lowest class in slot K
    assert status[0] == (1 if mapped else 0) and len(ctab) == SLOTS
    if not mapped:
        assert not ctab.any() and len(out[11]) == 0 and len(out[12]) == 0 and status[1] == sum(reads)
        return q, ids, s
    wrows, wasg = np.zeros(K + 1, np.int64), np.zeros(K + 1, np.int64)
    for k, n_k, x in zip(cls, reads, per_launch):
        wrows[k] += n_k
        wasg[k] += len(x[0])
    wrows[K] += below
    assert np.array_equal(ctab[0:2 * (K + 1):2].astype(np.int64), wrows) and np.array_equal(ctab[1:2 * (K + 1):2].astype(np.int64), wasg), "the table: %s" % ctab[:2 * (K + 1)].tolist()
    assert not ctab[2 * (K + 1):SLOTS - 1].any() and int(ctab[SLOTS - 1]) == len(q)       # the slots of classes the run has not; the total as the last piece left it
    assert np.array_equal(np.frombuffer(out[11], "<i8"), wrows) and np.array_equal(np.frombuffer(out[12], "<i8"), wasg), "the owner's table"
    assert status[1] == sum(reads) + below
    return q, ids, s


@pytest.mark.parametrize("nr", [0, 1, 255, 256, 257, 1000])
def test_row_counts(harness, tmp_path, nr):
    """0, 1, 255, 256, 257 and 1,000 rows in one launch of class 1: no workgroup, one thread, one row short of a workgroup, a full one, one
    over - with a read whose rows straddle the boundary - and four workgroups.  3 rows below the lowest class.  Time limit 60 s."""
    rows = _rows(nr)
    q, ids, s = _run(harness, tmp_path, "rows%d" % nr, rows, [nr], [1], [nr + 2], below=3)
    assert len(ids) == len(np.unique(rows["query"][rows["subject"] < NSEQ]))
    if nr >= 257:
        assert s[q == 254].tolist() == [2]                                            # the straddling read: its last row is its best


def test_pieces_of_three_classes_and_an_empty_one(harness, tmp_path):
    """1,000 rows in five launches - classes 2, 0, 0, 1 and 2 again - one of them without rows (a piece of 9 reads, none with a hit):
    every piece adds to its own class, a class that comes back goes on where it was.  Time limit 60 s."""
    rows = _rows(1000)
    cut = [int(np.searchsorted(rows["query"], p)) for p in (300, 300, 640, 641)] + [1000]
    _run(harness, tmp_path, "pieces", rows, cut, [2, 0, 0, 1, 2], [310, 9, 340, 1, 400])


def test_capacity_below_the_assigned_reads(harness, tmp_path):
    """a list seven entries short: the cursor counts every assigned read and `dropped` the seven, as in the unmapped kernel, and nothing
    is written behind the list.  Time limit 60 s."""
    rows = _rows(600)
    n = len(GR.assignments(R.rows_from_array(rows), NSEQ)[0])
    _run(harness, tmp_path, "short", rows, [600], [0], [600], capacity=n - 7)


def test_the_null_map_gives_the_unmapped_entries(harness, tmp_path):
    """mc_abund_launch without a ride: k_geneboot_collect as it was - the entries carry `query` itself - and the per-class buffer stays
    untouched.  Time limit 60 s."""
    rows = _rows(600)
    _, ids, _ = _run(harness, tmp_path, "null", rows, [300, 600], [0, 1], [300, 300], mapped=False)
    assert ids.max() < 600
