"""The seven kernels of the gapped stage (csrc/k_gapped.h), each on inputs built to reach its own edges - the suite otherwise runs them
inside mc_run_range only, on the flanks real reads happen to produce: but for one constructed read none carries 32 gap runs, none
leaves the 64-column window of the product build, and no read set controls which segments share a tag and a slot of the grouping
table, how many items a wave is dealt, or what the sort is given.
tests/emul/device_gapped.hip includes the library's kernel headers and is built here with the library's flags; every verb is one child
process per test (order_cases.run_child), and every comparison is exact.

The reference of every flank result is the oracle's AlignGapped (gapped_cases.oracle: trace planes and a traceback); which flank
leaves which window follows from the oracle's band width and, for the run counts, from the host statement of the windowed form over
packed cells, which tests/test_gapped_host.py holds to the oracle - never from a device output."""
import numpy as np
import pytest

import gapped_cases as gc
import order_cases as oc

pytestmark = pytest.mark.gpu

SENTINEL = 0xEEEE - 0x10000                                          # an int16 of the fill byte 0xEE


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_gapped", tmp_path_factory)


@pytest.fixture(scope="module")
def world():
    return gc.world()


@pytest.fixture(scope="module")
def base(world):
    return world.sections() + [world.records()]


@pytest.fixture(scope="module")
def pool(world, tmp_path_factory):
    """The item pool with, per item, whether it leaves the first and the second window (gapped_cases.item_pool; the host forms)."""
    tmp = tmp_path_factory.mktemp("gapped_win")
    items = gc.item_pool(world)
    forms, _ = gc.host_forms(gc.build_host_forms(tmp), items, tmp)
    want = np.array([f["o"] for f in items])
    assert np.array_equal(forms[:, 0, :7], want[:, :7])
    leaves = [(want[:, 7] >= W) | forms[:, k, 8].astype(bool) for k, W in ((1, gc.WIN), (2, gc.WIN2))]
    assert (leaves[0] | ~leaves[1]).all()                            # (what leaves the wider window leaves the narrower one)
    return items, want, leaves[0], leaves[1]


def _u32(b):
    return np.frombuffer(b, "<u4")


def _segments(world):
    return [None if t["read"] == gc.TASK_NONE else world.segment(t) for t in world.tasks]


def _n1(seg, side):
    return gc.QLEN[seg[2]] - seg[5] if side == 0 else seg[3]


@pytest.mark.parametrize("table", ("product", "small"))
def test_dedupe(harness, world, base, tmp_path, table):
    """k_gap_dedupe at the product's table size and at the smallest power of two above the number of distinct segments (probe chains,
    probing across the table's end): the members of a segment share one leader, which is one of them and leads itself; no two segments
    share a leader - the near misses in each of the six compared quantities and the equal-tag pairs included; padding records lead
    themselves and list nothing; C_ITEMS and the multiset of (item, key) are those of the leaders' extendable sides.
    Time limit 60 s per child (the whole test measured on the MI355X: 0.50 s / 0.33 s)."""
    n = len(world.tasks)
    slots = gc.table_slots(n) if table == "product" else gc.small_table(world)
    out = oc.run_child(harness, "dedupe_" + table, base + [np.array([slots], np.uint32)], tmp_path, 60, verb="dedupe")
    leader, key, item, counters = (_u32(b) for b in out)
    segs = _segments(world)
    assert len(leader) == n
    by_seg = {}
    for p, seg in enumerate(segs):
        ld = int(leader[p])
        if seg is None:
            assert ld == p, "padding record %d is led by %d" % (p, ld)
            continue
        assert ld < n and segs[ld] == seg, "task %d of segment %s is led by task %d of segment %s" % (p, seg, ld, segs[ld] if ld < n else None)
        assert leader[ld] == ld
        assert by_seg.setdefault(seg, ld) == ld, "segment %s has the leaders %d and %d" % (seg, by_seg[seg], ld)
    assert len(set(by_seg.values())) == len(by_seg)
    for (seg, size) in world.groups:
        assert sum(s == seg for s in segs) >= size
    for a, b, name in world.near:
        assert by_seg[a] != by_seg[b], name
    for a, b in world.pairs:
        assert by_seg[a] != by_seg[b], (a, b)
    want = sorted((2 * ld + side, 1 + _n1(seg, side)) for seg, ld in by_seg.items() for side, fl in enumerate(world.seg_flanks(seg)) if fl is not None)
    ni = int(counters[gc.C_ITEMS])
    assert ni == len(want)
    assert sorted(zip(item[:ni].tolist(), key[:ni].tolist())) == want
    print("%d tasks, %d segments, %d slots, %d items" % (n, len(by_seg), slots, ni))


SORT_N = (0, 1, 255, 256, 257, 511, 512, 513, 100003)
SORT_KEYS = ("equal", "distinct", "ends")


def test_flank_sort(harness, tmp_path):
    """k_gap_sort_hist / _scan / _scatter with the product's grids: the output is a permutation of the items in non-increasing order of
    their keys, the scanned histogram holds every bin's end, the guard words behind the list are intact - for n = 0, 1, around the
    workgroup sizes and 100,003 (a stretch per workgroup that does not divide n), keys all equal, all distinct modulo 1,024 in their
    order of appearance, and only 1 and 1,023; with n = cap + 1 nothing is written.
    Time limit 60 s (the whole test measured on the MI355X: 0.36 s, 29 sets in one child)."""
    rng = np.random.default_rng(11)
    sets = []
    for n in SORT_N:
        for kind in SORT_KEYS:
            key = {"equal": np.full(n, 77), "distinct": 1 + (rng.permutation(max(n, 1))[:n] + 5) % 1023, "ends": np.where(rng.random(n) < 0.5, 1, 1023)}[kind].astype(np.uint32)
            sets.append((n, n, key, rng.permutation(n).astype(np.uint32) * np.uint32(2) + np.uint32(1)))
    for kind in ("equal", "ends"):
        key = (np.full(1001, 77) if kind == "equal" else np.where(rng.random(1001) < 0.5, 1, 1023)).astype(np.uint32)
        sets.append((1001, 1000, key, np.arange(1001, dtype=np.uint32)))
    arrays = [np.array([len(sets)], np.uint32)]
    for n, cap, key, item in sets:
        arrays += [key, item, np.array([n, cap], np.uint32)]
    out = oc.run_child(harness, "sort", arrays, tmp_path, 60)
    for k, (n, cap, key, item) in enumerate(sets):
        got, hist, pad = (_u32(b) for b in out[3 * k:3 * k + 3])
        assert (pad == 0xFFFFFFFF).all(), (n, cap)
        if n > cap:
            assert (got == 0xFFFFFFFF).all() and not hist.any(), "n = cap + 1: something was written"
            continue
        assert len(got) == cap == n
        assert np.array_equal(np.sort(got), np.sort(item)), n
        key_of = dict(zip(item.tolist(), key.tolist()))
        ks = np.array([key_of[i] for i in got.tolist()], np.int64)
        assert (np.diff(ks) <= 0).all(), n
        # behind the scatter a bin's entry is where the bin ends: the keys above it and its own
        ends = np.bincount(key, minlength=1024)[::-1].cumsum()[::-1]
        assert np.array_equal(hist[1:], ends[1:]), n


EXTEND_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000)
EXTEND_GRIDS = ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3))


def _extend_cases(pool):
    """(name, grids, positions in the pool, in the order of the list).  Every count with every grid; the lists are in descending order
    of their keys, as the sort leaves them, but for the last case."""
    items, want, r1, r2 = pool
    rng = np.random.default_rng(5)
    n1 = np.array([len(f["q"]) for f in items])
    designed = np.flatnonzero(np.array([f["cls"] != "member" for f in items]))
    special = np.flatnonzero(r1)                                     # what leaves a window: some in every list of 63 items or more
    cases = []
    for count in EXTEND_COUNTS:
        if count >= 1000:
            sel = np.concatenate([designed, rng.permutation(np.setdiff1d(np.arange(len(items)), designed))[:count - len(designed)]])
        elif count >= 63:
            sel = np.concatenate([rng.permutation(special)[:count // 4], rng.permutation(np.setdiff1d(designed, special))[:count - count // 4]])
        else:
            sel = rng.permutation(designed)[:count]
        assert len(sel) == count == len(set(sel.tolist()))
        sel = sel[np.argsort(-n1[sel], kind="stable")]
        for grid in EXTEND_GRIDS:
            cases.append(("%d items, grids %s" % (count, grid), grid, sel))
    one_key = np.flatnonzero(n1 == np.bincount(n1).argmax())[:200]     # (the members of the largest group: one flank, one key)
    cases.append(("one key", (2, 2, 2), one_key))
    longest, shortest = np.flatnonzero(n1 == 169), np.flatnonzero(n1 == 3)
    m = min(len(longest), len(shortest))
    cases.append(("longest and shortest alternating", (1, 1, 1), np.stack([longest[:m], shortest[:m]], 1).ravel()))
    assert len(one_key) > 64 and m >= 20
    return cases


def test_extend_equals_the_oracle(harness, world, base, pool, tmp_path):
    """The three DP launches as stage_b issues them - k_gapped_lds at 36 columns, at 64 columns, k_gapped on full-size rows - on lists
    of 0 ... 1,000 items with the product's grids and with 1, 2 and 3 workgroups per launch (every further window of items then comes
    from the `take` counter): every listed item's fout holds the oracle's seven numbers and over = 0, whichever launch decided it;
    every other slot and the guards on both sides keep the fill; the first retry list is exactly the set of flanks whose band is 36
    columns wide or whose packed run count overflows, the second the same at 64; C_OVERFLOW stays 0.
    Time limit 60 s (the whole test measured on the MI355X: 0.54 s, 50 cases in one child, and 0.68 s for the pool's
    oracle and host forms)."""
    items, want, r1, r2 = pool
    ids = np.array([f["item"] for f in items], np.int64)
    cases = _extend_cases(pool)
    arrays = base + [np.array([len(cases)], np.uint32)]
    for _, grid, sel in cases:
        arrays += [ids[sel].astype(np.uint32), np.array(grid, np.int32)]
    out = oc.run_child(harness, "extend", arrays, tmp_path, 60)
    n = len(world.tasks)
    reached = [0, 0, 0]
    for k, (name, grid, sel) in enumerate(cases):
        fout = np.frombuffer(out[4 * k], gc.FOUT)
        retry, retry2, counters = (_u32(b) for b in out[4 * k + 1:4 * k + 4])
        assert len(fout) == 2 * n + 32
        listed = np.zeros(2 * n + 32, bool)
        listed[16 + ids[sel]] = True
        rest = fout[~listed]
        assert all((rest[f] == SENTINEL).all() for f in gc.FOUT.names), "%s: a slot of no listed item, or a guard, was written" % name
        got = fout[16 + ids[sel]]
        for c, f in enumerate(gc.FOUT.names[:7]):
            bad = np.flatnonzero(got[f] != want[sel, c])
            assert not len(bad), "%s: %s of item %d (%s) is %d, the oracle says %d" % (name, f, ids[sel][bad[0]], items[sel[bad[0]]]["cls"], got[f][bad[0]], want[sel[bad[0]], c])
        assert not got["over"].any(), name
        assert counters[gc.C_OVERFLOW] == 0 and counters[gc.C_ITEMS] == len(sel), name
        for lst, cnt, leaves, what in ((retry, gc.C_RETRY, r1, "first"), (retry2, gc.C_RETRY2, r2, "second")):
            m = int(counters[cnt])
            assert sorted(lst[:m].tolist()) == sorted(ids[sel][leaves[sel]].tolist()), "%s: the %s retry list" % (name, what)
            assert (lst[m:] == 0xFFFFFFFF).all(), name
        if grid[0] and len(sel):
            assert counters[gc.C_GTAKE] >= max(1, -(-len(sel) // 64) - grid[0]), name
            if r1[sel].any():
                assert counters[gc.C_GTAKE2] >= 1, name
        reached = [reached[0] + len(sel), reached[1] + int(r1[sel].sum()), reached[2] + int(r2[sel].sum())]
    print("%d cases: %d flanks extended, %d went to the second window, %d to k_gapped" % (len(cases), *reached))
    assert reached[2] >= 24


def _expected_hsps(world, loge_r, loge_thr):
    """mc_make_hsp restated on the task records and the oracle's numbers of each segment's two flanks: the kept HSPs."""
    res = gc.segment_results(world)
    rows = []
    for t in world.tasks:
        if t["read"] == gc.TASK_NONE:
            continue
        frame = t["chrono"] >> 25
        score, nmatch, alnlen, gaps, gapcols = t["score"], t["nmatch"], t["qfwd"] + t["L"] + t["qbwd"], 0, 0
        ext = [[t["qfwd"], t["qfwd"]], [t["qbwd"], t["qbwd"]]]
        for side, o in enumerate(res[world.segment(t)]):
            if o is not None and o[0] > 0:
                score += o[0]; nmatch += o[3]; ext[side][0] += o[1]; ext[side][1] += o[2]; alnlen += o[4]; gaps += o[5]; gapcols += o[6]
        if not 0 <= score < len(loge_r):
            continue
        le = loge_r[score]
        if not score > 30 and not loge_thr > le:                     # the keep rule (CalRes 0x4078e4)
            continue
        (qfwd, dfwd), (qbwd, dbwd) = ext
        qb, db, L = t["qp"], t["dp"], t["L"]
        if frame <= 2:
            qnts, qnte = (qb - qbwd) * 3 + frame + 1, (qb + qfwd + L) * 3 + frame
        else:
            qnts = gc.L_NT - (qb - qbwd) * 3 - (frame - 3)
            qnte = qnts + 1 - (qfwd + qbwd + L) * 3
        rows.append((t["read"], t["chrono"], t["sidx"], score, frame, alnlen, alnlen - nmatch - gapcols, gaps, nmatch, qb - qbwd, qb + qfwd - 1 + L, db - dbwd,
                     db + dfwd - 1 + L, qnts, qnte, le))
    return np.array(rows, oc.HSP)


def _canon(rec):
    return np.sort(rec, order=list(oc.HSP.names))


def test_chain_and_emit(harness, world, base, tmp_path):
    """dedupe, sort, extend and k_gap_emit in the product's order with the product's grids: every task that is no padding has exactly
    one HSP or - by the keep rule of mc_make_hsp, restated here - none; its integer fields follow from the task record and the
    oracle's numbers of its group's two flanks (a flank that gains nothing adds nothing, whatever the leader's slot holds), its log E is
    loge_r[score]; hkeys and hplace belong to the record beside them; low and cand are marked for exactly the reads with a kept HSP
    under the E-value threshold / at the candidate score.  With the pool one short of the kept HSPs C_OVERFLOW is 2, C_HSPS still
    counts them all and nothing is written behind the pool.  Time limit 60 s per child (the whole test measured on the MI355X: 0.65 s, two children)."""
    n = len(world.tasks)
    slots = np.array([gc.table_slots(n), 2 * n], np.uint32)
    thr = 40.0
    out = oc.run_child(harness, "chain", base + [slots, np.array([thr])], tmp_path, 60)
    loge_r, bits_r, loge_thr = np.frombuffer(out[11], "<f8"), np.frombuffer(out[12], "<f8"), float(np.frombuffer(out[13], "<f8")[0])
    want = _expected_hsps(world, loge_r, loge_thr)
    tasks = sum(t["read"] != gc.TASK_NONE for t in world.tasks)
    counters = _u32(out[5])
    nh = int(counters[gc.C_HSPS])
    print("%d tasks, %d HSPs kept, %d not" % (tasks, len(want), tasks - len(want)))
    assert 0 < len(want) < tasks and nh == len(want) and counters[gc.C_OVERFLOW] == 0
    pool_, hkeys, hplace = np.frombuffer(out[0], oc.HSP), np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<u8")
    got = pool_[:nh]
    assert np.array_equal(_canon(got), _canon(want))
    assert all((np.frombuffer(out[k], "u1") == 0xEE).all() for k in (8, 9, 10)) and (np.frombuffer(out[0], "u1")[nh * 48:] == 0xEE).all()
    u = np.uint64
    key = (got["read"].astype(u) << u(43)) | (got["sidx"].astype(u) << u(28)) | got["chrono"].astype(u)
    place = ((got["score"].astype(u) << u(41)) | (got["frame"].astype(u) << u(38)) | (got["qaas"].astype(u) << u(30)) | (got["qaae"].astype(u) << u(22))
             | (got["ds"].astype(u) << u(11)) | got["de"].astype(u))
    assert np.array_equal(hkeys[:nh], key) and np.array_equal(hplace[:nh], place)
    low, cand = np.frombuffer(out[3], "u1"), np.frombuffer(out[4], "u1")
    want_low, want_cand = np.zeros(gc.NREADS, np.uint8), np.zeros(gc.NREADS, np.uint8)
    want_low[want["read"][want["loge"] < loge_thr]] = 1
    want_cand[want["read"][bits_r[want["score"]] >= thr]] = 1
    assert 0 < want_cand.sum() < want_low.sum() < gc.NREADS and np.array_equal(low, want_low) and np.array_equal(cand, want_cand)
    # the pool one short
    slots[1] = len(want) - 1
    out = oc.run_child(harness, "chain_short", base + [slots, np.array([thr])], tmp_path, 60, verb="chain")
    counters = _u32(out[5])
    assert counters[gc.C_OVERFLOW] == 2 and counters[gc.C_HSPS] == len(want)
    assert all((np.frombuffer(out[k], "u1") == 0xEE).all() for k in (8, 9, 10))
    short = np.frombuffer(out[0], oc.HSP)
    assert len(short) == len(want) - 1
    kept, all_ = [tuple(r) for r in short.tolist()], {tuple(r) for r in want.tolist()}
    assert len(set(kept)) == len(kept) and set(kept) <= all_
