"""The device algorithms of the ordering and finishing kernels (csrc/k_order.h, csrc/k_finish.h), each on inputs built to reach its own
edges - the suite otherwise runs them end to end on real reads only, which never control array lengths around 16 / 64 / the
capacities, segments of exactly 32 HSPs, runs that straddle a wave or workgroup boundary, arrays of nothing but ties or introsort's
depth limit.  tests/emul/device_order.hip includes the library's kernel headers and is built here with the library's flags; every
case is one child process, and every comparison is exact (the outputs are permutations, counts and copied records).

A child that ends by a signal, at its time limit or with a HIP error fails its test with its output, and every later test of the
three unit modules then fails at once without starting anything on the GPU (order_cases.run_child)."""
import numpy as np
import pytest

import order_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_order", tmp_path_factory)


def _run(exe, case, arrays, tmp, limit):
    return oc.run_child(exe, case, arrays, tmp, limit)


@pytest.fixture(scope="module")
def adversary(harness, tmp_path_factory):
    """McIlroy's adversary against mc_std_sort, frozen per length (computed on the host by the harness)."""
    lens = oc.adversary_lengths()
    out = _run(harness, "adversary", [np.array(lens, np.int32)], tmp_path_factory.mktemp("adversary"), 60)
    return {n: np.frombuffer(b, "<f8") for n, b in zip(lens, out)}


def _u32(b):
    return np.frombuffer(b, "<u4")


def _differences(arrs, got, want):
    """Per-array comparison of two concatenated results; the (length, pattern) of the arrays that differ."""
    bad, at = [], 0
    for n, kind, _ in arrs:
        if not np.array_equal(got[at:at + n], want[at:at + n]):
            bad.append((n, kind))
        at += n
    assert at == len(got) == len(want)
    return bad


def test_wave_sort(harness, adversary, tmp_path):
    """mc_wave_std_sort == mc_std_sort, permutation for permutation: a wave per array at k_finish_heavy's LDS layout for the three MAXN.
    Time limit 60 s (the whole test measured: 0.5 s, input generation included)."""
    sets = oc.wave_sort_sets(adversary)
    out = _run(harness, "wave_sort", oc.wave_input(sets), tmp_path, 60)
    print("\n".join(oc.fallback_conditions(sets, [np.frombuffer(out[3 * q + 2], "<i4") for q in range(len(sets))])))
    for q, (maxn, arrs) in enumerate(sets):
        bad = _differences(arrs, _u32(out[3 * q]), _u32(out[3 * q + 1]))
        assert not bad, "MAXN %d: %d arrays differ from mc_std_sort: %s" % (maxn, len(bad), bad[:20])


def test_thread_sorts(harness, adversary, tmp_path):
    """mc_std_sort_inl and mc_heapsort_inl on a thread's own LDS stretch, placed as k_finish<32, 96> and k_finish<128, 16> place it,
    every lane of a wave with another length.  Time limit 60 s (the whole test measured: 0.3 s, input generation included)."""
    sets = oc.thread_sorts_sets(adversary)
    arrays = [np.uint32(len(sets))]
    for items, arrs in sets:
        off, keys = oc.pack([k for _, _, k in arrs], np.float64)
        arrays += [np.uint32(items), off, keys]
    out = _run(harness, "thread_sorts", arrays, tmp_path, 60)
    for q, (items, arrs) in enumerate(sets):
        for h, name in enumerate(("mc_std_sort_inl", "mc_heapsort_inl")):
            bad = _differences(arrs, _u32(out[4 * q + 2 * h]), _u32(out[4 * q + 2 * h + 1]))
            print("%s, %d items per thread: %d arrays, %d differ" % (name, items, len(arrs), len(bad)))
            assert not bad, "%s, %d items per thread: %s" % (name, items, bad[:20])


def test_mergesort(harness, tmp_path):
    """mc_group_mergesort<64 / 256 / 1024> in k_order_heavy's two LDS buffers == std::sort, m = 64 ... the kernel's capacity.
    Time limit 60 s (the whole test measured: 0.4 s, input generation included)."""
    sets = oc.mergesort_sets()
    arrays = [np.uint32(len(sets))]
    for cap, arrs in sets:
        off, items = oc.pack([v for _, _, v in arrs], np.uint64)
        arrays += [np.uint32(cap), off, items]
    out = _run(harness, "mergesort", arrays, tmp_path, 60)
    for q, (cap, arrs) in enumerate(sets):
        got, want = np.frombuffer(out[2 * q], "<u8"), np.frombuffer(out[2 * q + 1], "<u8")
        assert np.array_equal(want, np.concatenate([np.sort(v) for _, _, v in arrs]))
        bad = _differences(arrs, got, want)
        print("capacity %d: %d arrays of %d ... %d items, %d differ" % (cap, len(arrs), arrs[0][0], arrs[-1][0], len(bad)))
        assert not bad, "capacity %d: %s" % (cap, bad)


def test_order(harness, tmp_path):
    """k_order_lists, k_order_light, the three k_order_heavy and k_order_copy on synthetic segments == mc_build_stacks on every read's
    sorted records (test_order_host.py holds that to CalRes' rule restated).  Time limit 60 s (the whole test measured: 1.4 s, input generation included)."""
    pool, slots, heads, low, reads = oc.order_case()
    want_marked = oc.expected_marks(pool, slots, heads, low)
    lens = np.array([n for n, _, _ in reads])
    light, small, mid = oc.BIN_LIGHT, oc.ORDER_CAPS[0], oc.ORDER_CAPS[1]
    kernel = np.where(lens == 0, -1, np.where(lens <= light, 0, np.where(lens <= small, 1, np.where(lens <= mid, 2, 3))))
    # the conditions on the inputs
    later_best = 0
    for r in np.flatnonzero(want_marked)[:60]:
        seg = pool[slots[heads[r]:heads[r + 1]]]
        o = sorted(range(len(seg)), key=lambda k: (seg["sidx"][k], seg["chrono"][k], k))
        s = seg[o]
        same = (s["sidx"][1:] == s["sidx"][:-1]) & (oc.place_words(s)[1:] == oc.place_words(s)[:-1])
        later_best += int((same & (s["score"][1:] > s["score"][:-1])).sum())
    assert later_best > 0, "no run whose best member is not its first"
    for k, name in enumerate(("k_order_light", "k_order_heavy<64>", "k_order_heavy<256>", "k_order_heavy<1024>")):
        mine = kernel == k
        counts = (int(mine.sum()), int((mine & want_marked).sum()), int((mine & ~want_marked).sum()), int((mine & want_marked & (low == 0)).sum()))
        print("%s: %d reads, %d marked, %d unmarked, %d marked though not by low" % ((name,) + counts))
        assert counts[0] >= 20 and counts[1] > 0 and counts[2] > 0 and counts[3] > 0, name
    assert {(n, kind) for n, kind, _ in reads} >= {(light, "last_starts_subject"), (light, "last_starts_run")}
    blocks = [set(kernel[b:b + 64]) for b in range(0, len(reads), 64)]
    assert any(0 in b and -1 in b and len(b & {1, 2, 3}) > 0 for b in blocks), "no block of 64 reads with light, heavy and empty ones"

    out = _run(harness, "order", [pool, slots, heads, low], tmp_path, 60)
    v, nv, nrow, counters = np.frombuffer(out[0], oc.HSP), _u32(out[1]), _u32(out[2]), _u32(out[3])
    lists = [_u32(out[4]), _u32(out[5]), _u32(out[6])]
    vexp, vn = np.frombuffer(out[7], oc.HSP), _u32(out[8])
    for k, (cnt, take) in enumerate(((oc.C_ORDER, oc.C_OTAKE), (oc.C_ORDER2, oc.C_OTAKE2), (oc.C_ORDER3, oc.C_OTAKE3))):
        assert sorted(lists[k][:counters[cnt]]) == list(np.flatnonzero(kernel == k + 1)), "list of heavy kernel %d" % (k + 1)
        assert counters[take] >= counters[cnt]
    assert np.array_equal(nrow, want_marked.astype(np.uint32)), "marked reads: %s" % [reads[r] for r in np.flatnonzero(nrow != want_marked)[:10]]
    bad = []
    for r in np.flatnonzero(want_marked):
        a, k = int(heads[r]), int(vn[r])
        same = nv[r] == vn[r] and np.array_equal(v["read"][a:a + k], vexp["read"][a:a + k]) and all(np.array_equal(v[f][a:a + k], vexp[f][a:a + k]) for f in oc.COMPARED_FIELDS)
        if not same:
            bad.append(reads[r])
    print("%d marked reads compared record by record, %d stacked HSPs, %d differ" % (int(want_marked.sum()), int(vn[want_marked].sum()), len(bad)))
    assert not bad, bad[:20]


def test_heap_lanes(harness, tmp_path):
    """k_heap_lanes with its product geometry == mc_heapsort on the same words keyed by their upper halves; unflagged entries and reads
    with fewer than two rows keep their words.  Time limit 60 s (the whole test measured: 0.4 s, input generation included)."""
    sets = oc.heap_lanes_sets()
    arrays = [np.uint32(len(sets))]
    for s in sets:
        arrays += [s["heads"], s["rows"], s["heavy_first"], s["order"], np.concatenate(s["words"]).astype(np.uint32)]
    out = _run(harness, "heap_lanes", arrays, tmp_path, 60)
    for q, s in enumerate(sets):
        got, host = _u32(out[2 * q]), _u32(out[2 * q + 1])
        flagged = np.zeros(len(s["rows"]), bool)
        flagged[s["heavy_first"][s["heavy_first"] >> 31 == 1] & 0x7FFFFFFF] = True
        at, bad, nsorted = 0, [], 0
        for r, w in enumerate(s["words"]):
            want = host[at:at + len(w)] if flagged[r] and len(w) >= 2 else w
            nsorted += int(flagged[r] and len(w) >= 2)
            if not np.array_equal(got[at:at + len(w)], want):
                bad.append((r, len(w), bool(flagged[r])))
            at += len(w)
        nheavy = len(s["heavy_first"])
        print("nheavy %d: %d heap sorts, %d unflagged, rows %s, rounds of the busiest wave %d, %d differ" % (
            nheavy, nsorted, int(nheavy - flagged.sum()), sorted(set(s["rows"][flagged].tolist()))[:12], -(-nheavy // (256 * 64)), len(bad)))
        assert not bad, bad[:20]
        assert nsorted > 0 or nheavy == 1


def test_counting_sorts(harness, tmp_path):
    """k_heavy_order and k_heap_order: the output is a permutation of the input list with non-increasing keys under the kernel's own
    key rule (any order among equal keys).  Time limit 60 s (the whole test measured: 0.3 s, input generation included)."""
    sets = oc.counting_sorts_sets()
    arrays = [np.uint32(len(sets))]
    for s in sets:
        arrays += [np.array([s["kind"], s["shift"]], np.uint32)] + ([s["list"], s["heavy"], s["nv"]] if s["kind"] == 0 else [s["heavy_first"], s["rows"]])
    out = _run(harness, "counting_sorts", arrays, tmp_path, 60)
    for q, s in enumerate(sets):
        got = _u32(out[q])
        if s["kind"] == 0:
            assert np.array_equal(np.sort(got), np.sort(s["list"])), (q, s["keys"])
            key = np.minimum(s["nv"][s["heavy"][got] & 0x7FFFFFFF] >> s["shift"], 511)
        else:
            assert np.array_equal(np.sort(got), np.arange(len(s["heavy_first"]))), (q, s["keys"])
            e = s["heavy_first"][got]
            key = np.where(e >> 31 == 1, np.minimum(s["rows"][e & 0x7FFFFFFF], oc.MAX_M8), 0)
        assert np.all(key[1:].astype(np.int64) <= key[:-1].astype(np.int64)), (q, s["kind"], s["keys"], len(got))
    print("%d lists sorted: sizes %s, keys %s" % (len(sets), oc.COUNT_SIZES, oc.COUNT_KEYS))


def test_bins_and_scan(harness, tmp_path):
    """k_bin_count == numpy.bincount; behind mc_scan_u32 and k_bin_scatter every read's segment holds exactly its (key, place, slot)
    and cur ends at the next read's start; mc_scan_u32 alone == numpy.cumsum up to 4096 * 1024 counts, and one more is refused on
    the host.  Time limit 60 s (the whole test measured: 0.4 s, input generation included)."""
    bins, scans = oc.bins_sets(), oc.scan_sets()
    arrays = [np.array([len(bins), len(scans), 1], np.uint32)]
    for s in bins:
        arrays += [np.array([s["nreads"], s["use_cand"]], np.uint32), s["hkeys"], s["hplace"], s["cand"]]
    for s in scans:
        arrays += [np.array([s["inplace"]], np.uint32), s["values"]]
    arrays += [np.uint32(oc.SCAN_REFUSED)]
    out = _run(harness, "bins_and_scan", arrays, tmp_path, 60)
    for q, s in enumerate(bins):
        cnt, start, end = (_u32(out[6 * q + k]) for k in range(3))
        keys, places, slots = np.frombuffer(out[6 * q + 3], "<u8"), np.frombuffer(out[6 * q + 4], "<u8"), _u32(out[6 * q + 5])
        read = (s["hkeys"] >> np.uint64(43)).astype(np.int64)
        valid = s["hkeys"] != np.uint64(0xFFFFFFFFFFFFFFFF)
        if s["use_cand"]:
            valid &= s["cand"][np.where(valid, read, 0)] != 0
        want = np.bincount(read[valid], minlength=s["nreads"])
        assert np.array_equal(cnt, want), q
        assert np.array_equal(start, np.cumsum(want) - want) and np.array_equal(end, np.cumsum(want)), q
        total = int(want.sum())
        assert np.array_equal(s["hkeys"][slots[:total]], keys[:total]) and np.array_equal(s["hplace"][slots[:total]], places[:total]), q
        assert np.array_equal(np.sort(slots[:total]), np.flatnonzero(valid)), q            # every valid HSP once ...
        assert np.array_equal((keys[:total] >> np.uint64(43)).astype(np.int64), np.repeat(np.arange(s["nreads"]), want)), q   # ... in its read's segment
        assert np.all(slots[total:] == 0xFFFFFFFF), q
        print("bins %d: %d pool slots, %d valid, %d reads with HSPs of %d, filter %d" % (q, len(valid), total, int((want > 0).sum()), s["nreads"], s["use_cand"]))
    at = 6 * len(bins)
    for q, s in enumerate(scans):
        want = (np.cumsum(s["values"], dtype=np.uint64) - s["values"]).astype(np.uint32)
        assert np.array_equal(_u32(out[at + q]), want), len(want)
    print("scan: n = %s" % (oc.SCAN_SIZES,))
    rc, msg = np.frombuffer(out[at + len(scans)], "<i4"), out[at + len(scans) + 1].decode()
    assert rc[0] == -1 and msg == "scan of more than 4 M counts", (rc, msg)
