"""The lookahead (csrc/mc_ahead.h; mc_hip.hip: range_end, range_begin): mc_range_end issues the translation of the range it expects
next beside the ordering and finishing kernels of the range that ends, and mc_range_begin uses those frames where they are the begun
range's.  Whatever is guessed, begun, changed or overflowing in between, the results are those of mc_run_range per range on a fresh
engine: rows, best hits, the per-range counts and - where noted - the frames themselves.  6,007 reads of 100 bp: the last workgroup of
the translation (10 reads each) is a partial one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, L = 6007, 100
RANGES = [(0, 2000), (2000, 2000), (4000, 2007)]
COUNTS = ("reads", "seed_tasks", "hsps", "gap_tasks", "rows", "classified")


def _fields_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def _engine():
    from microbecensus_amd import _native
    return _native.Engine(device=0)


def _set_run(eng, length=L):
    from microbecensus_amd import _native
    model = _native.load_model()
    eng.set_run(length, model["pars"][str(length)], model["families"])


def _result(eng, frames=False):
    return {"rows": eng.rows(), "best": eng.best_hits(), "stats": eng.stats(), "frames": eng.debug_stage(0) if frames else None}


def _same(got, want, what=""):
    assert _fields_equal(got["rows"], want["rows"]), what
    assert _fields_equal(got["best"], want["best"]), what
    assert all(got["stats"][k] == want["stats"][k] for k in COUNTS), (what, got["stats"], want["stats"])


def _yardstick(reads, ranges, length=L, best_only=False, frames=False):
    """mc_run_range per range on a fresh engine"""
    eng = _engine()
    try:
        _set_run(eng, length)
        eng.set_best_hits_only(best_only)
        eng.upload(reads)
        out = []
        for first, count in ranges:
            eng.run_range(first, count, first)
            out.append(_result(eng, frames))
        return out
    finally:
        eng.close()


def _stream(eng, ranges):
    """end(i), begin(i + 1), results of i - as mc_search and the bench issue their ranges"""
    out = []
    eng.range_begin(ranges[0][0], ranges[0][1], ranges[0][0])
    for i in range(len(ranges)):
        eng.range_end()
        if i + 1 < len(ranges):
            eng.range_begin(ranges[i + 1][0], ranges[i + 1][1], ranges[i + 1][0])
        out.append(_result(eng))
    return out


@pytest.fixture(scope="module")
def reads():
    from microbecensus_amd import synth
    return synth.GenomeReads(device="cpu", seed=20261001).single(N, L).numpy()


@pytest.fixture(scope="module")
def other_reads():
    from microbecensus_amd import synth
    return synth.GenomeReads(device="cpu", seed=20261001).single(N, L, first=1 << 20).numpy()


@pytest.fixture(scope="module")
def want(reads):
    """the three contiguous ranges, and the whole set as one range (its frames too)"""
    per = _yardstick(reads, RANGES + [(0, N)], frames=True)
    assert sum(len(w["rows"]) for w in per[:3]) > 1000 and sum(len(w["best"]) for w in per[:3]) > 20
    return {"ranges": per[:3], "all": per[3]}


@pytest.fixture()
def eng(reads):
    """An engine whose pools hold the whole set (one range over all of it): a range larger than the pools replaces them, and the
    frames of a lookahead with them - test_pools_that_grow_give_the_lookahead_up."""
    e = _engine()
    _set_run(e)
    e.upload(reads)
    e.run_range(0, N, 0)
    yield e
    e.close()


def test_contiguous_ranges_are_translated_ahead(eng, want):
    got = _stream(eng, RANGES)
    for g, w, r in zip(got, want["ranges"], RANGES):
        _same(g, w, r)
    assert eng.ranges_translated_ahead() == 2


def test_pools_that_grow_give_the_lookahead_up(reads, want):
    """a fresh engine: its pools are those of the first range, 2,000 reads - the third range, 2,007, replaces them"""
    e = _engine()
    try:
        _set_run(e)
        e.upload(reads)
        got = _stream(e, RANGES)
        for g, w, r in zip(got, want["ranges"], RANGES):
            _same(g, w, r)
        assert e.ranges_translated_ahead() == 1
    finally:
        e.close()


def test_uneven_and_shrinking_ranges(eng, reads):
    ranges = [(0, 2500), (2500, 1500), (4000, 2007)]                   # the second is a prefix of the lookahead (2,500 reads from 2,500)
    got = _stream(eng, ranges)
    for g, w, r in zip(got, _yardstick(reads, ranges), ranges):
        _same(g, w, r)
    assert eng.ranges_translated_ahead() == 2                          # (1,500 of the third range's 2,007 reads were expected: the last 507 on top)


def test_ranges_2_0_1(eng, want):
    """Nothing follows 2, and 0 is not what anybody expected; 1 behind 0 IS the contiguous range - the one step of this order that the
    rule covers, the same step as in test_contiguous_ranges_are_translated_ahead."""
    order = [2, 0, 1]
    got = _stream(eng, [RANGES[k] for k in order])
    for g, k in zip(got, order):
        _same(g, want["ranges"][k], RANGES[k])
    assert eng.ranges_translated_ahead() == 1


def test_ranges_out_of_order_use_no_lookahead(eng, reads, want):
    """2, 1, 0, then a range that overlaps the expected one at another start: no step is covered, and the count stays"""
    order = [2, 1, 0]
    got = _stream(eng, [RANGES[k] for k in order])
    for g, k in zip(got, order):
        _same(g, want["ranges"][k], RANGES[k])
    # 0 ended last: 2,000 reads from 2,000 are expected
    eng.range_begin(2500, 1500, 2500)
    eng.range_end()
    _same(_result(eng), _yardstick(reads, [(2500, 1500)])[0])
    assert eng.ranges_translated_ahead() == 0


@pytest.mark.parametrize("change", ["upload", "set_run", "best_hits_only", "counting"])
def test_a_change_between_end_and_begin(eng, reads, other_reads, change):
    eng.range_begin(0, 2000, 0)
    eng.range_end()                                                    # (reads 2,000 .. 3,999 of `reads` at 100 bp are being translated)
    used = eng.ranges_translated_ahead()
    if change == "upload":                                             # the same buffer, the same address, the same count: other reads
        eng.upload(other_reads)
        w = _yardstick(other_reads, [RANGES[1]])[0]
    elif change == "set_run":
        from microbecensus_amd import synth
        reads150 = synth.GenomeReads(device="cpu", seed=20261001).single(N, 150).numpy()
        _set_run(eng, 150)
        eng.upload(reads150)
        w = _yardstick(reads150, [RANGES[1]], length=150)[0]
    elif change == "best_hits_only":
        eng.set_best_hits_only(True)
        w = _yardstick(reads, [RANGES[1]], best_only=True)[0]
    else:
        eng.set_counting(True)
        eng.set_counting(False)
        w = _yardstick(reads, [RANGES[1]])[0]
    eng.range_begin(RANGES[1][0], RANGES[1][1], RANGES[1][0])
    eng.range_end()
    _same(_result(eng), w, change)
    if change in ("upload", "set_run", "counting"):
        assert eng.ranges_translated_ahead() == used                   # (dropped: the frames were other reads', another length's, or given up)


def test_frames_after_run_range_are_that_range_s(eng, want):
    eng.range_begin(*RANGES[2], RANGES[2][0])
    eng.range_end()                                                    # the last range of the set: nothing follows it
    eng.run_range(0, N, 0)
    g = _result(eng, frames=True)
    _same(g, want["all"])
    assert g["frames"].shape == want["all"]["frames"].shape and np.array_equal(g["frames"], want["all"]["frames"])
    eng.range_begin(*RANGES[0], RANGES[0][0])
    eng.range_end()                                                    # a lookahead of 2,000 reads from 2,000 is in flight: run_range of another range waits for it
    eng.run_range(0, N, 0)
    assert np.array_equal(eng.debug_stage(0), want["all"]["frames"])
    eng.range_begin(*RANGES[0], RANGES[0][0])
    eng.range_end()
    eng.run_range(*RANGES[1], RANGES[1][0])                            # the expected range itself: its frames are the lookahead's
    assert np.array_equal(eng.debug_stage(0), want["ranges"][1]["frames"])
    _same(_result(eng), want["ranges"][1])


def test_contiguous_ranges_best_hits_only(eng, reads):
    eng.set_best_hits_only(True)
    got = _stream(eng, RANGES)
    for g, w, r in zip(got, _yardstick(reads, RANGES, best_only=True), RANGES):
        _same(g, w, r)
        assert len(g["rows"]) == 0
    assert eng.ranges_translated_ahead() == 2


def test_overflow_while_a_lookahead_is_in_flight():
    """A library of nothing but marker genes, as tests/test_gpu_blindspots.py builds it (~290 HSPs a read where the pools hold 58 a read
    and 3.1 M): a range of 30,000 reads overflows them.  mc_range_end has issued the translation of the 30,000 reads behind it by
    then; it returns -2, mc_run_range answers in halves."""
    from microbecensus_amd import _native, synth
    names, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0)
    dense = synth.sample_reads(genome, 60_000, 150, seed=405)
    w = _yardstick(dense, [(0, 30_000)], length=150)[0]
    assert w["stats"]["range_splits"] > 0, "the range did not overflow: the test no longer meets a lookahead in flight at -2"
    e = _engine()
    try:
        _set_run(e, 150)
        e.upload(dense)
        e.range_begin(0, 30_000, 0)
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            e.range_end()
        assert e.ranges_in_flight() == 0
        e.run_range(0, 30_000, 0)
        g = _result(e)
        assert g["stats"]["range_splits"] > 0
        _same(g, w)
    finally:
        e.close()


def test_search_in_batches_looks_ahead(eng, reads, want, monkeypatch):
    monkeypatch.setenv("MC_STREAM_BATCH", "2000")
    before = eng.ranges_translated_ahead()
    rows, best = eng.search(reads)
    st = eng.stats()
    assert _fields_equal(rows, want["all"]["rows"]) and _fields_equal(best, want["all"]["best"])
    assert all(st[k] == want["all"]["stats"][k] for k in COUNTS)
    assert eng.ranges_translated_ahead() > before
