"""The lookahead beside the front of the running range (csrc/mc_ahead.h; mc_hip.hip: range_begin, ahead_issue): mc_range_begin
issues the translation of the range it expects next into the SECOND frame buffer while its own range still reads the first, and the
range_begin that takes it makes that buffer the current one.  After every range_end of a stream of ranges the frames of the range that
ended (debug_stage(0)), its rows and its best hits are those mc_run_range gives for that range on a fresh engine - while the next
lookahead has been in flight in the other buffer since this range began.  tests/test_gpu_ahead.py's 6,007 reads of 100 bp in ranges of
2,000 / 2,000 / 2,007: the last workgroup of a translation is a partial one.

debug_stage() gives a lookahead up (it waits for its kernel and discards it), so a stream that looked at the frames after EVERY end
would never take one: each case runs its stream up to range k, looks at the frames there, and starts again for the next k."""
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


def _result(eng, frames=True):
    """(rows, best hits and counts first: debug_stage gives the lookahead up, and nothing else may depend on that)"""
    out = {"rows": eng.rows(), "best": eng.best_hits(), "stats": eng.stats()}
    out["frames"] = eng.debug_stage(0) if frames else None
    return out


def _same(got, want, what=""):
    assert _fields_equal(got["rows"], want["rows"]), what
    assert _fields_equal(got["best"], want["best"]), what
    assert all(got["stats"][k] == want["stats"][k] for k in COUNTS), (what, got["stats"], want["stats"])
    if got["frames"] is not None:
        assert got["frames"].shape == want["frames"].shape and np.array_equal(got["frames"], want["frames"]), what


@pytest.fixture(scope="module")
def reads():
    from microbecensus_amd import synth
    return synth.GenomeReads(device="cpu", seed=20261001).single(N, L).numpy()


class Yardstick:
    """mc_run_range of a range on a fresh engine, once per range and setting (shared by the module's tests, never changed)"""

    def __init__(self, reads):
        self.reads, self.known = reads, {}

    def __call__(self, first, count, best_only=False):
        key = (first, count, best_only)
        if key not in self.known:
            eng = _engine()
            try:
                _set_run(eng)
                eng.set_best_hits_only(best_only)
                eng.upload(self.reads)
                eng.run_range(first, count, first)
                self.known[key] = _result(eng)
            finally:
                eng.close()
        return self.known[key]


@pytest.fixture(scope="module")
def want(reads):
    return Yardstick(reads)


@pytest.fixture()
def eng(reads):
    """an engine whose pools hold the whole set, so that no range of a test replaces the frame buffers"""
    e = _engine()
    _set_run(e)
    e.upload(reads)
    e.run_range(0, N, 0)
    yield e
    e.close()


def _stream_to(eng, ranges, k):
    """end(i), begin(i + 1), results of i - as mc_search and the bench issue their ranges - up to the end of range k and the begin
    of the range behind it; returns the results of range k, frames included, looked at between its end and that begin"""
    eng.debug_stage(5)                                                  # (a lookahead left by the stream before is given up: every stream starts from none)
    eng.range_begin(ranges[0][0], ranges[0][1], ranges[0][0])
    for i in range(k + 1):
        eng.range_end()
        if i == k:
            got = _result(eng)                                          # (the lookahead range k's begin issued has been running beside all of range k)
        if i + 1 < len(ranges):
            eng.range_begin(ranges[i + 1][0], ranges[i + 1][1], ranges[i + 1][0])
        if i < k:
            _result(eng, frames=False)
    if k + 1 < len(ranges):
        eng.range_end()
    return got


def _check_stream(eng, want, ranges, taken, best_only=False):
    for k in range(len(ranges)):
        before = eng.ranges_translated_ahead()
        got = _stream_to(eng, ranges, k)
        _same(got, want(ranges[k][0], ranges[k][1], best_only), (ranges, k))
        assert eng.ranges_translated_ahead() - before == sum(taken[:k + 1]), (ranges, k)     # (the begin behind range k finds its lookahead given up)


def test_contiguous_ranges(eng, want):
    _check_stream(eng, want, RANGES, taken=[0, 1, 1])


def test_ranges_2_0_1(eng, want):
    """nothing follows 2; 0 is nobody's guess, so the lookahead 2 could not issue leaves the buffers alone; 1 behind 0 is taken"""
    _check_stream(eng, want, [RANGES[2], RANGES[0], RANGES[1]], taken=[0, 0, 1])


def test_a_prefix_and_a_longer_range(eng, want):
    """2,500 reads, then 1,500 of the 2,500 expected behind them (a prefix of the lookahead), then 2,007 where 1,500 were expected: the
    last 507 are translated on top, into the buffer the lookahead wrote"""
    _check_stream(eng, want, [(0, 2500), (2500, 1500), (4000, 2007)], taken=[0, 1, 1])


def test_a_lookahead_never_taken_then_one_that_is(eng, want):
    """behind range 1 the reads from 4,000 are expected and range 0 comes: the lookahead is not taken and the current buffer stays;
    range 1 behind range 0 takes the next one"""
    _check_stream(eng, want, [RANGES[1], RANGES[0], RANGES[1], RANGES[2]], taken=[0, 0, 1, 1])


def test_best_hits_only(eng, want):
    eng.set_best_hits_only(True)
    _check_stream(eng, want, RANGES, taken=[0, 1, 1], best_only=True)


def test_stage_times_add_up(eng):
    """ms_translate is the range's own stream's: its A0, or its wait for the lookahead.  A range that took a whole lookahead translates
    nothing itself, so its ms_translate is a wait alone, and a wait ends with the kernel it waits for, which started before the range
    was begun: at most the background kernel's interval (0.01 ms for the clock's grain).  That interval comes through
    ahead_kernel_ms - positive for a range that took a lookahead, 0 for one that did not.  (The sum of the six stages pins the
    definition of ms_total, no measurement.)"""
    eng.range_begin(*RANGES[0], RANGES[0][0])
    eng.range_end()
    st = eng.stats()
    assert eng.ahead_kernel_ms() == 0.0 and st["ms_translate"] > 0.0
    eng.range_begin(*RANGES[1], RANGES[1][0])
    eng.range_end()
    st = eng.stats()
    assert eng.ahead_kernel_ms() > 0.0
    assert 0.0 <= st["ms_translate"] <= eng.ahead_kernel_ms() + 0.01, (st["ms_translate"], eng.ahead_kernel_ms())
    parts = sum(st[k] for k in ("ms_translate", "ms_seed", "ms_eval", "ms_gapped", "ms_sort", "ms_finish"))
    assert abs(parts - st["ms_total"]) <= 1e-3 * max(1.0, st["ms_total"]), st
