"""Twelve seed waves per CU beside a lookahead (csrc/mc_stages.h: mc_enumerate_launch; mc_hip.hip: range_begin): a
mc_range_begin that issues the translation of the range it expects next launches k_enumerate_q as ONE workgroup of twelve waves per CU
where that translation is the narrow form (reads up to 191 bp), so that eight translation waves fit beside it instead of six;
everywhere else the kernel keeps its sixteen waves per CU.  The launch shape changes, the results may not: after every range_end of a
stream of ranges the rows, the best hits and the counts - and, at the one range per run where they are looked at, the frames - are
those mc_run_range (sixteen waves) gives for that range on a fresh engine.  debug_stage() gives a lookahead up (it waits for its kernel
and discards it) and is refused while a range is in flight, so each case runs its stream up to range k, looks there, between the end of
range k and the begin of the range behind it, and starts again for the next k (tests/test_gpu_ahead_background.py).

Three ranges whose last translation workgroup is a partial one: 20,000 / 20,000 / 20,007 reads of 150 bp (narrow; more workgroups than
the 256 of the twelve-wave grid) and 2,000 / 2,000 / 2,007 reads of 100 bp (narrow; a grid of 167 workgroups of twelve waves, the last
one partly idle) and of 240 bp (wide: sixteen waves).  debug_stage(7) is the witness: waves per workgroup x workgroups per CU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {150: [(0, 20000), (20000, 20000), (40000, 20007)],
         100: [(0, 2000), (2000, 2000), (4000, 2007)],
         240: [(0, 2000), (2000, 2000), (4000, 2007)]}
COUNTS = ("reads", "seed_tasks", "hsps", "gap_tasks", "rows", "classified")
STAGES = ("ms_translate", "ms_seed", "ms_eval", "ms_gapped", "ms_sort", "ms_finish")
TASK_NONE = 0xFFFFFFFF                                                  # MC_TASK_NONE: the padding that closes a partly used block of the seed hits' pool


def _fields_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def _engine(length):
    """(the classification parameters of the nearest length the model lists: the same on both sides of every comparison)"""
    from microbecensus_amd import _native
    model = _native.load_model()
    eng = _native.Engine(device=0)
    near = min(model["pars"], key=lambda k: (abs(int(k) - length), int(k)))
    eng.set_run(length, model["pars"][near], model["families"])
    return eng


def _shape(eng):
    return int(eng.debug_stage(7).reshape(-1).view("<u4")[0])


def _seed_hits(eng):
    """the seed kernel's hits (McSeedTask: four words, the first the read), padding dropped, sorted"""
    t = eng.debug_stage(1).reshape(-1, 16).view("<u4")
    t = t[t[:, 0] != TASK_NONE]
    return t[np.lexsort(t.T[::-1])]


def _result(eng, look=True):
    """(rows, best hits and counts first: debug_stage gives the lookahead up, and nothing else may depend on that)"""
    out = {"rows": eng.rows(), "best": eng.best_hits(), "stats": eng.stats()}
    out["shape"] = _shape(eng) if look else None
    out["hits"] = _seed_hits(eng) if look else None
    out["frames"] = eng.debug_stage(0) if look else None
    return out


def _same(got, want, what=""):
    assert _fields_equal(got["rows"], want["rows"]), what
    assert _fields_equal(got["best"], want["best"]), what
    assert all(got["stats"][k] == want["stats"][k] for k in COUNTS), (what, got["stats"], want["stats"])
    if got["frames"] is not None:
        assert got["frames"].shape == want["frames"].shape and np.array_equal(got["frames"], want["frames"]), what
        assert got["hits"].shape == want["hits"].shape and np.array_equal(got["hits"], want["hits"]), what   # (the same multiset)


def _times_add_up(st):
    assert all(st[k] >= 0.0 for k in STAGES), st
    assert abs(sum(st[k] for k in STAGES) - st["ms_total"]) <= 1e-3 * max(1.0, st["ms_total"]), st


class Setting:
    """the reads of one length, and mc_run_range of a range of them on a fresh engine - once per range and setting, shared by the
    module's tests and never changed"""

    def __init__(self, length):
        from microbecensus_amd import synth
        self.length, self.ranges = length, CASES[length]
        self.n = sum(c for _, c in self.ranges)
        self.reads = synth.GenomeReads(device="cpu", seed=20261001).single(self.n, length).numpy()
        self.known = {}

    def want(self, first, count, best_only=False):
        key = (first, count, best_only)
        if key not in self.known:
            eng = _engine(self.length)
            try:
                eng.set_best_hits_only(best_only)
                eng.upload(self.reads)
                eng.run_range(first, count, first)
                self.known[key] = _result(eng)
            finally:
                eng.close()
        return self.known[key]


@pytest.fixture(scope="module")
def settings():
    known = {}

    def get(length):
        if length not in known:
            known[length] = Setting(length)
        return known[length]
    return get


@pytest.fixture()
def engine_of(settings):
    """an engine whose pools hold the whole set, so that no range of a test replaces the frame buffers"""
    made = []

    def make(length):
        s = settings(length)
        e = _engine(length)
        made.append(e)
        e.upload(s.reads)
        e.run_range(0, s.n, 0)
        return e, s
    yield make
    for e in made:
        e.close()


def _stream_to(eng, ranges, k):
    """end(i), begin(i + 1), results of i - as mc_search and the bench issue their ranges - up to the end of range k and the begin of
    the range behind it; returns the results of range k, frames, seed hits and witness included, looked at between its end and that
    begin"""
    eng.debug_stage(5)                                                  # (a lookahead left by the stream before is given up: every stream starts from none)
    eng.range_begin(ranges[0][0], ranges[0][1], ranges[0][0])
    for i in range(k + 1):
        eng.range_end()
        _times_add_up(eng.stats())
        if i == k:
            got = _result(eng)
        if i + 1 < len(ranges):
            eng.range_begin(ranges[i + 1][0], ranges[i + 1][1], ranges[i + 1][0])
        if i < k:
            _result(eng, look=False)
    if k + 1 < len(ranges):
        eng.range_end()
        _times_add_up(eng.stats())
    assert eng.ranges_in_flight() == 0
    return got


def _check_stream(eng, s, ranges, shapes, best_only=False):
    for k in range(len(ranges)):
        got = _stream_to(eng, ranges, k)
        _same(got, s.want(ranges[k][0], ranges[k][1], best_only), (s.length, ranges, k))
        assert got["shape"] == shapes[k], (s.length, ranges, k, got["shape"])


def _beside(length):
    return 12 if length <= 191 else 16


@pytest.mark.parametrize("best_only", [False, True], ids=["rows", "best_only"])
@pytest.mark.parametrize("length", sorted(CASES))
def test_contiguous_ranges(engine_of, length, best_only):
    """ranges 0 and 1 issue a lookahead beside their seed kernel - twelve waves per CU where it is the narrow form; range 2 is the
    set's last and issues none"""
    eng, s = engine_of(length)
    eng.set_best_hits_only(best_only)
    _check_stream(eng, s, s.ranges, shapes=[_beside(length), _beside(length), 16], best_only=best_only)


@pytest.mark.parametrize("length", sorted(CASES))
def test_a_walk_that_defeats_the_prediction(engine_of, length):
    """0, 2, 1: the lookahead range 0 issued (range 1) is never taken and range 2 waits for its kernel; nothing follows 2; 1 is not
    what anybody expected and expects 2.  The results are the yardstick's and nothing is left in flight."""
    eng, s = engine_of(length)
    r = s.ranges
    _check_stream(eng, s, [r[0], r[2], r[1]], shapes=[_beside(length), 16, _beside(length)])
    assert eng.ranges_in_flight() == 0


@pytest.mark.parametrize("length", sorted(CASES))
def test_run_range_keeps_sixteen_waves(settings, length):
    """mc_run_range issues no lookahead"""
    s = settings(length)
    got = s.want(*s.ranges[0])
    assert got["shape"] == 16
    _times_add_up(got["stats"])


def test_a_search_in_batches_names_its_next_range_at_the_end(engine_of, monkeypatch):
    """Engine.search over three batches (mc_search: run_stream tells range_end the next range, whose lookahead runs behind the gapped
    stage, not beside a seed kernel): sixteen waves, and the rows are those of the whole set in one range"""
    eng, s = engine_of(100)
    want = _result(eng, look=False)                                     # (the fixture's run_range of the whole set)
    monkeypatch.setenv("MC_STREAM_BATCH", "2500")
    rows, best = eng.search(s.reads)
    assert _fields_equal(rows, want["rows"]) and _fields_equal(best, want["best"])
    assert _shape(eng) == 16
