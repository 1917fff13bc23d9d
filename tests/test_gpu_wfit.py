"""The weight fit (training step 5) on the device: mc_weights_mue and mc_fit_weights against the numpy restatement of csrc/mc_wfit.h
(wfit_restated.py) bit for bit, the refusals, the planted problem at the header's defaults, and training end to end with
--fit-weights."""
import gzip
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import wfit_restated as wr
from microbecensus_amd import _native, training
from microbecensus_amd import microbe_census as mc
from test_wfit_host import SHAPES, bits, planted_conditions, table, weight_vectors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_training_library_golden as mk  # noqa: E402

# the shapes of the CPU test, N above 64 (two to four rounds in registers), above 256 (the errors in LDS), a table too large for
# LDS, and the limit
GPU_SHAPES = SHAPES + [(65, 30), (129, 7), (256, 22), (300, 18), (2048, 1), (1000, 32), (wr.MAX_N, 30)]


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine(device=0)
    yield e
    e.close()


@pytest.mark.parametrize("N,F", GPU_SHAPES)
def test_weights_mue_equals_the_restatement(eng, N, F):
    rng = np.random.default_rng(31 * N + F)
    pred, truth = table(rng, N, F, na_columns=(2,) if F > 2 else (), dead=(5, 7) if F > 7 else ())
    K = 3000 if N <= 300 else 600
    W = weight_vectors(rng, K, F)
    pm, keep, _ = wr.mask(pred)
    want = wr.mue(pm, keep, truth, W, chunk=max(1, 400_000 // N))
    got = eng.weights_mue(pred, truth, W)
    print("mc_weights_mue N=%d F=%d K=%d: %d of %d differ, %d infinite, kernel %.3f ms" % (N, F, K, int((bits(got) != bits(want)).sum()), K, int(np.isinf(want).sum()), eng.fit_weights_ms()))
    assert np.array_equal(bits(got), bits(want))
    assert np.isinf(want[0]) and (F == 1 or np.isfinite(want).any())


@pytest.mark.parametrize("N,F", GPU_SHAPES)
def test_fit_equals_the_restatement(eng, N, F):
    rng = np.random.default_rng(53 * N + F)
    pred, truth = table(rng, N, F, na_columns=(1,) if F > 2 else (), dead=(3,) if F > 7 else ())
    C, G = (64, 24) if N <= 300 else (48, 6)
    for seed, L in ((0, 100), (0xFEEDFACE12345678, 150), (7, 500)):
        want_w, want_t = wr.fit(pred, truth, seed, L, C, G)
        w, t = eng.fit_weights(pred, truth, seed, L, C, G)
        print("mc_fit_weights N=%d F=%d seed=%x: mue %.6g -> %.6g, kernels %.3f ms" % (N, F, seed, t[0, 0], t[-1, 0], eng.fit_weights_ms()))
        assert np.array_equal(bits(w), bits(want_w)) and np.array_equal(bits(t.reshape(-1)), bits(want_t.reshape(-1)))
        w2, t2 = eng.fit_weights(pred, truth, seed, L, C, G)
        assert w2.tobytes() == w.tobytes() and t2.tobytes() == t.tobytes()
    w0, t0 = eng.fit_weights(pred, truth, 0, 100, C, 0)
    assert t0.shape == (1, 3) and np.array_equal(bits(w0), bits(np.full(F, 1.0 / F))) and bits(t0[0, 0]) == bits(want_t[0, 0]) and t0[0, 1] == 0.0 and t0[0, 2] == wr.SIGMA0


def test_a_search_that_ends_early(eng):
    rng = np.random.default_rng(3)
    pred, truth = table(rng, 5, 1, na=0.0)
    want_w, want_t = wr.fit(pred, truth, 1, 100, 8, 40)
    w, t = eng.fit_weights(pred, truth, 1, 100, 8, 40)
    assert np.array_equal(bits(w), bits(want_w)) and np.array_equal(bits(t.reshape(-1)), bits(want_t.reshape(-1))) and t[-1, 1] == -1.0


def test_refusals(eng):
    rng = np.random.default_rng(1)
    pred, truth = table(rng, 10, 4)
    W = np.full((2, 4), 0.5)

    def refused(msg, fn, *a):
        with pytest.raises(RuntimeError, match=msg):
            fn(*a)
    big, bt = np.ones((3, 33)), np.ones(3)
    refused("1 to 32 families", eng.fit_weights, big, bt, 0, 100, 8, 2)
    refused("1 to 32 families", eng.weights_mue, big, bt, np.full((1, 33), 0.5))
    refused("1 to 4096 libraries", eng.fit_weights, np.ones((wr.MAX_N + 1, 2)), np.ones(wr.MAX_N + 1), 0, 100, 8, 2)
    refused("1 to 4096 libraries", eng.weights_mue, np.ones((0, 4)), np.ones(0), W)
    refused("65536 candidates", eng.fit_weights, pred, truth, 0, 100, 65537, 2)
    refused("65536 candidates", eng.fit_weights, pred, truth, 0, 100, -1, 2)
    refused("4096 generations", eng.fit_weights, pred, truth, 0, 100, 8, 4097)
    refused("4096 generations", eng.fit_weights, pred, truth, 0, 100, 8, -2)
    for bad in (0.0, -1.0, np.inf, np.nan):
        t = truth.copy(); t[3] = bad
        refused("positive finite", eng.fit_weights, pred, t, 0, 100, 8, 2)
        refused("positive finite", eng.weights_mue, pred, t, W)
    p = pred.copy(); p[2, 1] = -np.inf
    refused("infinite prediction", eng.fit_weights, p, truth, 0, 100, 8, 2)
    refused("infinite prediction", eng.weights_mue, p, truth, W)
    for bad in (-0.1, 1.5, np.nan):
        w = W.copy(); w[1, 2] = bad
        refused(r"outside \[0, 1\]", eng.weights_mue, pred, truth, w)
    # the defaults are selected by C = 0 / G = -1 (a trace of the default length comes back)
    w, t = eng.fit_weights(pred, truth, 0, 100, None, 1)
    assert t.shape == (2, 3)


def test_planted_problem_at_the_defaults(eng):
    pred, truth = wr.planted(1)
    w, trace = eng.fit_weights(pred, truth, 0, 100)
    assert trace.shape == (wr.DEFAULT_G + 1, 3)
    fresh = planted_conditions(w, trace)
    print("planted problem at C=%d G=%d: mue %.6g -> %.6g in sample, %.6g -> %.6g on 150 further libraries; mean weight good %.4g bad %.4g; kernels %.1f ms"
          % (wr.DEFAULT_C, wr.DEFAULT_G, trace[0, 0], trace[-1, 0], fresh[0], fresh[1], w[:wr.PLANTED_GOOD].mean(), w[wr.PLANTED_GOOD:].mean(), eng.fit_weights_ms()))
    pm, keep, _ = wr.mask(pred)
    assert bits(wr.mue(pm, keep, truth, w)[0]) == bits(trace[-1, 0])


def _md5s(d):
    return {f: hashlib.md5(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))}


def test_training_end_to_end(tmp_path, monkeypatch):
    """train(fit_weights=True), scripts/optimize_weights.py and run_pipeline --model on a model with fitted weights; and train()
    without the flag against a second default run, every file by md5.  The grid's coverage sums are accumulated in no fixed order
    (reproducible to 1e-12, the grid's contract: on the device two default runs of train() differed in training_preds.map, md5
    7b78e1a9... against 8cba313b...), so the first run's grid counts are recorded and the later runs are given the same ones - what
    is compared byte for byte is everything train() makes of them, which is all this switch could change."""
    counts = {}
    real = _native.Engine.train_library

    def recorded(self, genome, nreads, seed, library_id, *grid):
        key = (self.read_len, nreads, seed, library_id)
        if key not in counts:
            counts[key] = real(self, genome, nreads, seed, library_id, *grid)
        return counts[key]
    monkeypatch.setattr(_native.Engine, "train_library", recorded)
    genomes_dir = tmp_path / "genomes"
    genomes_dir.mkdir()
    for k in (3, 6, 7, 9):
        name, bases, off = mk.load_genome(k)
        with gzip.open(str(genomes_dir / (name + ".fna.gz")), "wb", compresslevel=1) as f:
            for c in range(len(off) - 1):
                f.write(b">%s_%d\n%s\n" % (name.encode(), c, bases[off[c]:off[c + 1]].tobytes()))
    quiet = dict(xfolds=2, log=lambda *a: None)
    Ls, C, G = [100, 150], 256, 20
    plain = training.train(str(genomes_dir), str(tmp_path / "plain"), Ls, 2, **quiet)
    assert len(counts) == 8
    fitted = training.train(str(genomes_dir), str(tmp_path / "fit"), Ls, 2, fit_weights=True, fit_seed=5, fit_candidates=C, fit_generations=G, **quiet)
    plain2 = training.train(str(genomes_dir), str(tmp_path / "plain2"), Ls, 2, **quiet)
    assert len(counts) == 8
    fams = fitted["families"]
    # the weights written are fit_weights on the training_preds.map written
    rows = training.read_map(str(tmp_path / "fit" / "training_preds.map"), header=True)
    eng = _native.Engine(device=0)
    try:
        weights, mues = training.fit_weights(rows, fams, Ls, eng, 5, C, G)
        tables = training.weight_tables(rows, fams, Ls)
        for L in Ls:
            pred, truth, _ = tables[L]
            ones = eng.weights_mue(pred, truth, np.ones((1, len(fams))))[0]
            got = eng.weights_mue(pred, truth, np.array([[weights["%d_%s" % (L, f)] for f in fams]]))[0]
            print("L=%d: in-sample mue %.6g at 1.0, %.6g fitted (record %s)" % (L, ones, got, fitted["weights_fit"]["mue"][str(L)]))
            assert got <= ones and bits(got) == bits(mues[L][1]) and fitted["weights_fit"]["mue"][str(L)] == [mues[L][0], mues[L][1]]
    finally:
        eng.close()
    assert weights == fitted["weights"] and fitted["weights_fit"]["seed"] == 5 and fitted["weights_fit"]["candidates"] == C and fitted["weights_fit"]["generations"] == G
    assert {k: float(v) for k, v in training.read_map(str(tmp_path / "fit" / "weights.map"))} == weights
    assert any(v != 1.0 / len(fams) for v in weights.values())
    # the command of its own leaves weights.map as it is
    before = _md5s(str(tmp_path / "fit"))
    subprocess.check_call([sys.executable, os.path.join(REPO, "scripts", "optimize_weights.py"), str(tmp_path / "fit"), "--fit-seed", "5", "--fit-candidates", str(C),
                           "--fit-generations", str(G)])
    after = _md5s(str(tmp_path / "fit"))
    assert after["weights.map"] == before["weights.map"] and after == before
    # without the flag: the files of a default run, weights 1.0
    assert _md5s(str(tmp_path / "plain")) == _md5s(str(tmp_path / "plain2"))
    assert "weights_fit" not in plain and set(plain["weights"].values()) == {1.0} and plain2["weights"] == plain["weights"]
    ones_map = "".join("%s\t1.0\n" % k for k in sorted(plain["weights"]))
    assert open(str(tmp_path / "plain" / "weights.map")).read() == ones_map
    b, p = _md5s(str(tmp_path / "fit")), _md5s(str(tmp_path / "plain"))
    assert {f for f in b if b[f] != p[f]} == {"model.json", "weights.map"}
    # run_pipeline --model on a written library: _ags_of_sums with the fitted weights
    name, bases, off = mk.load_genome(6)
    g = _native.Genome(bases, off, 0)
    try:
        reads = g.simulate(100, 20000, 9, 1)
    finally:
        g.close()
    fa = str(tmp_path / "lib.fa")
    training.write_reads(fa, reads)
    args = {"seqfiles": [fa], "model_dir": str(tmp_path / "fit"), "read_length": 100, "nreads": 20000, "verbose": False, "device": 0}
    est, _ = mc.run_pipeline(dict(args))
    eng = mc._open_engine(0, str(tmp_path / "fit"))
    try:
        model = mc._model(str(tmp_path / "fit"))
        eng.set_run(100, model["pars"]["100"], fams)
        _, best = eng.search(reads)
    finally:
        eng.close()
    agg = mc.aggregate_hits({"model_dir": str(tmp_path / "fit"), "read_length": 100}, {}, mc._BestHits(best, fams))
    assert bits(est) == bits(mc._ags_of_sums(model, 100, agg, 20000 * 100))
    plain_model = dict(model, weights={k: 1.0 for k in model["weights"]})
    print("run_pipeline --model: %.1f with the fitted weights, %.1f with 1.0" % (est, mc._ags_of_sums(plain_model, 100, agg, 20000 * 100)))
