"""The weight fit (training step 5) on the CPU: csrc/mc_wfit.h built with g++ (tests/emul/wfit.cpp, -ffp-contract=off) against its
numpy restatement (wfit_restated.py) bit for bit - perturbations, mask, errors, mue, whole fits -, the objective against
_ags_of_sums, the planted problem on the restatement, and the host side of training.fit_weights and the two commands."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wfit_restated as wr
from microbecensus_amd import _native, training
from microbecensus_amd import microbe_census as mc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SHAPES = [(N, F) for N in (1, 2, 29, 30, 150) for F in (1, 30, 32)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def table(rng, N, F, na=0.05, na_columns=(), dead=()):
    """a random table: predictions within 10 % of the truth, some NA, whole NA columns, families so far off that no library keeps them"""
    truth = np.floor(rng.uniform(1e6, 9e6, N))
    pred = truth[:, None] * (1.0 + 0.1 * rng.standard_normal((N, F)))
    pred[rng.random((N, F)) < na] = np.nan
    for f in na_columns:
        pred[:, f] = np.nan
    for f in dead:
        pred[:, f] = truth * 50.0
    return pred, truth


def weight_vectors(rng, K, F):
    """random vectors, vectors with zeros, the all-zero vector (every library without an estimate) and single-family vectors"""
    W = rng.random((K, F))
    W[rng.random((K, F)) < 0.3] = 0.0
    W[0] = 0.0
    for k in range(1, min(K, 1 + F)):
        W[k] = 0.0
        W[k, k - 1] = 1.0
    W[-1] = 1.0
    return W


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wfit") / "wfit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "emul", "wfit.cpp")])
    return exe


def run_driver(driver, tmp_path, mode, head, *arrays):
    blob = np.array(head, dtype=np.int64).tobytes() if head is not None else b""
    (tmp_path / "in.bin").write_bytes(blob + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
    subprocess.check_call([driver, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64)


def driver_fit(driver, tmp_path, pred, truth, seed, L, C, G):
    N, F = pred.shape
    out = run_driver(driver, tmp_path, "fit", [N, F, C, G, seed, L], pred, truth)
    return out[:F], out[F:].reshape(G + 1, 3)


def test_header_constants_are_what_the_compiler_sees(driver):
    vals = subprocess.check_output([driver, "consts"]).split()
    assert [int(v) for v in vals[:4]] == [wr.WFIT_KEY, wr.DEFAULT_C, wr.DEFAULT_G, wr.MAX_N]
    assert [float(v) for v in vals[4:]] == [wr.SIGMA0, wr.SIGMA_MIN, wr.MAD_CONST]
    assert wr.MAX_N >= 4096 and wr.SIGMA_MIN == 2.0 ** -20 and wr.MAD_CONST == 1.48
    assert (_native.WFIT_DEFAULT_C, _native.WFIT_DEFAULT_G) == (wr.DEFAULT_C, wr.DEFAULT_G)


def test_perturbations_match_the_numpy_statement(driver, tmp_path):
    rng = np.random.default_rng(11)
    n = 400_000
    q = np.stack([rng.choice(np.array([0, 1, 0xDEADBEEFCAFEF00D, 2**64 - 1], dtype=np.uint64), n), rng.choice(np.array([50, 100, 150, 500], dtype=np.uint64), n),
                  rng.integers(0, 4096, n, dtype=np.uint64), rng.integers(0, 65536, n, dtype=np.uint64), rng.integers(0, 32, n, dtype=np.uint64)], axis=1)
    got = run_driver(driver, tmp_path, "d", None, q)
    want = np.concatenate([wr.d(int(s), q[q[:, 0] == s][:, 1], q[q[:, 0] == s][:, 2], q[q[:, 0] == s][:, 3], q[q[:, 0] == s][:, 4]) for s in np.unique(q[:, 0])])
    order = np.concatenate([np.nonzero(q[:, 0] == s)[0] for s in np.unique(q[:, 0])])
    assert np.array_equal(bits(got[order]), bits(want))
    assert got.min() >= -1.0 and got.max() < 1.0
    moved = got != 0.0
    assert 0.25 < moved.mean() < 0.40                              # 1/4 dense + 1/4 x 1/4 + 1/2 x 1/32
    assert abs(got[moved].mean()) < 0.01


@pytest.mark.parametrize("N,F", SHAPES)
def test_mask_errors_and_mue_match(driver, tmp_path, N, F):
    rng = np.random.default_rng(1000 * N + F)
    pred, truth = table(rng, N, F, na_columns=(2,) if F > 2 else (), dead=(5, 7) if F > 7 else ())
    K = 64
    W = weight_vectors(rng, K, F)
    out = run_driver(driver, tmp_path, "eval", [N, F, K, 0, 0, 0], pred, truth, W)
    pm, keep, alive = wr.mask(pred)
    o = 0
    assert np.array_equal(bits(out[o:o + N * F]), bits(pm.reshape(-1))); o += N * F
    keep_bits = (keep.astype(np.uint64) << np.arange(F, dtype=np.uint64)[None, :]).sum(axis=1)
    assert np.array_equal(out[o:o + N].astype(np.uint64), keep_bits); o += N
    assert int(out[o]) == int((alive.astype(np.uint64) << np.arange(F, dtype=np.uint64)).sum()); o += 1
    errs = wr.errors(pm, keep, truth, W)
    assert np.array_equal(bits(out[o:o + K * N]), bits(errs.reshape(-1))); o += K * N
    mue = wr.mue(pm, keep, truth, W)
    assert np.array_equal(bits(out[o:o + K]), bits(mue))
    assert np.isinf(errs[0]).all() and np.isinf(mue[0])            # the all-zero vector: no library has an estimate
    if F > 7:
        assert not alive[2] and not alive[5] and not alive[7] and (N < 29 or alive.sum() >= F - 4)
        assert np.isinf(mue[1 + 5])                                # all weight on a family kept nowhere
    if F == 1:
        assert not keep.any()                                      # one prediction: the spread is 0, nothing is strictly inside it


@pytest.mark.parametrize("N,F", SHAPES)
def test_small_fits_match(driver, tmp_path, N, F):
    rng = np.random.default_rng(77 * N + F)
    pred, truth = table(rng, N, F, na_columns=(1,) if F > 2 else (), dead=(3,) if F > 7 else ())
    for seed, L in ((0, 100), (0xFEEDFACE12345678, 150)):
        C, G = 64, 24
        w, trace = wr.fit(pred, truth, seed, L, C, G)
        gw, gtrace = driver_fit(driver, tmp_path, pred, truth, np.array(seed, dtype=np.uint64).astype(np.int64), L, C, G)
        assert np.array_equal(bits(gw), bits(w)) and np.array_equal(bits(gtrace.reshape(-1)), bits(trace.reshape(-1)))
        assert (trace[1:, 0] <= trace[:-1, 0]).all() and w.min() >= 0.0 and w.max() <= 1.0
        if F > 7:
            assert w[1] == 1.0 / F and w[3] == 1.0 / F             # never kept: never moved
    if N >= 29 and F >= 30:
        assert trace[-1, 0] < trace[0, 0]


def test_a_fit_that_runs_out_of_sigma_ends_early(driver, tmp_path):
    """F = 1 keeps nothing: every mue is +inf, no candidate is better, sigma halves each generation and the search ends"""
    rng = np.random.default_rng(3)
    pred, truth = table(rng, 5, 1, na=0.0)
    w, trace = wr.fit(pred, truth, 1, 100, 8, 40)
    gw, gtrace = driver_fit(driver, tmp_path, pred, truth, 1, 100, 8, 40)
    assert np.array_equal(bits(gw), bits(w)) and np.array_equal(bits(gtrace.reshape(-1)), bits(trace.reshape(-1)))
    assert np.isinf(trace[:, 0]).all() and trace[-1, 1] == -1.0 and trace[-1, 2] < wr.SIGMA_MIN
    ended = int(np.argmax(trace[:, 1] == -1.0))
    assert ended == int(np.log2(wr.SIGMA0 / wr.SIGMA_MIN)) + 2 and (trace[1:ended, 1] == 0.0).all()
    # G = 0: the start
    w0, t0 = wr.fit(pred, truth, 1, 100, 8, 0)
    assert t0.shape == (1, 3) and w0[0] == 1.0


def test_the_objective_is_the_estimators():
    """_ags_of_sums with given weights = the restatement's weighted prediction of pred = coefficient / (hits / bases); the families
    it drops are the mask's."""
    rng = np.random.default_rng(2026)
    L = 100
    for trial in range(200):
        F = int(rng.integers(2, 33))
        fams = ["f%02d" % i for i in range(F)]
        hits = rng.integers(0, 400, F).astype(np.float64)
        hits[rng.random(F) < 0.1] = 0.0
        bases = float(rng.integers(10**6, 10**8))
        coeff = rng.uniform(1e-3, 1.0, F) * rng.choice([1.0, 1.0, 1.0, 3.0], F)
        w = rng.random(F)
        w[rng.random(F) < 0.2] = 0.0
        model = {"coefficients": {"%d_%s" % (L, f): float(c) for f, c in zip(fams, coeff)}, "weights": {"%d_%s" % (L, f): float(x) for f, x in zip(fams, w)}}
        agg = {f: float(h) for f, h in zip(fams, hits)}                       # ascending family order
        pred = np.array([[c / (h / bases) if h / bases != 0 else np.nan for c, h in zip(coeff.tolist(), hits.tolist())]])
        pm, keep, _ = wr.mask(pred)
        ests = {f: p for f, p in zip(fams, pred[0].tolist()) if p == p}
        if ests:
            spread, centre = mc.mad(list(ests.values())), mc.median(list(ests.values()))
            assert [abs(p - centre) < spread for p in ests.values()] == keep[0][~np.isnan(pred[0])].tolist()
        truth = np.array([3.0e6])
        e = wr.errors(pm, keep, truth, w)[0, 0]
        try:
            ags = mc._ags_of_sums(model, L, agg, bases)
        except ZeroDivisionError:
            assert np.isinf(e)
            continue
        assert e == abs(truth[0] - ags) / truth[0]
        num = den = 0.0
        for f in range(F):
            num = num + w[f] * pm[0, f]
            den = den + (w[f] if keep[0, f] else 0.0)
        assert bits(num / den) == bits(ags)


PLANTED_C, PLANTED_G = 512, 48          # the header's defaults scaled down to what a CPU test can afford


def planted_conditions(w, trace):
    """the three conditions of the planted problem on a fit's result"""
    assert trace[-1, 0] < trace[0, 0]
    assert w[wr.PLANTED_GOOD:].mean() < w[:wr.PLANTED_GOOD].mean()
    pred2, truth2 = wr.planted(2)
    pm2, keep2, _ = wr.mask(pred2)
    F = len(w)
    fresh = wr.mue(pm2, keep2, truth2, np.stack([np.full(F, 1.0 / F), w]))
    assert fresh[1] < fresh[0], fresh
    return fresh


def test_planted_problem_on_the_restatement():
    pred, truth = wr.planted(1)
    assert pred.shape == (150, 30)
    _, keep, alive = wr.mask(pred)
    assert alive.all() and 0.2 < keep[:, wr.PLANTED_GOOD:].mean() < 0.8      # the bad families are cut sometimes, not always
    w, trace = wr.fit(pred, truth, 0, 100, PLANTED_C, PLANTED_G)
    planted_conditions(w, trace)


def test_write_model_round_trips_fitted_weights(tmp_path):
    fams = ["fa", "fb"]
    weights = {"100_fa": 0.1 + 0.2, "100_fb": 1.0 / 3.0}
    rec = training.weights_fit_record(5, None, None, {100: (0.5, 0.25)})
    model = training.write_model(str(tmp_path), ["m0", "m1"], ["MKT", "MKV"], [0, 1], fams, [100], {"100": {"fa": [0.0, 100.0, 23.0, "hits"], "fb": [0.0, 100.0, 23.0, "hits"]}},
                                 {"100_fa": 1.0, "100_fb": 2.0}, weights, weights_fit=rec)
    assert model["weights_fit"] == {"seed": 5, "candidates": wr.DEFAULT_C, "generations": wr.DEFAULT_G, "mue": {"100": [0.5, 0.25]}}
    back = {k: float(v) for k, v in training.read_map(str(tmp_path / "weights.map"))}
    assert back == weights and json.load(open(str(tmp_path / "model.json")))["weights"] == weights
    # without the record the model has no such key
    plain = training.write_model(str(tmp_path / "p"), ["m0", "m1"], ["MKT", "MKV"], [0, 1], fams, [100], {"100": {}}, {}, {"100_fa": 1.0})
    assert "weights_fit" not in plain and open(str(tmp_path / "p" / "weights.map")).read() == "100_fa\t1.0\n"


def test_weight_tables_from_map_rows():
    rows = [["100", "fa", "g1", "3000000", repr(2.5e6 / 3.0)], ["100", "fb", "g1", "3000000", "NA"], ["100", "fa", "g0", "10", "7.5"], ["150", "fa", "g1", "3000000", "1.0"]]
    t = training.weight_tables(rows, ["fa", "fb"], [100, 150])
    pred, truth, genomes = t[100]
    assert genomes == ["g1", "g0"] and truth.tolist() == [3000000.0, 10.0]
    assert pred[0, 0] == 2.5e6 / 3.0 and np.isnan(pred[0, 1]) and pred[1, 0] == 7.5 and np.isnan(pred[1, 1])
    assert t[150][0].shape == (1, 2)
    typed = training.weight_tables([(100, "fa", "g1", 3000000, 2.5e6 / 3.0), (100, "fb", "g1", 3000000, None), (100, "fa", "g0", 10, 7.5)], ["fa", "fb"], [100])
    assert np.array_equal(bits(typed[100][0]), bits(pred))


def test_fitting_without_a_gpu_is_an_error_not_a_fallback(tmp_path):
    import gzip
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        training.fit_weights([], ["fa"], [100], None)
    gd = tmp_path / "genomes"
    gd.mkdir()
    for i in range(2):
        with gzip.open(str(gd / ("g%d.fna.gz" % i)), "wt") as f:
            f.write(">c\n%s\n" % ("ACGT" * 200))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        training.train(str(gd), str(tmp_path / "out"), [100], 1, xfolds=2, fit_weights=True, log=lambda *a: None)
    # the command on a model directory
    names, seqs = _native.load_markers()
    model = _native.load_model()
    md = tmp_path / "model"
    training.write_model(str(md), names[:4], seqs[:4], [0, 0, 1, 1], model["families"][:2], [100], {"100": {}}, {}, {}, {"g0": 10}, [(100, model["families"][0], "g0", 5.0)])
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "optimize_weights.py"), str(md)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr and "Traceback" not in r.stderr
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "optimize_weights.py"), str(tmp_path / "nothing")], capture_output=True, text=True)
    assert r.returncode != 0 and "Traceback" not in r.stderr


def test_fit_weights_flags_parse():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import optimize_weights
    import train_microbe_census as t
    a = t.parse_arguments(["g", "o", "-l", "100", "-c", "2"])
    assert a.fit_weights is False and a.fit_seed == 0 and a.fit_candidates is None and a.fit_generations is None
    a = t.parse_arguments(["g", "o", "-l", "100", "-c", "2", "--fit-weights", "--fit-seed", "7", "--fit-candidates", "256", "--fit-generations", "12"])
    assert (a.fit_weights, a.fit_seed, a.fit_candidates, a.fit_generations) == (True, 7, 256, 12)
    with pytest.raises(SystemExit):
        t.parse_arguments(["g", "o", "-l", "100", "-c", "2", "--fit-seed", "7"])
    b = optimize_weights.parse_arguments(["m", "-g", "1", "--fit-seed", "3"])
    assert (b.model_dir, b.device, b.fit_seed, b.fit_candidates, b.fit_generations) == ("m", 1, 3, None, None)
