"""The bootstrap and the -n curve on the CPU: the weights of csrc/mc_boot.h (g++ build, tests/emul/boot_weights.cpp) against their
numpy restatement (boot_restated.py), the threshold table against exact arithmetic, the statistics a sum of Poisson(1) weights must
have, the refactored estimate against every golden, the report with the switches off, and the curve's definition."""
import glob
import json
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import boot_restated as br
from microbecensus_amd import _native
from microbecensus_amd import microbe_census as mc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("boot") / "boot_weights")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "emul", "boot_weights.cpp")])
    return exe


def test_header_table_is_what_the_compiler_sees(driver):
    vals = [int(x) for x in subprocess.check_output([driver, "table"]).split()]
    assert vals[0] == br.BOOT_K and vals[1] == br.BOOT_KEY and vals[2:] == br.THRESHOLDS


def test_weights_match_the_numpy_statement(driver, tmp_path):
    """3.2 M (seed, b, r) triples: random ones, r around 2^31 (the largest read ids), r = 0, b = 0 and b = B - 1."""
    rng = np.random.default_rng(5)
    n = 800_000
    B = 1000
    blocks = []
    for seed in (0, 1, 0xDEADBEEFCAFEF00D, 2**64 - 1):
        r = rng.integers(0, 2**31, n, dtype=np.uint64)
        r[:50_000] = np.uint64(2**31 - 1) - np.arange(50_000, dtype=np.uint64)          # the top of the int32 range
        r[50_000:60_000] = np.arange(10_000, dtype=np.uint64)
        b = rng.integers(0, B, n, dtype=np.uint64)
        b[:200_000:2] = 0
        b[1:200_000:2] = B - 1
        blocks.append(np.stack([np.full(n, seed, np.uint64), b, r], axis=1))
    trip = np.concatenate(blocks)
    (tmp_path / "in.bin").write_bytes(trip.tobytes())
    subprocess.check_call([driver, "weights", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    want = np.concatenate([br.weights(int(blk[0, 0]), blk[:, 1], blk[:, 2]) for blk in blocks])
    assert len(got) == len(trip) == 4 * n and np.array_equal(got, want)
    assert 0.99 < want.mean() < 1.01 and want.max() <= br.BOOT_K


def test_threshold_table_against_exact_arithmetic():
    """threshold k = floor(2^64 x P[X <= k]), X ~ Poisson(1), from a rational e good to far more than 64 bits; the mass folded into
    the last weight, P[X > K], is below 2^-60."""
    e = sum(Fraction(1, math.factorial(k)) for k in range(60))          # the series' remainder is < 2 / 60! ~ 2^-271
    cdf = Fraction(0)
    for k, t in enumerate(br.THRESHOLDS):
        cdf += Fraction(1, math.factorial(k)) / e
        assert abs(Fraction(t) - cdf * 2**64) <= 1, k
        assert t == (cdf * 2**64).__floor__(), k
    below_k = cdf                                                        # P[X <= K - 1]: weight K takes everything above it
    tail = 1 - below_k - Fraction(1, math.factorial(br.BOOT_K)) / e      # P[X > K], the part that is folded
    assert 0 < tail < Fraction(1, 2**60)
    assert all(a < b for a, b in zip(br.THRESHOLDS, br.THRESHOLDS[1:]))


def test_sum_of_weights_has_mean_and_variance_n():
    """n hits of one 'hits' family, B = 4096: S[b] is a sum of n Poisson(1) draws - mean n, variance n.  Margins: 5 standard errors of
    the two estimators (sqrt(n / B) for the mean; sqrt(2 / B) relative for the variance).  Seed 11 (fixed; it passes on the CPU)."""
    n, B = 5000, 4096
    best = np.zeros(n, _native.BEST_DTYPE)
    best["read"] = np.arange(n) * 7 + 3
    best["aln"], best["target_len"] = 30, 100
    si, sf = br.sums(best, ["hits"], B, 11)
    S = si[:, 0].astype(np.float64)
    assert np.array_equal(si[:, 0], si[:, 1]) and not sf.any()
    assert abs(S.mean() - n) <= 5 * math.sqrt(n / B)
    assert abs(S.var(ddof=1) / n - 1) <= 5 * math.sqrt(2 / B)


def _goldens_with_ags():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLD, "*.json"))):
        try:
            g = json.load(open(p))
        except ValueError:
            continue
        if isinstance(g, dict) and "est_ags" in g and "agg_hits" in g:
            out.append(os.path.basename(p)[:-5])
    return out


def test_there_are_goldens_with_an_ags():
    assert len(_goldens_with_ags()) >= 4


@pytest.mark.parametrize("case", _goldens_with_ags())
def test_estimate_through_the_helper_is_bit_identical(case):
    g = json.load(open(os.path.join(GOLD, case + ".json")))
    args = {"verbose": False, "read_length": g["args"]["read_length"], "sampled_reads": g["sampled_reads"]}
    # (the estimate's weighted sum runs over the families in the order of their first hit: the golden JSON is key-sorted, so the
    # sums are made again from its best hits in m8 order = ascending read id, as tests/test_host_logic.py does)
    best = dict(sorted(g["best_hits"].items(), key=lambda kv: int(kv[0])))
    agg = mc.aggregate_hits(args, {}, best)
    assert agg == g["agg_hits"]
    assert mc.estimate_average_genome_size(args, {}, agg) == g["est_ags"]
    assert mc._ags_of_sums(mc._model(), g["args"]["read_length"], agg, g["sampled_reads"] * g["args"]["read_length"]) == g["est_ags"]


def _report(tmp_path, name, **extra):
    args = {"outfile": str(tmp_path / name), "seqfiles": ["a", "b"], "sampled_reads": 5, "read_length": 100, "min_quality": -5, "mean_quality": -5,
            "filter_dups": False, "max_unknown": 100}
    args.update(extra)
    mc.report_results(args, 3051745.7641809303, 980306)
    return open(args["outfile"]).read()


PLAIN = ("Parameters\nmetagenome:\ta,b\nreads_sampled:\t5\ntrimmed_length:\t100\nmin_quality:\t-5\nmean_quality:\t-5\n"
         "filter_dups:\tFalse\nmax_unknown:\t100\n\nResults\naverage_genome_size:\t3051745.7641809303\ntotal_bases:\t980306\n"
         "genome_equivalents:\t0.32122793828571367\n")


def test_report_is_unchanged_with_the_switches_off(tmp_path):
    assert _report(tmp_path, "a.txt") == PLAIN
    assert _report(tmp_path, "b.txt", bootstrap=0, bootstrap_seed=0, curve=0) == PLAIN
    # figures of an earlier run left in args do not leak into a report whose switches are off
    assert _report(tmp_path, "c.txt", bootstrap=0, curve=0, ags_boot_se=1.0, ags_ci95=(1.0, 2.0), ags_boot_replicates=(3, 3), ags_curve=[]) == PLAIN


def test_report_appends_the_new_lines(tmp_path):
    text = _report(tmp_path, "d.txt", bootstrap=200, curve=2, ags_boot_se=1234.5, ags_ci95=(3000000.0, 3100000.0), ags_boot_replicates=(199, 200),
                   ags_curve=[{"reads": 3, "ags": 3.5e6, "se": 9.0}, {"reads": 5, "ags": None, "se": float("nan")}])
    assert text == PLAIN + ("ags_boot_se:\t1234.5\nags_ci95_low:\t3000000.0\nags_ci95_high:\t3100000.0\nags_boot_replicates:\t199/200\n"
                            "curve_reads:\t3\t5\ncurve_ags:\t3500000.0\tNone\ncurve_se:\t9.0\tnan\n")


@pytest.mark.parametrize("case", ["config1_example_fq", "c2_100bp", "c5_300bp_q20_dups", "unittest_metagenome"])
def test_curve_point_is_the_helper_on_the_prefix(case):
    fams = mc._model()["families"]
    best, g = br.golden_best(case, fams)
    K = 4
    args = {"verbose": False, "read_length": g["args"]["read_length"], "sampled_reads": g["sampled_reads"], "curve": K}
    curve = mc.ags_curve(args, {}, best, fams)
    n_ks = [math.ceil(k * g["sampled_reads"] / K) for k in range(1, K + 1)]
    assert [p["reads"] for p in curve] == n_ks and n_ks[-1] == g["sampled_reads"]
    model = mc._model()
    for p, n_k in zip(curve, n_ks):
        head = best[best["read"] < n_k]
        if len(head) == 0:
            assert p["ags"] is None
            continue
        agg = mc.aggregate_hits(args, {}, mc._BestHits(head, fams))
        assert p["ags"] == mc._ags_of_sums(model, args["read_length"], agg, n_k * args["read_length"])
    # the whole sample is the run's own estimate
    assert curve[-1]["ags"] == g["est_ags"]


def test_replicates_from_host_sums_and_their_summary():
    """bootstrap_replicates on the host statement's sums of a golden: every replicate has a value near the estimate, the summary's
    SE is their sample standard deviation, and the draws for the unclassified reads are the documented generator's."""
    fams = mc._model()["families"]
    best, g = br.golden_best("unittest_metagenome", fams)
    L = g["args"]["read_length"]
    args = {"verbose": False, "read_length": L, "sampled_reads": g["sampled_reads"]}
    stats = [mc.find_opt_pars(None, L)[f]["aln_stat"] for f in fams]
    B, seed = 64, 3
    si, sf = br.sums(best, stats, B, seed)
    vals = mc.bootstrap_replicates(args, best, fams, si, sf, g["sampled_reads"], seed)
    assert len(vals) == B and all(v is not None for v in vals)
    s = mc._boot_summary(vals, B)
    assert s["used"] == B and s["asked"] == B and s["se"] == float(np.std(np.array(vals), ddof=1)) and s["ci95"][0] < s["ci95"][1]
    assert 0.5 * g["est_ags"] < min(vals) and max(vals) < 2 * g["est_ags"]
    n0 = mc.bootstrap_unclassified(seed, B, g["sampled_reads"] - len(best))
    want = np.random.Generator(np.random.PCG64(np.random.SeedSequence([mc.BOOT_N0_DOMAIN, seed]))).poisson(float(g["sampled_reads"] - len(best)), size=B)
    assert np.array_equal(n0, want)
    # a replicate without any hit has no value and is counted as left out
    empty = mc.bootstrap_replicates(args, best, fams, np.zeros_like(si), np.zeros_like(sf), g["sampled_reads"], seed)
    assert empty == [None] * B and mc._boot_summary(empty, B)["used"] == 0


def test_bootstrap_without_a_gpu_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    fams = mc._model()["families"]
    best, g = br.golden_best("config1_example_fq", fams)
    args = {"verbose": False, "read_length": 100, "sampled_reads": g["sampled_reads"], "bootstrap": 10, "device": 0}
    with pytest.raises(Exception, match="no CPU fallback"):
        mc.bootstrap_ags(args, best, fams)


def test_distributed_run_refuses_the_switches():
    src = open(os.path.join(os.path.dirname(HERE), "microbecensus_amd", "distributed.py")).read()
    assert "--bootstrap and --curve are not available in a distributed run" in src
