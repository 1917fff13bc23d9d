"""The bootstrap on the GPU: mc_bootstrap against the numpy statement of csrc/mc_boot.h (boot_restated.py) on the goldens' best hits
and on 2 M synthetic hits, its independence of the hits' order and of how they are split; run_pipeline with args['bootstrap'] and
args['curve']; the command line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import boot_restated as br
from microbecensus_amd import _native
from microbecensus_amd import microbe_census as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
INPUTS = os.path.join(GOLD, "inputs")
GOLDEN_CASES = ["config1_example_fq", "c2_100bp", "c5_300bp_q20_dups", "unittest_metagenome"]
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    return mc._engine(0)


def _stats(read_length):
    fams = mc._model()["families"]
    pars = mc.find_opt_pars(None, read_length)
    return fams, [pars[f]["aln_stat"] for f in fams]


def synthetic_hits(n=2_000_000, nfam=30, seed=1):
    """n best hits in ascending read id (about one read in three classified, ids up to the top of the int32 range at the end),
    families uniform over nfam, alignment and target lengths like the markers'."""
    rng = np.random.default_rng(seed)
    best = np.zeros(n, _native.BEST_DTYPE)
    reads = np.cumsum(rng.integers(1, 6, n))
    reads[-1000:] = 2**31 - 1000 + np.arange(1000)
    best["read"] = reads
    best["family"] = rng.integers(0, nfam, n)
    best["aln"] = rng.integers(12, 100, n)
    best["target_len"] = rng.integers(80, 900, n)
    best["bits"] = rng.uniform(30, 200, n)
    stats = [("hits", "cov", "aln")[f % 3] for f in range(nfam)]
    return best, stats


def check_sums(got, want, stats, what):
    """int64 sums equal; cov sums within n_f x 2^-53 relative of the statement's exact sum, n_f = the family's weighted hit count
    (at most n_f positive terms, each rounded once: (n_f - 1) x unit roundoff bounds any order of adding them)."""
    (gi, gf), (wi, wf) = got, want
    assert gi.shape == wi.shape and gf.shape == wf.shape, what
    assert np.array_equal(gi, wi), what
    cov = [f for f, s in enumerate(stats) if br.STAT.get(s, s) == 1]
    for f in range(len(stats)):
        if f not in cov:
            assert not gf[:, f].any(), what
    return cov


def cov_bound_ok(gf, wf, n_f):
    """|got - want| <= n_f x 2^-53 x want, per replicate and cov family; prints the worst ratio to the bound"""
    err = np.abs(gf - wf)
    bound = n_f * U53 * np.abs(wf)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))) if err.size else 0.0
    print("cov sums: worst error / bound = %.3g" % worst)
    return bool(np.all(err <= bound))


@pytest.mark.parametrize("B", [1, 64, 1000])
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_sums_on_golden_best_hits(eng, case, B):
    g = json.load(open(os.path.join(GOLD, case + ".json")))
    fams, stats = _stats(g["args"]["read_length"])
    best, _ = br.golden_best(case, fams)
    seed = 17
    got = eng.bootstrap(best, stats, B, seed)
    wi, wf, n_f = br.sums(best, stats, B, seed, return_counts=True)
    cov = check_sums(got, (wi, wf), stats, case)
    assert cov_bound_ok(got[1][:, cov], wf[:, cov], n_f[:, cov])
    assert np.array_equal(got[0][:, -1], n_f.sum(axis=1))


@pytest.fixture(scope="module")
def synth():
    return synthetic_hits()


@pytest.mark.parametrize("B", [1, 64, 1000])
def test_sums_on_two_million_synthetic_hits(eng, synth, B):
    """Families of all three aln_stats; every replicate is checked against the numpy statement."""
    best, stats = synth
    assert {"hits", "cov", "aln"} == set(stats)
    seed = 2**63 + 5
    got = eng.bootstrap(best, stats, B, seed)
    wi, wf, n_f = br.sums(best, stats, B, seed, threads=12, return_counts=True)
    cov = check_sums(got, (wi, wf), stats, "synthetic B=%d" % B)
    assert cov_bound_ok(got[1][:, cov], wf[:, cov], n_f[:, cov])


def test_order_and_split_do_not_matter(eng, synth):
    best, stats = synth
    best = best[:300_000]
    B, seed = 64, 99
    whole = eng.bootstrap(best, stats, B, seed)
    perm = np.random.default_rng(3).permutation(len(best))
    shuffled = eng.bootstrap(best[perm], stats, B, seed)
    cut = 123_457
    a, b = eng.bootstrap(best[:cut], stats, B, seed), eng.bootstrap(best[cut:], stats, B, seed)
    split = (a[0] + b[0], a[1] + b[1])
    wi, wf, n_f = br.sums(best, stats, B, seed, threads=12, return_counts=True)
    for name, got in (("whole", whole), ("shuffled", shuffled), ("split", split)):
        cov = check_sums(got, (wi, wf), stats, name)
        assert cov_bound_ok(got[1][:, cov], wf[:, cov], n_f[:, cov]), name
    # the same call again: the same bits (the tiles are added in a fixed order)
    again = eng.bootstrap(best, stats, B, seed)
    assert np.array_equal(again[0], whole[0]) and np.array_equal(again[1], whole[1])


def test_refusals(eng, synth):
    best, stats = synth
    few = best[:10].copy()
    with pytest.raises(RuntimeError, match="families"):
        eng.bootstrap(few, ["hits"] * 33, 4, 0)
    with pytest.raises(RuntimeError, match="replicates"):
        eng.bootstrap(few, stats, 0, 0)
    with pytest.raises(RuntimeError, match="replicates"):
        eng.bootstrap(few, stats, 65537, 0)
    bad = few.copy()
    bad["family"][3] = len(stats)
    with pytest.raises(RuntimeError, match="family"):
        eng.bootstrap(bad, stats, 4, 0)
    si, sf = eng.bootstrap(few[:0], stats, 4, 0)
    assert not si.any() and not sf.any()


def _example_args(**extra):
    a = {"seqfiles": [os.path.join(INPUTS, "example.fq.gz")], "nreads": 10000, "read_length": 100, "threads": 1}
    a.update(extra)
    return a


def test_run_pipeline_with_bootstrap(monkeypatch):
    g = json.load(open(os.path.join(GOLD, "config1_example_fq.json")))
    plain, _ = mc.run_pipeline(_example_args())
    est, out = mc.run_pipeline(_example_args(bootstrap=200, bootstrap_seed=7))
    assert est == plain == g["est_ags"]
    used, asked = out["ags_boot_replicates"]
    vals = out["ags_boot_values"]
    assert asked == 200 and len(vals) == 200 and used == sum(v is not None for v in vals) and used + sum(v is None for v in vals) == asked
    assert out["ags_boot_se"] > 0 and out["ags_ci95"][0] <= out["ags_ci95"][1]
    print("est %.1f  se %.1f  ci95 %.1f - %.1f  used %d / %d" % (est, out["ags_boot_se"], out["ags_ci95"][0], out["ags_ci95"][1], used, asked))
    # the host statement fed with the same best hits: the integer sums are the same numbers, the cov sums differ by rounding only
    # (n_f x 2^-53 relative, above), and a replicate's AGS is a weighted mean of coefficient x bases / sum - so it moves by at most
    # the largest relative error of a sum, plus the few roundings of the mean itself: (max n_f + 64) x 2^-53 relative.
    fams, stats = _stats(100)
    best, _ = br.golden_best("config1_example_fq", fams)
    si, sf = br.sums(best, stats, 200, 7)
    want = mc.bootstrap_replicates(dict(out), best, fams, si, sf, g["sampled_reads"], 7)
    tol = (float(si[:, -1].max()) + 64) * U53
    assert [v is None for v in vals] == [w is None for w in want]
    for v, w in zip(vals, want):
        if v is not None:
            assert abs(v - w) <= tol * abs(w)
    # the same seed: the same numbers on a second run, and with the sample dealt to three engines of this process
    est2, out2 = mc.run_pipeline(_example_args(bootstrap=200, bootstrap_seed=7))
    assert est2 == est and out2["ags_boot_values"] == vals and out2["ags_boot_se"] == out["ags_boot_se"] and out2["ags_ci95"] == out["ags_ci95"]
    monkeypatch.setenv("MC_STREAM_BATCH", "3000")
    a3 = _example_args(bootstrap=200, bootstrap_seed=7, devices=[0, 0, 0])
    a3["nreads"] = 10_000_000                                    # (else a run of this size would be given one device); the file has fewer reads than 10,000 to give
    est3, out3 = mc.run_pipeline(a3)
    monkeypatch.delenv("MC_STREAM_BATCH")
    assert sorted(k for k in mc._engines if isinstance(k, tuple)) == [(0, 1), (0, 2)]
    assert est3 == est and out3["sampled_reads"] == out["sampled_reads"]
    assert out3["ags_boot_values"] == vals and out3["ags_boot_se"] == out["ags_boot_se"] and out3["ags_ci95"] == out["ags_ci95"]
    # another seed: other replicates
    _, other = mc.run_pipeline(_example_args(bootstrap=200, bootstrap_seed=8))
    assert other["ags_boot_values"] != vals


def test_curve_equals_runs_at_smaller_n():
    """curve = 4 on c2_100bp's input: point k is run_pipeline at nreads = n_k on the same file, bit for bit."""
    f = os.path.join(INPUTS, "c2_100bp.fa.gz")
    g = json.load(open(os.path.join(GOLD, "c2_100bp.json")))
    est, out = mc.run_pipeline({"seqfiles": [f], "threads": 8, "curve": 4, "bootstrap": 64})
    assert est == g["est_ags"] and out["sampled_reads"] == g["sampled_reads"]
    n_ks = [math.ceil(k * g["sampled_reads"] / 4) for k in range(1, 5)]
    assert [p["reads"] for p in out["ags_curve"]] == n_ks
    for p in out["ags_curve"]:
        e, o = mc.run_pipeline({"seqfiles": [f], "threads": 8, "nreads": p["reads"]})
        print("n_k %d  curve %.4f  run %.4f  se %.1f" % (p["reads"], p["ags"], e, p["se"]))
        assert o["sampled_reads"] == p["reads"] and e == p["ags"]
        # the point's SE is the bootstrap of that smaller run
        _, ob = mc.run_pipeline({"seqfiles": [f], "threads": 8, "nreads": p["reads"], "bootstrap": 64})
        assert ob["ags_boot_se"] == p["se"]
    assert out["ags_curve"][-1]["ags"] == est and out["ags_curve"][-1]["se"] == out["ags_boot_se"]


def test_stage_by_stage_and_m8_routes(tmp_path):
    """keep_tmp (stage by stage) gives the same replicates as the fused route; best hits classified from the m8 file (the -r
    route's classification) give the same too."""
    _, fused = mc.run_pipeline(_example_args(bootstrap=50, bootstrap_seed=1, curve=2))
    _, staged = mc.run_pipeline(_example_args(bootstrap=50, bootstrap_seed=1, curve=2, keep_tmp=True))
    assert staged["ags_boot_values"] == fused["ags_boot_values"] and staged["ags_curve"] == fused["ags_curve"]
    args = _example_args(bootstrap=50, bootstrap_seed=1, curve=2)
    paths = mc.get_relative_paths(args)
    mc.check_paths(paths); mc.check_input(args); mc.impute_missing_args(args); mc.check_arguments(args)
    mc.process_seqfile(args, paths)
    mc.search_seqs(args, paths)
    mc._run_cache[paths["tempfile"]].pop("best")                 # as after an external search: classify_reads parses the m8 file
    best_hits = mc.classify_reads(args, paths)
    assert not isinstance(best_hits, mc._BestHits)
    arr, fams = mc._best_array(args, paths, best_hits)
    mc.clean_up(paths)
    mc._uncertainty(args, paths, arr, fams)
    assert args["ags_boot_values"] == fused["ags_boot_values"] and args["ags_curve"] == fused["ags_curve"]
    # the reference's -r hook (an external executable writes the m8 file; here the GPU engine behind RAPsearch2's command line)
    est, ext = mc.run_pipeline(_example_args(bootstrap=50, bootstrap_seed=1, curve=2, rapsearch=os.path.join(REPO, "scripts", "rapsearch_mi355x")))
    assert est == json.load(open(os.path.join(GOLD, "config1_example_fq.json")))["est_ags"]
    assert ext["ags_boot_values"] == fused["ags_boot_values"] and ext["ags_curve"] == fused["ags_curve"]


def test_cli_writes_the_new_lines(tmp_path):
    script = os.path.join(REPO, "scripts", "run_microbe_census.py")
    common = ["-n", "10000", "-l", "100", "-t", "1", os.path.join(INPUTS, "example.fq.gz")]
    plain, boot = tmp_path / "plain.txt", tmp_path / "boot.txt"
    subprocess.check_call([sys.executable, script] + common + [str(plain)])
    subprocess.check_call([sys.executable, script, "--bootstrap", "100", "--bootstrap-seed", "5", "--curve", "3"] + common + [str(boot)])
    g = json.load(open(os.path.join(GOLD, "config1_example_fq.json")))
    want = ("Parameters\nmetagenome:\t%s\nreads_sampled:\t%d\ntrimmed_length:\t100\nmin_quality:\t-5\nmean_quality:\t-5\nfilter_dups:\tFalse\nmax_unknown:\t100\n\n"
            "Results\naverage_genome_size:\t%s\ntotal_bases:\t980306\ngenome_equivalents:\t%s\n" % (common[-1], g["sampled_reads"], g["est_ags"], 980306 / g["est_ags"]))
    assert plain.read_text() == want
    text = boot.read_text()
    assert text.startswith(want)
    extra = [l.split("\t") for l in text[len(want):].splitlines()]
    assert [l[0] for l in extra] == ["ags_boot_se:", "ags_ci95_low:", "ags_ci95_high:", "ags_boot_replicates:", "curve_reads:", "curve_ags:", "curve_se:"]
    assert float(extra[0][1]) > 0 and float(extra[1][1]) <= float(extra[2][1]) and extra[3][1].endswith("/100")
    assert [int(x) for x in extra[4][1:]] == [math.ceil(k * g["sampled_reads"] / 3) for k in (1, 2, 3)] and float(extra[5][-1]) == g["est_ags"]
