#!/usr/bin/env python3
"""Measurements behind the bootstrap, one GPU.

    python tools/bootstrap_timing.py kernel [--hits 10000,100000,1000000] [-B 1000] [--reps 15] [--numpy-replicates 20]
        mc_bootstrap's kernels by HIP events (warmed, median of --reps calls; also the whole call's wall time, upload and download
        included) beside the numpy statement of csrc/mc_boot.h (tests/boot_restated.py) on this host, single-threaded: timed for
        --numpy-replicates replicates and scaled to B (a replicate costs the same whichever it is).
    python tools/bootstrap_timing.py run [--reads 2000000] [-B 1000] [--reps 10] [--tree DIR]
        run_pipeline on a FASTQ of the bench workload, plain and with args['bootstrap'] = B, alternating in one process.  --tree: the
        checkout whose microbecensus_amd is imported (a parent commit's, for its plain run; the bootstrap legs are skipped there).
    python tools/bootstrap_timing.py se [--samples 50] [--reads 2000000] [-B 1000]
        --samples independent samples of one community (synth.GenomeReads, disjoint read indices): the standard deviation of their
        AGS values beside the median of their bootstrap standard errors.

Each mode prints JSON lines."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_hits(n, nfam, seed=1):
    from microbecensus_amd import _native
    rng = np.random.default_rng(seed)
    best = np.zeros(n, _native.BEST_DTYPE)
    best["read"] = np.cumsum(rng.integers(1, 20, n))
    best["family"] = rng.integers(0, nfam, n)
    best["aln"] = rng.integers(12, 50, n)
    best["target_len"] = rng.integers(80, 900, n)
    return best


def mode_kernel(a):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import boot_restated as br
    from microbecensus_amd import microbe_census as mc
    fams = mc._model()["families"]
    pars = mc.find_opt_pars(None, 150)
    stats = [pars[f]["aln_stat"] for f in fams]
    eng = mc._engine(a.device)
    for n in [int(x) for x in a.hits.split(",")]:
        best = synthetic_hits(n, len(fams))
        for _ in range(3):
            eng.bootstrap(best, stats, a.B, 1)
        ms, wall = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            eng.bootstrap(best, stats, a.B, 1)
            wall.append((time.perf_counter() - t) * 1e3)
            ms.append(eng.bootstrap_ms())
        r = min(a.numpy_replicates, a.B)
        br.sums(best, stats, a.B, 1, replicates=range(1))
        t = time.perf_counter()
        br.sums(best, stats, a.B, 1, replicates=range(r))
        numpy_ms = (time.perf_counter() - t) * 1e3 * a.B / r
        print(json.dumps({"mode": "kernel", "hits": n, "B": a.B, "kernel_ms_median": round(statistics.median(ms), 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                          "call_wall_ms_median": round(statistics.median(wall), 3), "reps": a.reps, "numpy_ms_scaled_to_B": round(numpy_ms, 1), "numpy_replicates_timed": r,
                          "ratio_numpy_over_kernel": round(numpy_ms / statistics.median(ms), 1), "ratio_numpy_over_call": round(numpy_ms / statistics.median(wall), 1)}), flush=True)


def mode_run(a):
    tree = os.path.abspath(a.tree) if a.tree else REPO
    sys.path.insert(0, tree)
    from microbecensus_amd import microbe_census as mc
    from microbecensus_amd import synth
    sys.path.insert(1, REPO)
    import bench
    import torch
    gen = synth.GenomeReads(device=torch.device("cuda", a.device), seed=20261001, path=os.path.join(REPO, "tests", "golden", "genomes", "genomes30.npz"))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "reads.fq")
        bench.write_fastq(gen, a.reads, 150, path, False)
        legs = {"plain": {}} if a.tree else {"plain": {}, "bootstrap": {"bootstrap": a.B}}
        walls = {k: [] for k in legs}
        est = {}
        for rep in range(a.reps + 1):                              # (the first round allocates the pools: not counted)
            for leg, extra in legs.items():
                args = dict({"seqfiles": [path], "device": a.device, "nreads": a.reads, "read_length": 150}, **extra)
                t = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    res = mc.run_pipeline(args)
                if rep:
                    walls[leg].append(time.perf_counter() - t)
                est[leg] = res[0]
        out = {"mode": "run", "tree": tree, "reads": a.reads, "B": a.B, "reps": a.reps, "est_ags": est}
        for leg, w in walls.items():
            out[leg] = {"wall_s_median": round(statistics.median(w), 4), "wall_s_min": round(min(w), 4), "wall_s_max": round(max(w), 4), "wall_s": [round(x, 4) for x in w]}
        print(json.dumps(out), flush=True)


def mode_se(a):
    from microbecensus_amd import microbe_census as mc
    from microbecensus_amd import synth
    import torch
    L = 150
    model = mc._model()
    fams = model["families"]
    eng = mc._engine(a.device)
    eng.set_run(L, model["pars"][str(L)], fams)
    gen = synth.GenomeReads(device=torch.device("cuda", a.device), seed=20261001)
    ags, se, used, nbest = [], [], [], []
    for s in range(a.samples):
        reads = gen.single(a.reads, L, first=(1 << 41) + s * a.reads).cpu().numpy()
        _, best = eng.search(reads)
        args = {"verbose": False, "read_length": L, "sampled_reads": a.reads, "bootstrap": a.B, "bootstrap_seed": s, "device": a.device}
        agg = mc.aggregate_hits(args, {}, mc._BestHits(best, fams))
        ags.append(mc._ags_of_sums(model, L, agg, a.reads * L))
        r = mc.bootstrap_ags(args, best, fams)
        se.append(r["se"]); used.append(r["used"]); nbest.append(len(best))
        print(json.dumps({"mode": "se", "sample": s, "ags": ags[-1], "boot_se": se[-1], "used": used[-1], "best_hits": nbest[-1]}), flush=True)
    print(json.dumps({"mode": "se", "samples": a.samples, "reads": a.reads, "B": a.B, "mean_ags": float(np.mean(ags)), "sd_of_ags_over_samples": float(np.std(ags, ddof=1)),
                      "median_boot_se": float(np.median(se)), "min_boot_se": float(np.min(se)), "max_boot_se": float(np.max(se)), "min_used": int(min(used)),
                      "mean_best_hits": float(np.mean(nbest))}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernel", "run", "se"])
    p.add_argument("--hits", default="10000,100000,1000000")
    p.add_argument("-B", type=int, default=1000)
    p.add_argument("--reps", type=int, default=None)
    p.add_argument("--numpy-replicates", type=int, default=20)
    p.add_argument("--reads", type=int, default=2000000)
    p.add_argument("--samples", type=int, default=50)
    p.add_argument("--tree", default=None)
    p.add_argument("--device", type=int, default=0)
    a = p.parse_args()
    if a.reps is None:
        a.reps = 15 if a.mode == "kernel" else 10
    if a.mode != "run":
        sys.path.insert(0, REPO)
    {"kernel": mode_kernel, "run": mode_run, "se": mode_se}[a.mode](a)


if __name__ == "__main__":
    main()
