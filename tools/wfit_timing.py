#!/usr/bin/env python3
"""Times the weight fit (mc_fit_weights) at the header's default candidates and generations on the planted problem of
tests/wfit_restated.py, N = 30, 150 and the limit with F = 30: the kernels' time (mc_fit_weights_ms: median, min and max of --runs
runs) and the whole call, beside the numpy restatement on one host thread - timed over --host-generations generations and scaled to
the generations the device ran (the restatement's cost per generation does not depend on the generation).  One JSON line per size.

    tools/wfit_timing.py [-g device] [--runs 5] [--host-generations 2]
    tools/wfit_timing.py --experiment [--coverage 5] [--lengths 100,150] [--communities 16] [--members 8] [--reads 500000]

--experiment: the recorded experiment of DESIGN.md 11, no pass mark - a model trained on the 30 fixture genomes
(tests/golden/genomes/genomes30.npz), a copy of it with the weights fitted (training.refit_model_dir: what --fit-weights writes), and
validation.validate of both on the same random communities: median and maximum unsigned error per read length, one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import wfit_restated as wr  # noqa: E402
from microbecensus_amd import _native  # noqa: E402


def experiment(a):
    import gzip
    import shutil
    import tempfile
    import community_restated as cr
    from microbecensus_amd import training, validation
    quiet = dict(log=lambda *x: None)
    lengths = [int(x) for x in a.lengths.split(",")]
    with tempfile.TemporaryDirectory() as td:
        gdir = os.path.join(td, "genomes")
        os.makedirs(gdir)
        for name, bases, off in cr.fixture_members():
            with gzip.open(os.path.join(gdir, name + ".fna.gz"), "wb", compresslevel=1) as f:
                for c in range(len(off) - 1):
                    f.write(b">%s_%d\n%s\n" % (name.encode(), c, bases[off[c]:off[c + 1]].tobytes()))
        plain, fitted = os.path.join(td, "plain"), os.path.join(td, "fitted")
        training.train(gdir, plain, lengths, a.coverage, device=a.device, **quiet)
        shutil.copytree(plain, fitted)
        model = training.refit_model_dir(fitted, device=a.device, **quiet)
        out = {"genomes": 30, "coverage": a.coverage, "communities": a.communities, "members": a.members, "reads": a.reads, "weights_fit": model["weights_fit"]}
        for tag, md in (("weights_1.0", plain), ("weights_fitted", fitted)):
            rec = validation.validate(gdir, os.path.join(td, "val_" + tag), lengths, a.reads, model_dir=md, random=a.communities, members=a.members, seed=11, device=a.device,
                                      **quiet)
            out[tag] = {str(L): {"median_unsigned_error": m, "max_unsigned_error": x} for L, (m, x) in validation.unsigned_error_summary(rec).items()}
        print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("-g", dest="device", type=int, default=0)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--host-generations", type=int, default=2)
    p.add_argument("--experiment", action="store_true")
    p.add_argument("--coverage", type=float, default=5.0)
    p.add_argument("--lengths", default="100,150")
    p.add_argument("--communities", type=int, default=16)
    p.add_argument("--members", type=int, default=8)
    p.add_argument("--reads", type=int, default=500000)
    a = p.parse_args()
    if a.experiment:
        return experiment(a)
    eng = _native.Engine(device=a.device)
    try:
        for N in (30, 150, wr.MAX_N):
            pred, truth = wr.planted(1, N=N, F=30)
            eng.fit_weights(pred, truth, 0, 100, 64, 2)                               # (warm-up: the code object is loaded)
            ms, wall = [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                w, trace = eng.fit_weights(pred, truth, 0, 100)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(eng.fit_weights_ms())
            ran = int((trace[1:, 1] >= 0).sum())
            t0 = time.perf_counter()
            hw, ht = wr.fit(pred, truth, 0, 100, wr.DEFAULT_C, a.host_generations)
            host = (time.perf_counter() - t0) * 1e3
            same = bool((ht.view("u8") == trace[:a.host_generations + 1].view("u8")).all())
            print(json.dumps({"N": N, "F": 30, "candidates": wr.DEFAULT_C, "generations": wr.DEFAULT_G, "generations_run": ran,
                              "kernels_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                              "call_ms_median": round(statistics.median(wall), 3), "mue_start": trace[0, 0], "mue_fitted": trace[-1, 0],
                              "host_ms_per_generation": round(host / max(a.host_generations, 1), 1), "host_ms_scaled": round(host / max(a.host_generations, 1) * ran, 0),
                              "host_trace_prefix_identical": same}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
