#!/usr/bin/env python3
"""Development aid (GPU box): what a batch of mixed read lengths costs.  2 M reads of uniform lengths 60..300 through
mc_search_varlen (about 240 length buckets, each through the fixed-length pipeline) against 2 M reads of 150 bp through mc_search,
both cut from the 30 fixture genomes; and one training library pass (mc_train_library) of --train-reads reads at 150 bp with illumina
errors, the default read-length mode against the reference mode (seq_sim.py's lengths, bucketed).  Each is run once to warm up and then
timed (wall clock, host to host).

    python tools/varlen_timing.py [--reads 2000000] [--lo 60] [--hi 300] [--fixed 150] [--repeats 2] [--device 0]

Prints one JSON line: wall seconds, reads/s and the kernels' own milliseconds (mc_stats.ms_total) of each path."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from microbecensus_amd import _native, synth, training  # noqa: E402


def timed(fn, repeats):
    fn()                                                              # warm-up: pools, staging buffers, tables
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reads", type=int, default=2_000_000)
    p.add_argument("--lo", type=int, default=60)
    p.add_argument("--hi", type=int, default=300)
    p.add_argument("--fixed", type=int, default=150)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--train-reads", type=int, default=2_000_000)
    a = p.parse_args()
    n = a.reads
    reads = synth.GenomeReads(device="cpu", seed=31).single(n, a.hi).numpy()
    lens = np.random.RandomState(5).randint(a.lo, a.hi + 1, n).astype(np.int64)
    mask = np.arange(a.hi)[None, :] < lens[:, None]
    bases = np.ascontiguousarray(reads[mask])
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    fixed = np.ascontiguousarray(reads[:, :a.fixed])
    eng = _native.Engine(device=a.device)
    try:
        eng.set_run(a.fixed)
        t_fixed = timed(lambda: eng.search(fixed), a.repeats)
        st_fixed = eng.stats()
        t_var = timed(lambda: eng.search_varlen((bases, off)), a.repeats)
        st_var = eng.stats()
        gb, goff = synth.load_genomes()
        g = _native.Genome(gb, goff, a.device)
        train = {}
        try:
            g.set_library("illumina")
            eng.set_run(150)
            for mode in (False, True):
                g.set_read_lengths(mode)
                t = timed(lambda: eng.train_library(g, a.train_reads, 1, 2, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES), a.repeats)
                train["reference" if mode else "fixed"] = {"wall_s": round(t, 4), "bases": eng.train_library_bases(), "times_ms": eng.train_times()}
        finally:
            g.close()
    finally:
        eng.close()
    print(json.dumps({"reads": n, "varlen": {"lengths": [a.lo, a.hi], "buckets": int(len(np.unique(lens))), "bases": int(off[-1]), "wall_s": round(t_var, 4),
                                             "reads_per_s": round(n / t_var), "kernel_ms": round(st_var["ms_total"], 2), "rows": st_var["rows"]},
                      "fixed": {"read_len": a.fixed, "wall_s": round(t_fixed, 4), "reads_per_s": round(n / t_fixed), "kernel_ms": round(st_fixed["ms_total"], 2),
                                "rows": st_fixed["rows"]},
                      "varlen_over_fixed": round(t_var / t_fixed, 3),
                      "train_150bp_illumina": dict(train, reads=a.train_reads, reference_over_fixed=round(train["reference"]["wall_s"] / train["fixed"]["wall_s"], 3))}))


if __name__ == "__main__":
    sys.exit(main())
