#!/usr/bin/env python3
"""Times one training library pass (mc_train_library: simulate -> search -> grid, rows never leave the device) per read length on
one GPU, split by HIP events into simulate / search / grid.  The genome is the 30 genomes of tests/golden/genomes/genomes30.npz
taken as one (84.8 Mbp, 193 contigs); every pass is run once to warm up and then timed.

    python tools/train_timing.py [--reads 4000000] [--lengths 100,150,300] [--device 0]
                                 [--error-model illumina|uniform [--error-rate R]] [--paired-end --insert I]

Prints one JSON line per read length: shape (genome bp, L, reads, batch), wall seconds, reads/s, and the split in ms."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from microbecensus_amd import _native, training  # noqa: E402


def genome30():
    d = np.load(os.path.join(REPO, "tests", "golden", "genomes", "genomes30.npz"))
    packed, off = d["packed"], d["contig_off"]
    codes = np.stack([(packed >> (2 * k)) & 3 for k in range(4)], axis=1).reshape(-1)[: off[-1]]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    bases[d["exc_pos"]] = d["exc_chr"]
    return bases, off.astype(np.int64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reads", type=int, default=4000000)
    p.add_argument("--lengths", default="100,150,300")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--error-model", choices=training.ERROR_MODELS, default=None)
    p.add_argument("--error-rate", type=float, default=None)
    p.add_argument("--paired-end", action="store_true")
    p.add_argument("--insert", type=int, default=None)
    a = p.parse_args()
    if a.reads % 2 and a.paired_end:
        p.error("--paired-end takes an even --reads")
    bases, off = genome30()
    eng = _native.Engine(device=a.device)
    g = _native.Genome(bases, off, a.device)
    g.set_library(a.error_model, a.error_rate, a.paired_end, a.insert)
    library = training.library_record(a.error_model, a.error_rate, a.paired_end, a.insert)
    batch = int(os.environ.get("MC_STREAM_BATCH", "2000000"))
    for L in [int(x) for x in a.lengths.split(",")]:
        eng.set_run(L)
        args = (g, a.reads, 1, training.library_id("genome30", L), training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)
        eng.train_library(*args)                                        # warm-up: pools, kernels
        t0 = time.perf_counter()
        hits, _, _ = eng.train_library(*args)
        wall = time.perf_counter() - t0
        ms = eng.train_times()
        st = eng.stats()
        print(json.dumps({"library": library, "genome_bp": int(off[-1]), "contigs": int(len(off) - 1), "L": L, "reads": a.reads, "batch": min(batch, a.reads),
                          "wall_s": round(wall, 4), "reads_per_s": round(a.reads / wall), "ms_simulate": round(ms["simulate"], 2),
                          "ms_search": round(ms["search"], 2), "ms_grid": round(ms["grid"], 2), "rows": st["rows"], "range_splits": st["range_splits"],
                          "reads_classified_at_loosest_cutoff": int(hits[0, -1, 0].sum())}), flush=True)
    g.close()
    eng.close()


if __name__ == "__main__":
    main()
