#!/usr/bin/env python3
"""Timings of the community simulator, one process, warm-up first, median of the repetitions with min - max.

    community_timing.py genome    [--root TREE]   the simulate kernel of a GENOME library (mc_train_library's HIP events) on the 30 fixture
                                                  genomes opened as one genome of 251 contigs; --root: the tree whose package and built
                                                  library are measured (the parent commit's, to compare against)
    community_timing.py community                 the simulate kernel of a COMMUNITY library (mc_community_library's HIP events) on the
                                                  same 30 genomes as 30 members with uneven copies
    community_timing.py fused                     a fused pass (mc_community_library) against simulate-to-host + mc_search with best hits
                                                  only: wall and HIP events
Every mode runs the default kind and Illumina errors with mate pairs (insert 400); --reads (2,000,000), --read-len (150), --reps (9).
Prints one JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"default": {}, "illumina_paired": dict(error_model="illumina", paired_end=True, insert=400)}


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "reps": len(v)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("genome", "community", "fused"))
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--reads", type=int, default=2000000)
    p.add_argument("--read-len", type=int, default=150)
    p.add_argument("--reps", type=int, default=9)
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import numpy as np
    from microbecensus_amd import _native, training
    import community_restated as cr
    members = [(b, o) for _, b, o in cr.fixture_members()]
    bases, off, _ = cr.join_members(members)
    rng = np.random.Generator(np.random.PCG64(20261016))
    copies = np.maximum(1, np.floor(rng.lognormal(0.0, 1.5, len(members)) * 30000)).astype(np.int64).tolist()
    model = _native.load_model()
    L, n = a.read_len, a.reads
    eng = _native.Engine(device=0)
    eng.set_run(L, model["pars"][str(L)], model["families"])
    lid = training.library_id("thirty", L)
    src = _native.Genome(bases, off, 0) if a.what == "genome" else _native.Community(members, copies, 0)
    for kname, kind in KINDS.items():
        src.set_library(**kind)
        out = {"what": a.what, "kind": kname, "reads": n, "read_len": L, "contigs": len(off) - 1}
        if a.what == "genome":
            ms = []
            for rep in range(a.reps + 2):
                eng.train_library(src, n, rep, lid, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)
                ms.append(eng.train_times()["simulate"])
            out["simulate_ms"] = spread(ms[2:])
        elif a.what == "community":
            ms = []
            for rep in range(a.reps + 2):
                eng.community_library(src, n, rep, lid)
                ms.append(eng.community_times()["simulate"])
            out["simulate_ms"] = spread(ms[2:])
        else:
            fw, fe, sw, se, sim_w = [], [], [], [], []
            eng.set_best_hits_only(False)
            for rep in range(a.reps + 2):
                t0 = time.perf_counter()
                eng.community_library(src, n, rep, lid)
                fw.append(1e3 * (time.perf_counter() - t0))
                t = eng.community_times()
                fe.append(t["simulate"] + t["search"])
                t0 = time.perf_counter()
                reads = src.simulate(L, n, rep, lid)
                t1 = time.perf_counter()
                eng.set_best_hits_only(True)
                eng.search(reads)
                eng.set_best_hits_only(False)
                t2 = time.perf_counter()
                sim_w.append(1e3 * (t1 - t0)); sw.append(1e3 * (t2 - t0)); se.append(eng.stats()["ms_total"])
            out.update(fused_wall_ms=spread(fw[2:]), fused_event_ms=spread(fe[2:]), staged_wall_ms=spread(sw[2:]), staged_simulate_to_host_wall_ms=spread(sim_w[2:]),
                       staged_search_event_ms=spread(se[2:]))
        print(json.dumps(out), flush=True)
    src.close()
    eng.close()


if __name__ == "__main__":
    main()
