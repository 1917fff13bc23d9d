#!/usr/bin/env python3
"""The measurements of DESIGN.md 13.14 (GPU box), one process per mode, warm-up first, median with min - max.  One JSON line per figure.
The reads: 1 M reads of 150 bp of bench.py's read recipe (the 30 genomes) against the marker database - the README's abundance leg.

    depthstats_timing.py read        coverage and ties ON, one search; then per read (reps + 1 times, the first dropped): depth_stats(80) - the
                                     selection kernel (depth_stats_ms()) and the wall time of the call -, the same with any=True, coverage() - the
                                     scan of mc_coverage_read (coverage_ms()) - and THE HOST ROUTE: coverage_depth() and a numpy sort per gene with
                                     reads (wall time, bytes copied), whose figures must equal the device's
    depthstats_timing.py one_gene    a database of ONE gene (the longest marker) and reads sampled from its back-translation: every assigned read
                                     in one gene - the deepest pile a workgroup meets; depth_stats(80) as above
    depthstats_timing.py long_gene   a gene of 65,535 residues (markers one after the other) under a gene fold, reads of the marker-dense
                                     library: the path that scans the difference array again in every walk; depth_stats(80) as above
    depthstats_timing.py files [--root TREE]
                                     wall time of file -> counts with every switch of this feature OFF: search_files(keep_rows=False) +
                                     abundance() on a FASTA of the reads; --root names the tree whose package and built library are measured -
                                     this tree and the parent commit's in turn, process after process, three runs each
--reads (1,000,000), --dense-reads (100,000), --reps (3)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAG = {}
FIGURES = ("median", "trimmed_sum", "low", "high")


def emit(d):
    print(json.dumps(dict(d, **TAG)), flush=True)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v)}


def timed_reads(a, eng, label, any_too):
    """depth_stats(80) reps + 1 times: the kernel's milliseconds and the call's wall time; returns the last figures"""
    ab = eng.abundance()
    for any_ in (False, True) if any_too else (False,):
        t = {"kernel": [], "wall": []}
        for rep in range(a.reps + 1):
            before = eng.depth_stats_ms()
            t0 = time.perf_counter()
            st = eng.depth_stats(80, any=any_)
            t["wall"].append(1e3 * (time.perf_counter() - t0))
            t["kernel"].append(eng.depth_stats_ms() - before)
        emit({"what": "depth_stats", "case": label, "any": any_, "keep": 80, "genes": int(eng.abundance_count()), "genes_with_reads": int((ab["reads"] > 0).sum()), "assigned": ab["assigned"],
              "largest_gene_reads": int(ab["reads"].max()), "max_high": int(st["high"].max()), "genes_median_gt0": int((st["median"] > 0).sum()), "k_depth_select_ms": spread(t["kernel"][1:]),
              "depth_stats_wall_ms": spread(t["wall"][1:])})
        if not any_:
            own = st
    return own, ab


def host_route(a, eng, lengths, want, ab):
    """mc_coverage_depth and a sort per gene with reads, in numpy: the figures are the device's"""
    off = np.concatenate([[0], np.cumsum(lengths)])
    wall, copy = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        depth = eng.coverage_depth()
        t1 = time.perf_counter()
        got = {k: np.zeros(len(lengths), np.int64) for k in FIGURES}
        for s in np.flatnonzero(ab["reads"]):
            x = np.sort(depth[off[s]:off[s + 1]].astype(np.int64))
            n = len(x)
            cut = n * 20 // 200
            got["median"][s], got["trimmed_sum"][s], got["low"][s], got["high"][s] = x[(n - 1) // 2], x[cut:n - cut].sum(), x[cut], x[n - cut - 1]
        wall.append(1e3 * (time.perf_counter() - t0)); copy.append(1e3 * (t1 - t0))
    assert all(np.array_equal(got[k], want[k]) for k in FIGURES), "the host route and the device disagree"
    emit({"what": "host_route", "genes": len(lengths), "genes_sorted": int((ab["reads"] > 0).sum()), "depth_bytes": int(depth.nbytes), "coverage_depth_wall_ms": spread(copy[1:]),
          "host_route_wall_ms": spread(wall[1:]), "equal_to_device": True})


def read(a, _native, synth):
    L = 150
    model = _native.load_model()
    seqs = _native.load_markers()[1]
    eng = _native.Engine(device=0)
    try:
        eng.set_run(L, model["pars"][str(L)], model["families"])
        eng.set_abundance(True)
        eng.set_coverage(True)
        eng.set_ties(True)
        eng.search(synth.GenomeReads(device="cpu", seed=20261001).single(a.reads, L).numpy(), keep_rows=False)
        want, ab = timed_reads(a, eng, "bench reads, marker database", True)
        scan = []
        for rep in range(a.reps + 1):
            before = eng.coverage_ms()
            eng.coverage()
            scan.append(eng.coverage_ms() - before)
        emit({"what": "coverage_scan", "genes": len(seqs), "k_coverage_scan_ms": spread(scan[1:])})
        host_route(a, eng, [len(s) for s in seqs], want, ab)
    finally:
        eng.close()


def one_gene(a, _native, synth):
    L = 150
    names, seqs = _native.load_markers()
    g = max(range(len(seqs)), key=lambda k: len(seqs[k]))
    eng = _native.Engine(device=0, names=[names[g]], seqs=[seqs[g]], marker_family=[0], nfam=1)
    try:
        eng.set_run(L)
        eng.set_abundance(True)
        eng.set_coverage(True)
        eng.search(synth.sample_reads(synth.build_genomes([seqs[g]], total_bp=200_000, seed=404, marker_gene_fraction=1.0), a.dense_reads, L, seed=405), keep_rows=False)
        timed_reads(a, eng, "every read in one gene of %d residues" % len(seqs[g]), False)
    finally:
        eng.close()


def long_gene(a, _native, synth, abundance):
    L = 150
    names, seqs = _native.load_markers()
    joined = "".join(seqs[:400])[:abundance.MAX_LONG_GENE_LEN]
    assert len(joined) == abundance.MAX_LONG_GENE_LEN
    gn, gs = ["long"] + list(names[400:500]), [joined] + list(seqs[400:500])
    sp = abundance.split_genes(gn, gs)
    eng = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"])
    try:
        eng.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
        eng.set_run(L)
        eng.set_abundance(True)
        eng.set_coverage(True)
        eng.search(synth.sample_reads(synth.build_genomes(seqs[:500], total_bp=3_000_000, seed=404, marker_gene_fraction=1.0), a.dense_reads, L, seed=405), keep_rows=False)
        want, ab = timed_reads(a, eng, "a gene of %d residues in gene space, %d segments" % (len(joined), len(sp["seg_names"])), False)
        host_route(a, eng, [int(n) for n in sp["gene_len"]], want, ab)
    finally:
        eng.close()


def files(a, _native, synth):
    L = 150
    model = _native.load_model()
    eng = _native.Engine(device=0)
    reads = synth.GenomeReads(device="cpu", seed=20261001).single(a.reads, L).numpy()
    n = len(reads)
    try:
        eng.set_run(L, model["pars"][str(L)], model["families"])
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "reads.fa")
            with open(fa, "wb") as f:
                for s in range(0, n, 50000):
                    f.write(b"".join(b">r%d\n%s\n" % (s + i, bytes(r)) for i, r in enumerate(reads[s:s + 50000])))
            wall = []
            for rep in range(a.reps + 1):
                rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
                try:
                    eng.set_abundance(True)
                    t0 = time.perf_counter()
                    eng.search_files(rd, keep_rows=False)
                    got = eng.abundance()
                    wall.append(1e3 * (time.perf_counter() - t0))
                finally:
                    rd.close()
        emit({"what": "files", "root": os.path.relpath(a.root), "has_switch": hasattr(eng, "depth_stats"), "reads": n, "assigned": got["assigned"], "wall_ms": spread(wall[1:]),
              "wall_ms_all": [round(w, 2) for w in wall[1:]]})
        eng.set_abundance(False)
    finally:
        eng.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("read", "one_gene", "long_gene", "files"))
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--dense-reads", type=int, default=100000)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--tag", default=None, help="whose code runs: every line printed carries it as \"tree\"")
    a = p.parse_args()
    if a.tag:
        TAG["tree"] = a.tag
    sys.path.insert(0, os.path.abspath(a.root))
    from microbecensus_amd import _native, abundance, synth
    if a.what == "read":
        read(a, _native, synth)
    elif a.what == "one_gene":
        one_gene(a, _native, synth)
    elif a.what == "long_gene":
        long_gene(a, _native, synth, abundance)
    else:
        files(a, _native, synth)


if __name__ == "__main__":
    main()
