#!/usr/bin/env python3
"""Timings of long genes, one process, warm-up first, median of the repetitions with min - max.

    long_genes_timing.py off     file to counts with the switch OFF: run_abundance on a synthetic FASTQ of --reads reads of 150 bp (written to
                                 --dir) against the packaged markers under --ags, wall time.  Run it on this commit and on the one before
                                 it: the figure to compare (the parent ignores the key it does not know).
    long_genes_timing.py fold    k_fold beside k_abundance: the engine on every second marker cut at --seg-len (768: 525 genes split), --reads
                                 reads of 150 bp searched with the rows staying on the device; k_fold's and the counting kernel's HIP-event
                                 milliseconds, the rows folded, edge_rows
    long_genes_timing.py split   the end-to-end input of tests/test_gpu_fold.py: the example reads against every second marker, unsplit and cut at
                                 --seg-len, one engine after the other: wall time of the search with counts, coverage and ties, and the engines' open time
NOT measured by this tool: a database of genes that are really longer than the engine's limit (none is packaged).
Prints one JSON line per figure; --reads (1,000,000), --reps (7)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "reps": len(v)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("off", "fold", "split"))
    p.add_argument("--dir", default="/tmp")
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seg-len", type=int, default=768)
    a = p.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from microbecensus_amd import _native, abundance, synth
    names, seqs = _native.load_markers()
    if a.what in ("off", "fold"):
        genome = synth.build_genomes(seqs, total_bp=8_000_000, seed=5, marker_gene_fraction=0.05)
        reads = synth.sample_reads(genome, a.reads, 150, seed=6)
    if a.what == "off":
        path = os.path.join(a.dir, "long_genes_timing_%d.fq" % a.reads)
        with open(path, "wb") as f:
            for i in range(a.reads):
                f.write(b"@r%d\n%s\n+\n%s\n" % (i, reads[i].tobytes(), b"I" * 150))
        t, kernel = [], []
        for rep in range(a.reps + 1):
            args = {"seqfiles": [path], "genes": os.path.join(_native.DATA_DIR, "markers.faa.gz"), "nreads": a.reads, "read_length": 150, "device": 0, "ags": 3.0e6, "long_genes": False}
            t0 = time.perf_counter()
            table, args = abundance.run_abundance(args)
            if rep:
                t.append((time.perf_counter() - t0) * 1e3); kernel.append(args["search_ms"])
        os.remove(path)
        print(json.dumps({"figure": "long_genes_off", "reads": a.reads, "wall_ms": spread(t), "search_ms": spread(kernel), "assigned": int(table["reads_assigned"])}))
        return
    names, seqs = names[::2], seqs[::2]               # (every second marker: all of them cut at 768 overfill a seed bucket, DESIGN.md 13.7 "Known limit")
    sp = abundance.split_genes(names, seqs, seg_len=a.seg_len, overlap=abundance.SEG_OVERLAP)

    def engine(split):
        t0 = time.perf_counter()
        if split:
            e = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"])
            e.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
        else:
            e = _native.Engine(device=0, names=names, seqs=seqs, marker_family=[0] * len(names), nfam=1)
        return e, (time.perf_counter() - t0) * 1e3

    if a.what == "fold":
        e, _ = engine(True)
        e.set_run(150)
        e.set_abundance(True)
        e.lib.mc_set_keep_rows(e.h, 0)
        fold, count, wall = [], [], []
        for rep in range(a.reps + 1):
            e.abundance_reset()
            t0 = time.perf_counter(); e.search(reads); dt = (time.perf_counter() - t0) * 1e3
            fs = e.gene_fold_stats()
            if rep:
                fold.append(fs["ms"]); count.append(e.abundance_ms()); wall.append(dt)
        print(json.dumps({"figure": "long_genes_fold", "reads": a.reads, "seg_len": a.seg_len, "genes": len(names), "genes_split": sp["genes_split"], "segments": len(sp["seg_names"]),
                          "k_fold_ms": spread(fold), "k_abundance_ms": spread(count), "search_wall_ms": spread(wall), "rows": int(e.stats()["rows"]) if "rows" in e.stats() else None,
                          "edge_rows": fs["edge_rows"], "assigned": e.abundance()["assigned"]}))
        e.close()
        return
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import abund_inputs
    reads = abund_inputs.example_reads()
    out = {}
    for split in (False, True):
        e, open_ms = engine(split)
        e.set_run(100); e.set_abundance(True); e.set_coverage(True); e.set_ties(True)
        e.lib.mc_set_keep_rows(e.h, 0)
        t = []
        for rep in range(a.reps + 1):
            e.abundance_reset()
            t0 = time.perf_counter(); e.search(reads); dt = (time.perf_counter() - t0) * 1e3
            if rep:
                t.append(dt)
        out["split" if split else "unsplit"] = {"open_ms": round(open_ms, 1), "search_wall_ms": spread(t), "search_ms": round(e.stats()["ms_total"], 3), "assigned": e.abundance()["assigned"],
                                                 "sequences": len(sp["seg_names"]) if split else len(names)}
        if split:
            out["split"].update(e.gene_fold_stats())
        e.close()
    print(json.dumps(dict({"figure": "long_genes_split", "reads": int(len(reads)), "seg_len": a.seg_len, "genes_split": sp["genes_split"]}, **out)))


if __name__ == "__main__":
    main()
