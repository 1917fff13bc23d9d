#!/usr/bin/env python3
"""Timings of a length-class run, one process, warm-up first, median of the repetitions with min - max.

    classes_timing.py prologue   the device prologue of a class run (mc_debug_classes_prologue's HIP events: [0] row lengths, classes,
                                 scan and scatter, [1] the trimming gather) on --reads rows of lengths spread evenly over
                                 0.53 .. 1 x stride, at strides 150 and 300 under the model's classes; the gather's achieved bytes/s
                                 (bytes read + bytes written of the trimmed reads) beside it
    classes_timing.py search     mc_search_classes on synthetic reads of 80 .. 150 bp against mc_search at 110 bp on the reads that
                                 reach 110 bp (what the single-length run keeps), alternating, wall time and reads / bases used
    classes_timing.py pipeline   file to AGS: run_pipeline on a synthetic FASTQ of --reads reads of 80 .. 150 bp (written to --dir) with the
                                 switch against the same file without it (the auto-detected -l), alternating, wall time and the reads
                                 and bases each side used
NOT measured by this tool: the prologue against vl_bucket on the same reads given as offsets (vl_bucket has no entry of its own in
the ABI), a run without the switch against the parent commit's (pipeline's "single" side is this tree's), and the accuracy run
(scripts/validate_microbe_census.py --length-mix does that one).
Prints one JSON line per figure; --reads (2,000,000, at most 2,097,151 for the prologue), --reps (9)."""
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
    p.add_argument("what", choices=("prologue", "search", "pipeline"))
    p.add_argument("--dir", default="/tmp")
    p.add_argument("--reads", type=int, default=2000000)
    p.add_argument("--reps", type=int, default=9)
    a = p.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from microbecensus_amd import _native, synth
    model = _native.load_model()
    valid = sorted(int(L) for L in model["pars"])
    if a.what == "pipeline":
        from microbecensus_amd import microbe_census as mc
        _, seqs = _native.load_markers()
        genome = synth.build_genomes(seqs, total_bp=8_000_000, seed=5, marker_gene_fraction=0.05)
        full = synth.sample_reads(genome, a.reads, 150, seed=6)
        lens = np.random.default_rng(7).integers(80, 151, size=a.reads)
        path = os.path.join(a.dir, "classes_timing_%d.fq" % a.reads)
        with open(path, "wb") as f:
            for i in range(a.reads):
                s = full[i, :lens[i]].tobytes()
                f.write(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
        t_mixed, t_single, used = [], [], {}
        for rep in range(a.reps + 1):
            for side, extra in (("mixed", {"mixed_lengths": True}), ("single", {})):
                t0 = time.perf_counter()
                est, r = mc.run_pipeline(dict({"seqfiles": [path], "outfile": os.path.join(a.dir, "classes_timing.out"), "nreads": a.reads, "device": 0}, **extra))
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    (t_mixed if side == "mixed" else t_single).append(dt)
                bases = sum(n * L for n, L in zip(r["class_reads"], r["length_classes"])) if side == "mixed" else r["sampled_reads"] * r["read_length"]
                used[side] = {"ags": est, "reads": r["sampled_reads"], "bases": int(bases), "length": r.get("length_classes", r["read_length"])}
        os.remove(path)
        print(json.dumps({"figure": "classes_pipeline", "file_reads": a.reads, "file_bases": int(lens.sum()), "mixed_ms": spread(t_mixed), "single_ms": spread(t_single), "used": used}))
        return
    eng = _native.Engine(device=0)
    if a.what == "prologue":
        n = min(a.reads, (1 << 21) - 1)
        for stride in (150, 300):
            classes = [L for L in valid if stride * 0.5 <= L <= stride]
            rng = np.random.default_rng(stride)
            lens = rng.integers(int(stride * 0.53), stride + 1, size=n)
            rows = rng.integers(65, 85, size=(n, stride), dtype=np.uint8)
            rows[np.arange(stride)[None, :] >= lens[:, None]] = 0
            eng.set_run_classes(classes)
            eng.classes_prologue(rows, want_sorted=False)
            front, gather = [], []
            for _ in range(a.reps):
                _, start, word0, _, ms = eng.classes_prologue(rows, want_sorted=False)
                front.append(ms[0]); gather.append(ms[1])
            moved = 2 * int(word0[-1]) * 16
            print(json.dumps({"figure": "classes_prologue", "stride": stride, "rows": n, "classes": classes, "front_ms": spread(front), "gather_ms": spread(gather),
                              "gather_bytes": moved, "gather_GBps_median": round(moved / statistics.median(gather) / 1e6, 1)}))
    else:
        _, seqs = _native.load_markers()
        genome = synth.build_genomes(seqs, total_bp=8_000_000, seed=5, marker_gene_fraction=0.05)
        full = synth.sample_reads(genome, a.reads, 150, seed=6)
        lens = np.random.default_rng(7).integers(80, 151, size=a.reads)
        rows = full.copy()
        rows[np.arange(150)[None, :] >= lens[:, None]] = 0
        classes = [L for L in valid if 80 <= L <= 150]
        single = np.ascontiguousarray(full[lens >= 110, :110])
        pars = {L: model["pars"][str(L)] for L in classes}
        t_mixed, t_single = [], []
        for rep in range(a.reps + 1):
            eng.set_run_classes(classes, pars, model["families"])
            eng.set_best_hits_only(True)
            t0 = time.perf_counter(); best, cls, class_reads = eng.search_classes(rows); t1 = time.perf_counter()
            eng.set_run(110, model["pars"]["110"], model["families"])
            eng.set_best_hits_only(True)
            t2 = time.perf_counter(); _, b1 = eng.search(single); t3 = time.perf_counter()
            if rep:
                t_mixed.append((t1 - t0) * 1e3); t_single.append((t3 - t2) * 1e3)
        used = int(sum(n * L for n, L in zip(class_reads[:-1], classes)))
        print(json.dumps({"figure": "classes_search", "mixed_ms": spread(t_mixed), "single_ms": spread(t_single), "mixed_reads": int(class_reads[:-1].sum()), "mixed_bases": used,
                          "single_reads": int(len(single)), "single_bases": int(len(single)) * 110, "mixed_best": int(len(best)), "single_best": int(len(b1))}))
    eng.close()


if __name__ == "__main__":
    main()
