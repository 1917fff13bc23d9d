#!/usr/bin/env python3
"""Timings of the gene counts on reads of mixed lengths, one process, warm-up first, the sides alternating within the
call (tools/classes_timing.py's idiom), median of the repetitions with min - max.

    abund_classes_timing.py      file -> counts on a synthetic FASTQ of --reads reads spread evenly over 80 .. 150 bp (written to --dir),
                                 the packaged markers as the genes: under the switch (a class reader, Engine.set_run_classes with the
                                 model's default classes for the file, set_abundance + set_abundance_classes, search_files, the two reads
                                 of the tables) against the fixed-length run of the same file (the auto-detected -l), and a third side, the
                                 switch with the gene bootstrap's list on.  Per side the wall time, the reads and bases sampled and the
                                 reads assigned; for the switch also the event times of its kernels (k_abund_class_add over the pieces;
                                 k_geneboot_collect_mapped on the third side) and the class prologue's event time on the same rows
                                 (mc_debug_classes_prologue, batch by batch) as a share of the wall time.
NOT measured by this tool: the run with the switch off against the parent commit's (tools/abundance_timing.py files --root TREE does that),
and the per-batch hipMalloc / hipMemcpy costs of a class batch, which are part of the wall time above.
Prints one JSON line; --reads (1,000,000), --reps (7)."""
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
    p.add_argument("--dir", default="/tmp")
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    from microbecensus_amd import _native, synth, microbe_census as mc
    _, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=8_000_000, seed=5, marker_gene_fraction=0.05)
    full = synth.sample_reads(genome, a.reads, 150, seed=6)
    lens = np.random.default_rng(7).integers(80, 151, size=a.reads)
    path = os.path.join(a.dir, "abund_classes_timing_%d.fq" % a.reads)
    with open(path, "wb") as f:
        for i in range(a.reads):
            s = full[i, :lens[i]].tobytes()
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    valid = list(mc._valid_read_lengths())
    classes = mc.auto_detect_length_classes(path, valid)
    L = mc.auto_detect_read_length(path, "fastq", None)
    qoff = mc.auto_detect_quality_offset(path)
    sampler = (a.reads, True, qoff, -5, -5, 100, False)
    eng = _native.Engine(device=0)
    wall = {"mixed": [], "fixed": [], "mixed_boot": []}
    used, cls_ms, collect_ms = {}, [], []
    try:
        for rep in range(a.reps + 1):
            for side in ("mixed", "fixed", "mixed_boot"):
                mixed = side != "fixed"
                rd = _native.Reader.with_classes([path], classes, *sampler) if mixed else _native.Reader([path], L, *sampler)
                try:
                    t0 = time.perf_counter()
                    if mixed:
                        eng.set_run_classes(classes)
                    else:
                        eng.set_run(L)
                    eng.set_abundance(True)
                    if mixed:
                        eng.set_abundance_classes(True)
                    if side == "mixed_boot":
                        eng.set_gene_bootstrap(a.reads)
                    eng.search_files(rd, keep_rows=False)
                    ab = eng.abundance()
                    ac = eng.abundance_classes() if mixed else None
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep:
                        wall[side].append(dt)
                        if side == "mixed":
                            cls_ms.append(eng.abundance_classes_ms())
                        if side == "mixed_boot":
                            collect_ms.append(eng.gene_bootstrap_ms())
                    bases = int(sum(int(n) * c for n, c in zip(ac["rows"], classes))) if mixed else ab["searched"] * L
                    used[side] = {"length": classes if mixed else L, "sampled_reads": ab["searched"], "sampled_bases": bases, "reads_assigned": ab["assigned"]}
                    if mixed:
                        used[side]["class_reads"] = [int(x) for x in ac["rows"]]
                        used[side]["class_reads_assigned"] = [int(x) for x in ac["assigned"]]
                finally:
                    eng.set_abundance(False)
                    rd.close()
        # the class prologue on the same rows, in batches the debug entry takes
        rd = _native.Reader.with_classes([path], classes, *sampler)
        try:
            n = rd.run()
            rows = rd.reads(n)
            eng.set_run_classes(classes)
            step = (1 << 21) - 1
            pro = []
            for rep in range(a.reps + 1):
                ms = 0.0
                for lo in range(0, n, step):
                    t = eng.classes_prologue(rows[lo:lo + step], want_sorted=False)[4]
                    ms += t[0] + t[1]
                if rep:
                    pro.append(ms)
        finally:
            rd.close()
    finally:
        eng.close()
        os.remove(path)
    print(json.dumps({"figure": "abund_classes_files", "file_reads": a.reads, "file_bases": int(lens.sum()), "mixed_wall_ms": spread(wall["mixed"]), "fixed_wall_ms": spread(wall["fixed"]),
                      "mixed_with_bootstrap_list_wall_ms": spread(wall["mixed_boot"]), "used": used, "class_add_kernel_ms": spread(cls_ms), "collect_mapped_kernel_ms": spread(collect_ms),
                      "prologue_ms": spread(pro), "prologue_share_of_mixed_wall": round(statistics.median(pro) / statistics.median(wall["mixed"]), 4)}))


if __name__ == "__main__":
    main()
