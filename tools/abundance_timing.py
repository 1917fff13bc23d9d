#!/usr/bin/env python3
"""The measurements of DESIGN.md 13 (GPU box), one process per mode, warm-up first, the two sides of a comparison alternating inside the
repetition loop, median with min - max.  One JSON line per figure.

    abundance_timing.py kernel               abundance_ms() against stats()["ms_total"] of the same ranges: 1 M reads of 150 bp of bench.py's
                                             read recipe on the marker database (few hits), and the marker-dense library of
                                             tests/test_gpu_abundance.py (about 100 rows per read) in ranges of 5,000 reads
    abundance_timing.py files [--root TREE]  wall time of search_files(keep_rows=False) on a FASTA of the same reads with the counts on and
                                             off, alternating; --root: the tree whose package and built library are measured - the parent
                                             commit's has no switch and gives the off side alone
    abundance_timing.py host                 what the kernel replaces: search_files(keep_rows=True) + numpy counting of the rows on the host,
                                             against the counts on with keep_rows=False
--reads (1,000,000), --dense-reads (100,000), --reps (7).
--coverage (kernel, files): coverage breadth and depth beside the counts (Engine.set_coverage; csrc/k_coverage.h), the two sides alternating
inside the repetition loop: `kernel` adds abundance_ms() with the marks riding in the counting kernel and coverage_ms() of one
coverage() read (the scan); `files` adds the wall time of file -> counts + coverage() with the switch on.  A tree without the switch
(the parent commit's) gives the off sides alone.
    abundance_timing.py ties                 the tie accounting beside the counts (Engine.set_ties; csrc/k_ties.h), three legs alternating inside
                                             the repetition loop on both libraries of `kernel`: counts alone, counts + ties, counts + coverage +
                                             ties - abundance_ms() and ties_ms() of each, against ms_total of the same ranges; then the wall
                                             time of file -> counts (+ ties()) with the switch off and on, as `files` measures it
    abundance_timing.py curve                the rarefaction curve beside the counts and the coverage (Engine.set_curve; csrc/k_curve.h), three legs
                                             alternating inside the repetition loop on both libraries of `kernel`: counts + coverage, the same with
                                             a curve of 10 points, with one of 64 - abundance_ms() of each (the counting kernel with its marks),
                                             k_curve's time over the ranges (curve_ms() before the read) and k_curve_scan's per read of the figures
                                             (what one curve() adds to it), against ms_total of the same ranges; then the wall time of file ->
                                             counts + coverage (the sampler beside the search) against file -> curve of 10 points (the sampler
                                             first, then one search: abundance.py's path with the switch)
    abundance_timing.py bench --root TREE    `bench.py --gpus 1 --steps 5 --warmup 1` of this tree and of TREE (the parent commit's, built) in turn,
                                             --reps times (3 is enough: a run is five steps), one child process each: ms per step of every run"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


TAG = {}                 # {"tree": --tag}: added to every line printed


def emit(d):
    print(json.dumps(dict(d, **TAG)), flush=True)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v)}


def numpy_counts(rows, nseq):
    """the statement without cut-offs on an mc_row array: the first row of the highest bit score per read"""
    import numpy as np
    if len(rows) == 0:
        return np.zeros(nseq, np.int64)
    q = rows["query"]
    first = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
    top = np.maximum.reduceat(rows["bits"], first)
    seg = np.repeat(np.arange(len(first)), np.diff(np.r_[first, len(rows)]))
    is_top = rows["bits"] == top[seg]
    pos = np.flatnonzero(is_top)
    keep = pos[np.r_[True, seg[pos][1:] != seg[pos][:-1]]]
    return np.bincount(rows["subject"][keep], minlength=nseq).astype(np.int64)


def ties_legs(a, eng, reads, _native, synth):
    L, n = 150, len(reads)
    names, seqs = _native.load_markers()
    dense = synth.sample_reads(synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0), a.dense_reads, L, seed=405)
    legs = (("counts", False, False), ("counts_ties", False, True), ("counts_coverage_ties", True, True))
    for label, rd, piece in (("bench reads, marker database", reads, n), ("marker-dense library, ranges of 5,000", dense, 5000)):
        eng.upload(rd)
        eng.set_abundance(True)
        ms = {leg[0]: {"abundance": [], "ties": [], "total": []} for leg in legs}
        rows, t = 0, None
        for rep in range(a.reps + 1):
            for name, marks, ties in legs:
                eng.set_coverage(marks)
                eng.set_ties(ties)
                eng.abundance_reset()
                tot, rows = 0.0, 0
                for lo in range(0, len(rd), piece):
                    eng.run_range(lo, min(piece, len(rd) - lo), lo)
                    st = eng.stats()
                    tot += st["ms_total"]; rows += st["rows"]
                    assert st["range_splits"] == 0
                ms[name]["abundance"].append(eng.abundance_ms() * 1e6 / len(rd)); ms[name]["total"].append(tot * 1e6 / len(rd))
                ms[name]["ties"].append(eng.ties_ms() * 1e6 / len(rd) if ties else 0.0)
                if ties:
                    t = eng.ties()
        got = eng.abundance()
        eng.set_abundance(False)
        out = {"what": "ties", "library": label, "reads": len(rd), "rows_per_read": round(rows / len(rd), 2), "assigned": got["assigned"], "ambiguous": t["ambiguous"],
               "candidates": int(t["candidates"].sum())}
        for name in ms:
            out[name] = {"abundance_ms_per_1M_reads": spread(ms[name]["abundance"][1:]), "ties_ms_per_1M_reads": spread(ms[name]["ties"][1:]),
                         "range_ms_total_per_1M_reads": spread(ms[name]["total"][1:])}
        emit(out)
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fa")
        with open(fa, "wb") as f:
            for s in range(0, n, 50000):
                f.write(b"".join(b">r%d\n%s\n" % (s + i, bytes(r)) for i, r in enumerate(reads[s:s + 50000])))
        wall = {"counts": [], "counts_ties": []}
        for rep in range(a.reps + 1):
            for name, ties in (("counts_ties", True), ("counts", False)):
                rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
                try:
                    eng.set_abundance(True)
                    eng.set_ties(ties)
                    t0 = time.perf_counter()
                    eng.search_files(rd, keep_rows=False)
                    eng.abundance()
                    if ties:
                        eng.ties()
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                finally:
                    rd.close()
        emit({"what": "ties files", "reads": n, "counts_wall_ms": spread(wall["counts"][1:]), "counts_ties_wall_ms": spread(wall["counts_ties"][1:])})


def curve_legs(a, eng, reads, _native, synth):
    from microbecensus_amd import microbe_census
    L, n = 150, len(reads)
    names, seqs = _native.load_markers()
    dense = synth.sample_reads(synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0), a.dense_reads, L, seed=405)
    legs = (("counts_coverage", 0), ("curve_10", 10), ("curve_64", 64))
    for label, rd, piece in (("bench reads, marker database", reads, n), ("marker-dense library, ranges of 5,000", dense, 5000)):
        eng.upload(rd)
        eng.set_abundance(True)
        eng.set_coverage(True)
        ms = {leg[0]: {"abundance": [], "curve": [], "scan": [], "total": []} for leg in legs}
        rows, cu = 0, None
        for rep in range(a.reps + 1):
            for name, K in legs:
                eng.set_curve(microbe_census.curve_points(len(rd), K) if K else None)      # (zeroes every counter, as abundance_reset does)
                eng.abundance_reset()
                tot, rows = 0.0, 0
                for lo in range(0, len(rd), piece):
                    eng.run_range(lo, min(piece, len(rd) - lo), lo)
                    st = eng.stats()
                    tot += st["ms_total"]; rows += st["rows"]
                    assert st["range_splits"] == 0
                ms[name]["abundance"].append(eng.abundance_ms() * 1e6 / len(rd)); ms[name]["total"].append(tot * 1e6 / len(rd))
                walk = eng.curve_ms() if K else 0.0
                if K:
                    cu = eng.curve()
                    assert cu["beyond"] == 0
                ms[name]["curve"].append(walk * 1e6 / len(rd)); ms[name]["scan"].append(eng.curve_ms() - walk if K else 0.0)
        got, cov = eng.abundance(), eng.coverage()
        assert (cu["reads"][-1] == got["reads"]).all() and (cu["covered"][-1] == cov["covered"]).all()
        eng.set_abundance(False)
        out = {"what": "curve", "library": label, "reads": len(rd), "rows_per_read": round(rows / len(rd), 2), "assigned": got["assigned"], "genes": len(eng.names),
               "genes_covered": int((cov["covered"] > 0).sum())}
        for name in ms:
            out[name] = {"abundance_ms_per_1M_reads": spread(ms[name]["abundance"][1:]), "k_curve_ms_per_1M_reads": spread(ms[name]["curve"][1:]),
                         "k_curve_scan_ms_per_read_of_the_figures": spread(ms[name]["scan"][1:]), "range_ms_total_per_1M_reads": spread(ms[name]["total"][1:])}
        emit(out)
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fa")
        with open(fa, "wb") as f:
            for s in range(0, n, 50000):
                f.write(b"".join(b">r%d\n%s\n" % (s + i, bytes(r)) for i, r in enumerate(reads[s:s + 50000])))
        wall = {"counts_coverage": [], "curve_10": []}
        for rep in range(a.reps + 1):
            for name, K in (("curve_10", 10), ("counts_coverage", 0)):
                rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
                try:
                    eng.set_abundance(True)
                    eng.set_coverage(True)
                    eng.set_curve(None)                              # (set_abundance(True) leaves the curve as the leg before set it)
                    t0 = time.perf_counter()
                    if K:
                        got = rd.run()
                        eng.set_curve(microbe_census.curve_points(got, K))
                        eng.lib.mc_set_keep_rows(eng.h, 0)
                        eng.search(rd.reads(got))
                        eng.lib.mc_set_keep_rows(eng.h, 1)
                        eng.curve()
                    else:
                        eng.search_files(rd, keep_rows=False)
                    eng.abundance()
                    eng.coverage()
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                finally:
                    rd.close()
        emit({"what": "curve files", "reads": n, "counts_coverage_wall_ms": spread(wall["counts_coverage"][1:]), "curve_10_wall_ms": spread(wall["curve_10"][1:])})


def bench_turns(a):
    import subprocess
    mine, ms = os.path.dirname(HERE), {"this_tree": [], "root": []}
    for rep in range(a.reps):
        for name, where in (("this_tree", mine), ("root", os.path.abspath(a.root))):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"], cwd=where, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit("bench.py in %s ended with status %d" % (where, p.returncode))      # (nothing more is started behind a run that failed)
            ms[name].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
    emit({"what": "bench", "command": "bench.py --gpus 1 --steps 5 --warmup 1", "root": a.root, "turns": a.reps, "this_tree_ms_per_step": ms["this_tree"], "root_ms_per_step": ms["root"],
          "this_tree_median": statistics.median(ms["this_tree"]), "root_max": max(ms["root"])})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("kernel", "files", "host", "ties", "curve", "bench"))
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--dense-reads", type=int, default=100000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--coverage", action="store_true")
    p.add_argument("--tag", default=None, help="whose code runs: every line printed carries it as \"tree\"")
    a = p.parse_args()
    if a.tag:
        TAG["tree"] = a.tag
    if a.what == "bench":
        return bench_turns(a)
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    from microbecensus_amd import _native, synth
    L, n = 150, a.reads
    model = _native.load_model()
    eng = _native.Engine(device=0)
    eng.set_run(L, model["pars"][str(L)], model["families"])
    has_switch = hasattr(eng, "set_abundance")
    cov = a.coverage and hasattr(eng, "set_coverage")
    reads = synth.GenomeReads(device="cpu", seed=20261001).single(n, L).numpy()
    if a.what == "ties":
        ties_legs(a, eng, reads, _native, synth)
    elif a.what == "curve":
        curve_legs(a, eng, reads, _native, synth)
    elif a.what == "kernel":
        names, seqs = _native.load_markers()
        dense = synth.sample_reads(synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0), a.dense_reads, L, seed=405)
        for label, rd, piece in (("bench reads, marker database", reads, n), ("marker-dense library, ranges of 5,000", dense, 5000)):
            eng.upload(rd)
            eng.set_abundance(True)
            ab, tot, rows = [], [], 0
            ab_cov, tot_cov, scan, figures = [], [], [], None
            for rep in range(a.reps + 1):
                for marks in ((False, True) if cov else (False,)):
                    if cov:
                        eng.set_coverage(marks)
                    eng.abundance_reset()
                    t, rows = 0.0, 0
                    for lo in range(0, len(rd), piece):
                        eng.run_range(lo, min(piece, len(rd) - lo), lo)
                        st = eng.stats()
                        t += st["ms_total"]; rows += st["rows"]
                        assert st["range_splits"] == 0
                    (ab_cov if marks else ab).append(eng.abundance_ms() * 1e6 / len(rd)); (tot_cov if marks else tot).append(t * 1e6 / len(rd))
                    if marks:
                        figures = eng.coverage()
                        scan.append(eng.coverage_ms())
            got = eng.abundance()
            eng.set_abundance(False)
            out = {"what": "kernel", "library": label, "reads": len(rd), "rows_per_read": round(rows / len(rd), 2), "assigned": got["assigned"],
                   "abundance_ms_per_1M_reads": spread(ab[1:]), "range_ms_total_per_1M_reads": spread(tot[1:]),
                   "share": round(statistics.median(ab[1:]) / statistics.median(tot[1:]), 5)}
            if cov:
                out.update({"coverage": True, "abundance_ms_per_1M_reads_with_marks": spread(ab_cov[1:]), "range_ms_total_per_1M_reads_with_marks": spread(tot_cov[1:]),
                            "coverage_ms_per_read_of_the_figures": spread(scan[1:]), "genes": len(eng.names), "genes_covered": int((figures["covered"] > 0).sum()),
                            "max_depth": int(figures["max_depth"].max())})
            emit(out)
    else:
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "reads.fa")
            with open(fa, "wb") as f:
                for s in range(0, n, 50000):
                    f.write(b"".join(b">r%d\n%s\n" % (s + i, bytes(r)) for i, r in enumerate(reads[s:s + 50000])))

            def run(on, keep_rows, marks=False):
                rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
                try:
                    if has_switch:
                        eng.set_abundance(on)
                    if cov and on:
                        eng.set_coverage(marks)                      # (explicitly on both sides: set_abundance(True) leaves coverage as it was)
                    t0 = time.perf_counter()
                    rows, _ = eng.search_files(rd, keep_rows=keep_rows)
                    if on:
                        counts = eng.abundance()["reads"]
                        if marks:
                            eng.coverage()
                    elif keep_rows:
                        counts = numpy_counts(rows, len(eng.names))
                    else:
                        counts = None
                    return 1e3 * (time.perf_counter() - t0), counts
                finally:
                    rd.close()
            if a.what == "files":
                on, off, on_cov = [], [], []
                for rep in range(a.reps + 1):
                    if cov:
                        on_cov.append(run(True, False, True)[0])
                    if has_switch:
                        on.append(run(True, False)[0])
                    off.append(run(False, False)[0])
                out = {"what": "files", "root": a.root, "has_switch": has_switch, "reads": n, "off_wall_ms": spread(off[1:])}
                if has_switch:
                    out["on_wall_ms"] = spread(on[1:])
                if cov:
                    out["on_with_coverage_wall_ms"] = spread(on_cov[1:])
                emit(out)
            else:
                dev, host = [], []
                for rep in range(a.reps + 1):
                    t1, c1 = run(True, False)
                    t2, c2 = run(False, True)
                    assert np.array_equal(c1, c2)
                    dev.append(t1); host.append(t2)
                emit({"what": "host", "reads": n, "device_counts_wall_ms": spread(dev[1:]), "rows_to_host_and_numpy_wall_ms": spread(host[1:])})
    if has_switch:
        eng.set_abundance(False)
    eng.close()


if __name__ == "__main__":
    main()
