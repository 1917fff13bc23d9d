#!/usr/bin/env python3
"""The measurements of DESIGN.md 13.12 (GPU box), one process per mode, warm-up first, median with min - max.  One JSON line per figure.
The reads: 1 M reads of 150 bp of bench.py's read recipe (the 30 genomes) against the marker database - the README's abundance leg.

    identity_timing.py files [--root TREE] [--identity]
                                 wall time of file -> counts: search_files(keep_rows=False) + abundance() on a FASTA of the reads.  Without
                                 --identity the switch is OFF: --root names the tree whose package and built library are measured - this tree
                                 and the parent commit's in turn, process after process (a library alone is swapped through MCENSUS_LIB where
                                 it exports what the package binds).  With --identity the switch is on and identity() at 8 levels is part of
                                 the wall time.
    identity_timing.py kernel    the switch ON: k_identity over the ranges (identity_ms()) beside the counting kernel (abundance_ms()) and
                                 ms_total of the same ranges, on the bench reads in one range and on the marker-dense library in ranges of
                                 5,000; then one identity() - the scan - at 0 and at 8 levels (identity_scan_ms() and the wall time), and
                                 identity_hist(), the copy of the histogram (wall time, bytes)
--reads (1,000,000), --dense-reads (100,000), --reps (3)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TAG = {}
LEVELS8 = [50, 60, 70, 80, 90, 95, 99, 100]


def emit(d):
    print(json.dumps(dict(d, **TAG)), flush=True)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v)}


def files(a, eng, reads, _native):
    L, n = 150, len(reads)
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fa")
        with open(fa, "wb") as f:
            for s in range(0, n, 50000):
                f.write(b"".join(b">r%d\n%s\n" % (s + i, bytes(r)) for i, r in enumerate(reads[s:s + 50000])))
        wall, idn = [], None
        for rep in range(a.reps + 1):
            rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
            try:
                eng.set_abundance(True)
                if a.identity:
                    eng.set_identity(True)
                t0 = time.perf_counter()
                eng.search_files(rd, keep_rows=False)
                got = eng.abundance()
                if a.identity:
                    idn = eng.identity(LEVELS8)
                wall.append(1e3 * (time.perf_counter() - t0))
            finally:
                rd.close()
        emit({"what": "files", "root": os.path.relpath(a.root), "lib": os.environ.get("MCENSUS_LIB"), "has_switch": hasattr(eng, "set_identity"), "identity": bool(a.identity), "reads": n,
              "assigned": got["assigned"], "matched": None if idn is None else int(idn["matched"].sum()), "wall_ms": spread(wall[1:]), "wall_ms_all": [round(w, 2) for w in wall[1:]]})


def kernel(a, eng, reads, seqs, synth):
    L = 150
    dense = synth.sample_reads(synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0), a.dense_reads, L, seed=405)
    for label, rd, piece in (("bench reads, marker database", reads, len(reads)), ("marker-dense library, ranges of 5,000", dense, 5000)):
        n = len(rd)
        eng.upload(rd)
        eng.set_abundance(True)
        eng.set_identity(True)
        ms = {k: [] for k in ("count", "identity", "total")}
        for rep in range(a.reps + 1):
            eng.abundance_reset()
            total, rows = 0.0, 0
            for lo in range(0, n, piece):
                eng.run_range(lo, min(piece, n - lo), lo)
                st = eng.stats()
                assert st["range_splits"] == 0
                total += st["ms_total"]; rows += st["rows"]
            ms["count"].append(eng.abundance_ms() * 1e6 / n); ms["identity"].append(eng.identity_ms() * 1e6 / n); ms["total"].append(total * 1e6 / n)
        got = eng.abundance()
        emit({"what": "kernel", "reads_of": label, "reads": n, "rows": rows, "assigned": got["assigned"], "genes_with_reads": int((got["reads"] > 0).sum()), "largest_gene": int(got["reads"].max()),
              "k_abundance_ms_per_1M_reads": spread(ms["count"][1:]), "k_identity_ms_per_1M_reads": spread(ms["identity"][1:]), "range_ms_total_per_1M_reads": spread(ms["total"][1:])})
        if piece != n:
            continue
        for levels in ([], LEVELS8):
            t = {"scan": [], "wall": []}
            for rep in range(a.reps + 1):
                before = eng.identity_scan_ms()
                t0 = time.perf_counter()
                eng.identity(levels)
                t["wall"].append(1e3 * (time.perf_counter() - t0))
                t["scan"].append(eng.identity_scan_ms() - before)
            emit({"what": "read", "levels": len(levels), "genes": len(eng.names), "k_identity_scan_ms": spread(t["scan"][1:]), "identity_wall_ms": spread(t["wall"][1:])})
        wall = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            h = eng.identity_hist()
            wall.append(1e3 * (time.perf_counter() - t0))
        emit({"what": "hist", "genes": len(eng.names), "host_bytes": int(h.nbytes), "device_bytes": 512 * len(eng.names), "reads_in_it": int(h.sum()), "identity_hist_wall_ms": spread(wall[1:])})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("files", "kernel"))
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--identity", action="store_true")
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--dense-reads", type=int, default=100000)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--tag", default=None, help="whose code runs: every line printed carries it as \"tree\"")
    a = p.parse_args()
    if a.tag:
        TAG["tree"] = a.tag
    sys.path.insert(0, os.path.abspath(a.root))
    from microbecensus_amd import _native, synth
    L = 150
    model = _native.load_model()
    seqs = _native.load_markers()[1]
    eng = _native.Engine(device=0)
    eng.set_run(L, model["pars"][str(L)], model["families"])
    reads = synth.GenomeReads(device="cpu", seed=20261001).single(a.reads, L).numpy()
    try:
        if a.what == "files":
            files(a, eng, reads, _native)
        else:
            kernel(a, eng, reads, seqs, synth)
        eng.set_abundance(False)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
