#!/usr/bin/env python3
"""The measurements of DESIGN.md 13.10 (GPU box), one process per mode, warm-up first, the two sides of a comparison alternating inside the
repetition loop where one process holds both, median with min - max.  One JSON line per figure.  The reads: 1 M reads of 150 bp of
bench.py's read recipe (the 30 genomes) against the marker database - the README's abundance leg.

    tieboot_timing.py files [--root TREE]   the switch OFF: wall time of file -> counts, search_files(keep_rows=False) + abundance() + ties() on a
                                            FASTA of the reads with --ties and --bootstrap on (a gene list of as many entries as reads);
                                            --root: the tree whose package and built library are measured - this tree and the parent
                                            commit's in turn, process after process
    tieboot_timing.py kernel                the switch ON: k_tieboot_collect over the ranges (tie_bootstrap_kernels_ms()["collect"]) beside
                                            ties_ms(), gene_bootstrap_ms() and ms_total of the same ranges; the list's entries and bytes; then
                                            mc_tie_bootstrap at B = 100, 1000 and 4096: its three kernels (HIP events) and the wall time of
                                            Engine.tie_bootstrap(), beside mc_gene_bootstrap's on the same run
    tieboot_timing.py host                  the same figures without the feature: a keep_rows search, and the restatement's entries and
                                            replicate shares from the host rows in numpy (tests/tieboot_restated.py) at B = 100
--reads (1,000,000), --reps (3)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TAG = {}


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
        wall = []
        for rep in range(a.reps + 1):
            rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
            try:
                eng.set_abundance(True)
                eng.set_ties(True)
                eng.set_gene_bootstrap(n)
                t0 = time.perf_counter()
                eng.search_files(rd, keep_rows=False)
                got, ti = eng.abundance(), eng.ties()
                wall.append(1e3 * (time.perf_counter() - t0))
            finally:
                rd.close()
        emit({"what": "files", "root": a.root, "has_switch": hasattr(eng, "set_tie_bootstrap"), "reads": n, "assigned": got["assigned"], "ambiguous": ti["ambiguous"],
              "wall_ms": spread(wall[1:])})


def kernel(a, eng, reads):
    import numpy as np
    n = len(reads)
    eng.upload(reads)
    eng.set_abundance(True)
    eng.set_ties(True)
    ms = {k: [] for k in ("ties", "gene_collect", "tie_collect", "total")}
    for rep in range(a.reps + 1):
        eng.set_gene_bootstrap(n)
        eng.set_tie_bootstrap(4 * n)
        eng.run_range(0, n, 0)
        st = eng.stats()
        assert st["range_splits"] == 0
        ms["ties"].append(eng.ties_ms() * 1e6 / n); ms["gene_collect"].append(eng.gene_bootstrap_ms() * 1e6 / n)
        ms["tie_collect"].append(eng.tie_bootstrap_kernels_ms()["collect"] * 1e6 / n); ms["total"].append(st["ms_total"] * 1e6 / n)
    got, ti = eng.abundance(), eng.ties()
    entries = int(ti["candidates"].sum())
    emit({"what": "kernel", "reads": n, "rows": st["rows"], "assigned": got["assigned"], "ambiguous": ti["ambiguous"], "entries": entries, "list_bytes": 12 * entries,
          "genes_with_candidates": int((ti["candidates"] > 0).sum()), "k_ties_ms_per_1M_reads": spread(ms["ties"][1:]), "k_geneboot_collect_ms_per_1M_reads": spread(ms["gene_collect"][1:]),
          "k_tieboot_collect_ms_per_1M_reads": spread(ms["tie_collect"][1:]), "range_ms_total_per_1M_reads": spread(ms["total"][1:])})
    for B in (100, 1000, 4096):
        scale = np.full(B, 1e-3)
        t = {k: [] for k in ("tie_kernels", "tie_wall", "gene_kernels", "gene_wall")}
        for rep in range(a.reps + 1):
            before = eng.tie_bootstrap_kernels_ms()["read"]
            t0 = time.perf_counter()
            eng.tie_bootstrap(B, 1, scale)
            t["tie_wall"].append(1e3 * (time.perf_counter() - t0))
            t["tie_kernels"].append(eng.tie_bootstrap_kernels_ms()["read"] - before)
            before = eng.gene_bootstrap_ms()
            t0 = time.perf_counter()
            eng.gene_bootstrap(B, 1, scale)
            t["gene_wall"].append(1e3 * (time.perf_counter() - t0))
            t["gene_kernels"].append(eng.gene_bootstrap_ms() - before)
        emit(dict({"what": "read", "B": B, "entries": entries, "gene_entries": got["assigned"]}, **{k + "_ms": spread(v[1:]) for k, v in t.items()}))


def host(a, eng, reads):
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import coverage_restated as V
    import tieboot_restated as TR
    n, B = len(reads), 100
    t = {k: [] for k in ("search_keep_rows", "entries", "shares")}
    for rep in range(a.reps):
        eng.set_abundance(True)
        t0 = time.perf_counter()
        rows, _ = eng.search(reads)
        rows = rows.copy()
        t["search_keep_rows"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        q, s, sh, ks = TR.entries(V.rows_from_array(rows), len(eng.names))
        t["entries"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        cs = TR.shares(q, s, sh, len(eng.names), B, 1)
        t["shares"].append(1e3 * (time.perf_counter() - t0))
    emit(dict({"what": "host", "reads": n, "rows": int(len(rows)), "row_bytes": int(rows.nbytes), "entries": int(len(q)), "B": B, "checksum": int(cs.sum() % (1 << 61))},
              **{k + "_wall_ms": spread(v) for k, v in t.items()}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("files", "kernel", "host"))
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--tag", default=None, help="whose code runs: every line printed carries it as \"tree\"")
    a = p.parse_args()
    if a.tag:
        TAG["tree"] = a.tag
    sys.path.insert(0, os.path.abspath(a.root))
    from microbecensus_amd import _native, synth
    L = 150
    model = _native.load_model()
    eng = _native.Engine(device=0)
    eng.set_run(L, model["pars"][str(L)], model["families"])
    reads = synth.GenomeReads(device="cpu", seed=20261001).single(a.reads, L).numpy()
    try:
        if a.what == "files":
            files(a, eng, reads, _native)
        elif a.what == "host":
            host(a, eng, reads)
        else:
            kernel(a, eng, reads)
        eng.set_abundance(False)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
