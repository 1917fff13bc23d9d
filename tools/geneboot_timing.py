#!/usr/bin/env python3
"""The measurements of DESIGN.md 13.5 and 13.9 (GPU box), one process per mode, warm-up first, the two sides of a comparison alternating inside the
repetition loop, median with min - max.  One JSON line per figure.  The reads: 1 M reads of 150 bp of bench.py's read recipe (the 30
genomes) against the marker database - the README's abundance leg.

    geneboot_timing.py files [--root TREE]   wall time of file -> counts, search_files(keep_rows=False) + abundance() on a FASTA of the reads:
                                             with the gene bootstrap off and - where the tree has the switch - on (a list of as many entries
                                             as reads, k_geneboot_collect behind every range), alternating; --root: the tree whose package
                                             and built library are measured - the parent commit's has no switch and gives the off side alone
    geneboot_timing.py kernel                k_geneboot_collect over the ranges (gene_bootstrap_ms() before the first read) beside
                                             abundance_ms() and ms_total of the same ranges, the switch off and on alternating; then
                                             mc_gene_bootstrap at B = 100, 1000 and 4096: its three kernels (HIP events) and the wall
                                             time of Engine.gene_bootstrap(), with and without the counts matrix
    geneboot_timing.py groups                DESIGN.md 13.9: mc_group_bootstrap at B = 100, 1000 and 4096 on the same list, every gene mapped to its
                                             marker family and - the serial worst case - all genes in one group: the two kernels (HIP events),
                                             the call's kernels and wall time on its own (it makes the genes' replicate counts) and behind a
                                             gene_bootstrap() of the same B and seed (it takes them over); as a comparison the host route,
                                             gene_bootstrap(counts=True) and a numpy reduction of the matrix (--host-reps, 3)
    geneboot_timing.py groups-files [--root TREE]   wall time of file -> counts -> gene_bootstrap(B = 100): what a run with --bootstrap and --groups
                                             does on the device WITHOUT --bootstrap-groups; --root as for files: this tree and the parent's in turn
--reads (1,000,000), --reps (7)."""
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
    has = hasattr(eng, "set_gene_bootstrap")
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "reads.fa")
        with open(fa, "wb") as f:
            for s in range(0, n, 50000):
                f.write(b"".join(b">r%d\n%s\n" % (s + i, bytes(r)) for i, r in enumerate(reads[s:s + 50000])))
        wall = {"off": [], "on": []}
        for rep in range(a.reps + 1):
            for name in (("on", "off") if has else ("off",)):
                rd = _native.Reader([fa], L, 10 * n, False, 0, -5, -5, 100, False)
                try:
                    eng.set_abundance(True)
                    if has:
                        eng.set_gene_bootstrap(n if name == "on" else 0)
                    t0 = time.perf_counter()
                    eng.search_files(rd, keep_rows=False)
                    got = eng.abundance()
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                finally:
                    rd.close()
        out = {"what": "files", "root": a.root, "has_switch": has, "reads": n, "assigned": got["assigned"], "off_wall_ms": spread(wall["off"][1:])}
        if has:
            out["on_wall_ms"] = spread(wall["on"][1:])
        emit(out)


def kernel(a, eng, reads):
    import numpy as np
    n = len(reads)
    eng.upload(reads)
    eng.set_abundance(True)
    ms = {k: {"abundance": [], "collect": [], "total": []} for k in ("off", "on")}
    for rep in range(a.reps + 1):
        for name in ("on", "off"):
            eng.set_gene_bootstrap(n if name == "on" else 0)
            eng.abundance_reset()
            eng.run_range(0, n, 0)
            st = eng.stats()
            assert st["range_splits"] == 0
            ms[name]["abundance"].append(eng.abundance_ms() * 1e6 / n); ms[name]["total"].append(st["ms_total"] * 1e6 / n)
            ms[name]["collect"].append(eng.gene_bootstrap_ms() * 1e6 / n)
    got = eng.abundance()
    out = {"what": "kernel", "reads": n, "rows": st["rows"], "assigned": got["assigned"], "genes_with_reads": int((got["reads"] > 0).sum())}
    for name in ms:
        out[name] = {"abundance_ms_per_1M_reads": spread(ms[name]["abundance"][1:]), "k_geneboot_collect_ms_per_1M_reads": spread(ms[name]["collect"][1:]),
                     "range_ms_total_per_1M_reads": spread(ms[name]["total"][1:])}
    emit(out)
    eng.set_gene_bootstrap(n)
    eng.abundance_reset()
    eng.run_range(0, n, 0)
    for B in (100, 1000, 4096):
        scale = np.full(B, 1e-3)
        dev, wall, wall_counts = [], [], []
        for rep in range(a.reps + 1):
            before = eng.gene_bootstrap_ms()
            t0 = time.perf_counter()
            eng.gene_bootstrap(B, 1, scale)
            wall.append(1e3 * (time.perf_counter() - t0))
            dev.append(eng.gene_bootstrap_ms() - before)
            t0 = time.perf_counter()
            eng.gene_bootstrap(B, 1, scale, counts=True)
            wall_counts.append(1e3 * (time.perf_counter() - t0))
        emit({"what": "read", "B": B, "entries": got["assigned"], "genes_with_reads": int((got["reads"] > 0).sum()), "kernels_ms": spread(dev[1:]), "gene_bootstrap_wall_ms": spread(wall[1:]),
              "gene_bootstrap_with_counts_wall_ms": spread(wall_counts[1:])})


def groups(a, eng, reads, _native):
    import numpy as np
    names, seqs = _native.load_markers()
    n, nseq = len(reads), len(names)
    kb = 3.0 * np.array([len(s) for s in seqs], np.float64) / 1000.0
    index = {}
    family = np.array([index.setdefault(nm.split("_")[0], len(index)) for nm in names], np.int32)
    maps = {"family": (family, len(index)), "one_group": (np.zeros(nseq, np.int32), 1)}
    eng.upload(reads)
    eng.set_abundance(True)
    eng.set_gene_bootstrap(n)
    eng.run_range(0, n, 0)
    got = eng.abundance()
    have = got["reads"] > 0
    for B in (100, 1000, 4096):
        scale = np.full(B, 1e-3)
        for name, (ids, ngroups) in maps.items():
            t = {k: [] for k in ("values", "summary", "own_kernels", "own_wall", "behind_kernels", "behind_wall")}
            for r in range(a.reps + 1):
                k0, ms0 = eng.group_bootstrap_kernels_ms(), eng.group_bootstrap_ms()
                t0 = time.perf_counter()
                eng.group_bootstrap(B, 1000 + r, scale, ids, ngroups, kb)           # another seed every time: the replicate counts are made anew
                t["own_wall"].append(1e3 * (time.perf_counter() - t0))
                k1, ms1 = eng.group_bootstrap_kernels_ms(), eng.group_bootstrap_ms()
                t["values"].append(k1["values"] - k0["values"]); t["summary"].append(k1["summary"] - k0["summary"]); t["own_kernels"].append(ms1 - ms0)
                eng.gene_bootstrap(B, 1, scale)
                t0 = time.perf_counter()
                eng.group_bootstrap(B, 1, scale, ids, ngroups, kb)                  # behind a gene read of the same B and seed: taken over
                t["behind_wall"].append(1e3 * (time.perf_counter() - t0))
                t["behind_kernels"].append(eng.group_bootstrap_ms() - ms1)
            emit(dict({"what": "groups", "map": name, "B": B, "groups": ngroups, "groups_with_reads": len(set(ids[have].tolist())), "genes_with_reads": int(have.sum()),
                       "largest_group_members_with_reads": int(np.bincount(ids[have]).max()), "entries": got["assigned"]},
                      **{"k_groupboot_values_ms" if k == "values" else "k_groupboot_summary_ms" if k == "summary" else k + "_ms": spread(v[1:]) for k, v in t.items()}))
        ids, ngroups = maps["family"]
        host = []
        for r in range(a.host_reps + 1):
            t0 = time.perf_counter()
            cm = eng.gene_bootstrap(B, 1, scale, counts=True)["counts"]
            y = np.zeros((ngroups, B))
            np.add.at(y, ids[have], cm[have].astype(np.float64) * scale / kb[have, None])
            se, ci = y.std(axis=1, ddof=1), np.percentile(y, [2.5, 97.5], axis=1)
            host.append(1e3 * (time.perf_counter() - t0))
        emit({"what": "groups_host_route", "map": "family", "B": B, "groups": ngroups, "wall_ms": spread(host[1:]), "checksum": float(se.sum() + ci.sum())})


def groups_files(a, eng, reads, _native):
    import numpy as np
    L, n, B = 150, len(reads), 100
    scale = np.full(B, 1e-3)
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
                eng.set_gene_bootstrap(n)
                t0 = time.perf_counter()
                eng.search_files(rd, keep_rows=False)
                got = eng.abundance()
                eng.gene_bootstrap(B, 1, scale)
                wall.append(1e3 * (time.perf_counter() - t0))
            finally:
                rd.close()
        emit({"what": "groups-files", "root": a.root, "has_group_bootstrap": hasattr(eng, "group_bootstrap"), "reads": n, "assigned": got["assigned"], "B": B, "wall_ms": spread(wall[1:])})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("files", "kernel", "groups", "groups-files"))
    p.add_argument("--host-reps", type=int, default=3)
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--reads", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=7)
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
        elif a.what == "groups":
            groups(a, eng, reads, _native)
        elif a.what == "groups-files":
            groups_files(a, eng, reads, _native)
        else:
            kernel(a, eng, reads)
        eng.set_abundance(False)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
