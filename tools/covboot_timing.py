#!/usr/bin/env python3
"""The measurements of DESIGN.md 13.11 (GPU box), one process per mode, warm-up first, median with min - max.  One JSON line per figure.
The reads: 1 M reads of 150 bp of bench.py's read recipe (the 30 genomes) against the marker database - the README's abundance leg.

    covboot_timing.py files [--root TREE]   the switch OFF: wall time of file -> counts, search_files(keep_rows=False) + abundance() + coverage()
                                            on a FASTA of the reads with --coverage and --bootstrap on (a gene list of as many entries as
                                            reads); --root: the tree whose package and built library are measured - this tree and the parent
                                            commit's in turn, process after process
    covboot_timing.py kernel                the switch ON: k_covboot_collect over the ranges (coverage_bootstrap_kernels_ms()["collect"]) beside
                                            abundance_ms() (the counting kernel with the marks) and ms_total of the same ranges; the list's
                                            entries and bytes; then mc_coverage_bootstrap at B = 100, 1000 and 4096: its three kernels (HIP
                                            events) and the wall time of Engine.coverage_bootstrap(), beside mc_gene_bootstrap's on the same run
    covboot_timing.py onegene               the serial worst case: every read cut from the back-translation of ONE marker (the longest), so
                                            that one gene holds nearly every entry; the same reads' figures at B = 100, 1000 and 4096
    covboot_timing.py host                  the same figures without the feature: a keep_rows search, and the restatement's entries and
                                            covered residues from the host rows in numpy (tests/covboot_restated.py) at B = 100
    covboot_timing.py prefix                detected_support at the first 100,000 reads against detected on all of them (--min-breadth 0.5)
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
CODON = dict(zip("ACDEFGHIKLMNPQRSTVWY", ("GCT", "TGT", "GAT", "GAA", "TTT", "GGT", "CAT", "ATT", "AAA", "CTG", "ATG", "AAT", "CCG", "CAG", "CGT", "AGC", "ACC", "GTG", "TGG", "TAT")))


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
                eng.set_coverage(True)
                eng.set_gene_bootstrap(n)
                t0 = time.perf_counter()
                eng.search_files(rd, keep_rows=False)
                got, cov = eng.abundance(), eng.coverage()
                wall.append(1e3 * (time.perf_counter() - t0))
            finally:
                rd.close()
        emit({"what": "files", "root": a.root, "has_switch": hasattr(eng, "set_coverage_bootstrap"), "reads": n, "assigned": got["assigned"], "covered": int(cov["covered"].sum()),
              "wall_ms": spread(wall[1:]), "wall_ms_all": [round(w, 2) for w in wall[1:]]})


def reads_of(a, eng, what, B_list, n_ranges):
    """mc_coverage_bootstrap beside mc_gene_bootstrap on the run as it stands"""
    import numpy as np
    got = eng.abundance()
    for B in B_list:
        scale = np.full(B, 1e-3)
        t = {k: [] for k in ("cov_kernels", "cov_wall", "gene_kernels", "gene_wall")}
        for rep in range(a.reps + 1):
            before = eng.coverage_bootstrap_kernels_ms()["read"]
            t0 = time.perf_counter()
            eng.coverage_bootstrap(B, 1)
            t["cov_wall"].append(1e3 * (time.perf_counter() - t0))
            t["cov_kernels"].append(eng.coverage_bootstrap_kernels_ms()["read"] - before)
            before = eng.gene_bootstrap_ms()
            t0 = time.perf_counter()
            eng.gene_bootstrap(B, 1, scale)
            t["gene_wall"].append(1e3 * (time.perf_counter() - t0))
            t["gene_kernels"].append(eng.gene_bootstrap_ms() - before)
        emit(dict({"what": what, "B": B, "entries": got["assigned"], "largest_gene": int(got["reads"].max())}, **{k + "_ms": spread(v[1:]) for k, v in t.items()}))


def kernel(a, eng, reads):
    n = len(reads)
    eng.upload(reads)
    eng.set_abundance(True)
    eng.set_coverage(True)
    ms = {k: [] for k in ("count", "gene_collect", "cov_collect", "total")}
    for rep in range(a.reps + 1):
        eng.set_gene_bootstrap(n)
        eng.set_coverage_bootstrap(n)
        eng.run_range(0, n, 0)
        st = eng.stats()
        assert st["range_splits"] == 0
        ms["count"].append(eng.abundance_ms() * 1e6 / n); ms["gene_collect"].append(eng.gene_bootstrap_ms() * 1e6 / n)
        ms["cov_collect"].append(eng.coverage_bootstrap_kernels_ms()["collect"] * 1e6 / n); ms["total"].append(st["ms_total"] * 1e6 / n)
    got = eng.abundance()
    emit({"what": "kernel", "reads": n, "rows": st["rows"], "assigned": got["assigned"], "list_bytes": 12 * got["assigned"], "genes_with_reads": int((got["reads"] > 0).sum()),
          "k_abundance_cov_ms_per_1M_reads": spread(ms["count"][1:]), "k_geneboot_collect_ms_per_1M_reads": spread(ms["gene_collect"][1:]),
          "k_covboot_collect_ms_per_1M_reads": spread(ms["cov_collect"][1:]), "range_ms_total_per_1M_reads": spread(ms["total"][1:])})
    reads_of(a, eng, "read", (100, 1000, 4096), 1)


def onegene(a, eng, seqs):
    import numpy as np
    g = max(range(len(seqs)), key=lambda k: len(seqs[k]) if set(seqs[k]) <= set(CODON) else 0)
    dna = np.frombuffer("".join(CODON[c] for c in seqs[g]).encode(), np.uint8)
    L, n = 150, a.reads
    at = np.random.default_rng(7).integers(0, len(dna) - L + 1, n)
    reads = dna[at[:, None] + np.arange(L)[None, :]]
    eng.set_abundance(True)
    eng.set_coverage(True)
    eng.set_gene_bootstrap(n)
    eng.set_coverage_bootstrap(n)
    t0 = time.perf_counter()
    eng.search(reads, keep_rows=False)
    wall = 1e3 * (time.perf_counter() - t0)
    got, cov = eng.abundance(), eng.coverage()
    emit({"what": "onegene_search", "gene": eng.names[g], "length_aa": len(seqs[g]), "reads": n, "assigned": got["assigned"], "reads_of_the_gene": int(got["reads"][g]),
          "covered_aa": int(cov["covered"][g]), "search_wall_ms": round(wall, 1), "k_covboot_collect_ms": round(eng.coverage_bootstrap_kernels_ms()["collect"], 4)})
    reads_of(a, eng, "onegene_read", (100, 1000, 4096), 1)


def host(a, eng, reads, seqs):
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import coverage_restated as V
    import covboot_restated as CR
    n, B = len(reads), 100
    lengths = np.array([len(s) for s in seqs], np.int64)
    t = {k: [] for k in ("search_keep_rows", "entries", "cover")}
    for rep in range(a.reps):
        eng.set_abundance(True)
        t0 = time.perf_counter()
        rows, _ = eng.search(reads)
        rows = rows.copy()
        t["search_keep_rows"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        q, g, s, e = CR.entries(V.rows_from_array(rows), lengths)
        t["entries"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        cov = CR.cover(q, g, s, e, lengths, B, 1)
        t["cover"].append(1e3 * (time.perf_counter() - t0))
    emit(dict({"what": "host", "reads": n, "rows": int(len(rows)), "row_bytes": int(rows.nbytes), "entries": int(len(q)), "B": B, "checksum": int(cov.sum() % (1 << 61))},
              **{k + "_wall_ms": spread(v) for k, v in t.items()}))


def prefix(a, eng, reads, seqs):
    import numpy as np
    from microbecensus_amd import abundance
    lengths = np.array([len(s) for s in seqs], np.int64)
    need = abundance.coverage_need(lengths, 0.5)
    out = {}
    for name, n in (("prefix", min(100000, len(reads))), ("full", len(reads))):
        eng.set_abundance(True)
        eng.set_coverage(True)
        eng.set_coverage_bootstrap(n)
        eng.search(reads[:n], keep_rows=False)
        cb, cov, ab = eng.coverage_bootstrap(1000, 1, need), eng.coverage(), eng.abundance()
        out[name] = {"det": (cov["covered"] >= need) & (ab["reads"] > 0), "support": cb["detected"] / 1000.0}
    det_p, sup, det_f = out["prefix"]["det"], out["prefix"]["support"], out["full"]["det"]
    bins = [(0.0, 0.5), (0.5, 0.9), (0.9, 0.99), (0.99, 1.0001)]
    emit({"what": "prefix", "prefix_reads": min(100000, len(reads)), "full_reads": len(reads), "detected_prefix": int(det_p.sum()), "detected_full": int(det_f.sum()),
          "detected_prefix_and_full": int((det_p & det_f).sum()),
          "by_support": [{"support": "[%g, %g)" % b, "detected_at_prefix": int((det_p & (sup >= b[0]) & (sup < b[1])).sum()),
                          "of_them_detected_at_full": int((det_p & det_f & (sup >= b[0]) & (sup < b[1])).sum())} for b in bins]})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("files", "kernel", "onegene", "host", "prefix"))
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
    seqs = _native.load_markers()[1]
    eng = _native.Engine(device=0)
    eng.set_run(L, model["pars"][str(L)], model["families"])
    reads = None if a.what == "onegene" else synth.GenomeReads(device="cpu", seed=20261001).single(a.reads, L).numpy()
    try:
        if a.what == "files":
            files(a, eng, reads, _native)
        elif a.what == "host":
            host(a, eng, reads, seqs)
        elif a.what == "onegene":
            onegene(a, eng, seqs)
        elif a.what == "prefix":
            prefix(a, eng, reads, seqs)
        else:
            kernel(a, eng, reads)
        eng.set_abundance(False)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
