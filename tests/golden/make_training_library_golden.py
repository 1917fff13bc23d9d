#!/usr/bin/env python3
"""Golden vectors of whole training library passes: the .hits table the REFERENCE's own classify_reads (training/training.py:311-334)
makes of the oracle's m8 of a simulated library, one file per case (tests/golden/training_library_<case>.json.gz).

For each case:
  1. the library's reads are made on the CPU by tests/simlib_restated.simulate (the numpy restatement the GPU tests pin k_sim_copy /
     k_sim_walk to, byte for byte), from one genome of tests/golden/genomes/genomes30.npz, with the (seed, library id, kind)
     recorded in the golden;
  2. the reads, named by their index (">%d", mates included, as Engine.write_m8 names them), are searched by oracle/rs_port on
     oracle/_ref/rapdb_2.15: one slice per core (at most 16 processes), the outputs joined in read order; the md5 of that m8 is
     recorded;
  3. training.py:210-219 (parse_rapsearch), :229-334 (read_hits .. classify_reads) and :336-343 (drange) are read from the
     reference and exec'd UNCHANGED, as make_training_golden.py does it, and classify_reads runs on that m8 with the grid of
     training/class_reads.py:51-53, the reference's gene_fam.map / gene_len.map and the read length as class_reads.py passes it
     (a string).

Output: tests/golden/training_library_<case>.json.gz, the rows of the .hits table with count_hits > 0 as [fam, aln_cov, max_pid,
min_score, count_hits, count_aln, count_cov] (the format of training_grid_unittest.json.gz), the library's parameters, the m8's md5
and row count; and tests/golden/training_library_<case>.m8.gz, the m8 itself, so that the CPU test of tests/grid_restated.py needs
neither the reference nor the oracle's database.  The files are written with a fixed gzip header, so running this twice gives the
same bytes.  Needs /root/reference and the built oracle
(__graft_entry__.build()).
    python tests/golden/make_training_library_golden.py"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PORT, RAPDB = os.path.join(REPO, "oracle", "rs_port"), os.path.join(REPO, "oracle", "_ref", "rapdb_2.15")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
import simlib_restated as sr  # noqa: E402
from microbecensus_amd import training  # noqa: E402

# case: (genome index in genomes30.npz, read length, reads, seed, library kind)
CASES = {
    "a": (1, 150, 16000, 101, dict(error_model="illumina", paired_end=True, insert=300)),     # L mod 3 = 0
    "b": (2, 100, 30000, 102, dict(error_model="uniform", error_rate=0.03)),                 # L mod 3 = 1
    "c": (5, 500, 6000, 103, dict()),                                                         # L mod 3 = 2, error-free
}


class Py2Dict(dict):
    def iteritems(self):
        return iter(self.items())


def load_genome(k):
    """(name, bases, contig_off) of genome k of genomes30.npz, named as the GPU tests name it ("g%02d")."""
    d = np.load(os.path.join(HERE, "genomes", "genomes30.npz"))
    packed, off = d["packed"], d["contig_off"]
    idx = np.nonzero(d["genome_of"] == k)[0]
    lo, hi = int(off[idx[0]]), int(off[idx[-1] + 1])
    codes = np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=1).reshape(-1)[: off[-1]]
    allb = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    allb[d["exc_pos"]] = d["exc_chr"]
    return "g%02d" % k, allb[lo:hi].copy(), (off[idx[0]: idx[-1] + 2] - lo).astype(np.int64)


def oracle_m8(reads, td, tag, rapdb=RAPDB):
    """The oracle's m8 of the reads (headers = read indices) on a database: one slice per core, at most 16 processes, joined in
    order."""
    n, k = len(reads), max(1, min(16, len(os.sched_getaffinity(0))))
    cuts = [n * i // k for i in range(k + 1)]
    procs = []
    for i in range(k):
        fa = os.path.join(td, "%s_%d.fa" % (tag, i))
        with open(fa, "w") as f:
            f.write("".join(">%d\n%s\n" % (j, bytes(reads[j]).decode()) for j in range(cuts[i], cuts[i + 1])))
        procs.append(subprocess.Popen([PORT, rapdb, fa, os.path.join(td, "%s_%d.m8" % (tag, i))]))
    out = b""
    for i, p in enumerate(procs):
        assert p.wait() == 0
        out += open(os.path.join(td, "%s_%d.m8" % (tag, i)), "rb").read()
    return out


def write_gz(path, data):
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
        f.write(data)


def reference_grid():
    src = open(os.path.join(REF, "training", "training.py")).read().split("\n")
    text = "\n".join(src[209:219] + [""] + src[228:334] + [""] + src[335:343]) + "\n"
    ns = {}
    exec(compile(text, "training.py[210-219,229-334,336-343]", "exec"), ns)
    ref_aggregate = ns["aggregate_hits"]
    ns["aggregate_hits"] = lambda *a, **k: Py2Dict(ref_aggregate(*a, **k))
    return ns


def main():
    assert os.path.exists(PORT) and os.path.exists(RAPDB), "oracle not built: run __graft_entry__.build() first"
    ns = reference_grid()
    data = os.path.join(REF, "microbe_census", "data")
    gene2fam = dict(line.split() for line in open(os.path.join(data, "gene_fam.map")))
    gene2len = {k: int(v) for k, v in (line.split() for line in open(os.path.join(data, "gene_len.map")))}
    fams = set(gene2fam.values())
    aln_covs, max_pids, min_scores = [0.00, 0.25, 0.50, 0.75], [50, 60, 70, 80, 90, 100], ns["drange"](23, 50, 1)
    for case, (gk, L, n, seed, kind) in sorted(CASES.items()):
        name, bases, off = load_genome(gk)
        lid = training.library_id(name, L)
        reads = sr.simulate(bases, off, L, 0, n, seed, lid, **kind)
        with tempfile.TemporaryDirectory() as td:
            m8_bytes = oracle_m8(reads, td, case)
            m8 = os.path.join(td, case + ".m8")
            with open(m8, "wb") as f:
                f.write(m8_bytes)
            out = os.path.join(td, case + ".hits")
            ns["classify_reads"](m8, out, aln_covs, max_pids, min_scores, gene2len, gene2fam, fams, str(L))
            rows = []
            with open(out) as f:
                assert f.readline().split() == ["fam", "aln_cov", "max_pid", "min_score", "count_hits", "count_aln", "count_cov"]
                for line in f:
                    x = line.split()
                    if int(x[4]) > 0:
                        rows.append([x[0], float(x[1]), int(x[2]), float(x[3]), int(x[4]), int(x[5]), float(x[6])])
        rows.sort()
        doc = {"source": "training/training.py:311-334 classify_reads on oracle/rs_port's m8 of a simulated library, read_length '%d'" % L,
               "library": {"genome": name, "genome_index": gk, "read_len": L, "nreads": n, "seed": seed, "library_id": lid, "kind": kind},
               "m8_md5": hashlib.md5(m8_bytes).hexdigest(), "m8_rows": m8_bytes.count(b"\n"),
               "aln_covs": aln_covs, "max_pids": max_pids, "min_scores": [float(v) for v in min_scores], "n_rows_with_hits": len(rows), "rows": rows}
        path = os.path.join(HERE, "training_library_%s.json.gz" % case)
        write_gz(path, json.dumps(doc).encode())
        write_gz(os.path.join(HERE, "training_library_%s.m8.gz" % case), m8_bytes)
        print("case %s: %s L=%d %d reads %s: %d m8 rows, %d table rows with hits, %d hits at the loosest cell, %d bytes"
              % (case, name, L, n, kind, doc["m8_rows"], len(rows), sum(r[4] for r in rows if r[1:4] == [0.0, 100, 23.0]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
