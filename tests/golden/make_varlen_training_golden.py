#!/usr/bin/env python3
"""Golden vectors of training library passes in the simulator's reference read-length mode (reads of seq_sim.py's lengths,
L + insertions - deletions): the .hits table the REFERENCE's own classify_reads makes of the oracle's m8 of the library, as
make_training_library_golden.py makes it for the default mode.

For each case the reads are made on the CPU by tests/simlib_varlen_restated.simulate_varlen (the restatement the CPU tests pin
csrc/mc_simlib.h's mc_sim_walk_ref to), searched by oracle/rs_port (every read at its own length), and classified by training.py's
classify_reads exec'd unchanged with the read length as class_reads.py passes it (the nominal L).  Recorded: the table's rows, the
library's real base count (the reference's rate denominator), the m8's md5 and row count.

Output: tests/golden/training_varlen_<case>.json.gz.  Needs /root/reference and the built oracle (__graft_entry__.build()).
    python tests/golden/make_varlen_training_golden.py"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_training_library_golden as mk  # noqa: E402
import simlib_varlen_restated as svr  # noqa: E402
from microbecensus_amd import training  # noqa: E402

CASES = {
    "a": (1, 150, 12000, 201, dict(error_model="illumina")),                                      # illumina, single end
    "b": (2, 150, 12000, 202, dict(error_model="uniform", error_rate=0.03, paired_end=True, insert=300)),   # uniform, paired end
}


def main():
    ns = mk.reference_grid()
    data = os.path.join(mk.REF, "microbe_census", "data")
    gene2fam = dict(line.split() for line in open(os.path.join(data, "gene_fam.map")))
    gene2len = {k: int(v) for k, v in (line.split() for line in open(os.path.join(data, "gene_len.map")))}
    fams = set(gene2fam.values())
    aln_covs, max_pids, min_scores = [0.00, 0.25, 0.50, 0.75], [50, 60, 70, 80, 90, 100], ns["drange"](23, 50, 1)
    for case, (gk, L, n, seed, kind) in sorted(CASES.items()):
        name, bases, off = mk.load_genome(gk)
        lid = training.library_id(name, L)
        vb, vo, _ = svr.simulate_varlen(bases, off, L, 0, n, seed, lid, **kind)
        reads = [vb[vo[i]:vo[i + 1]].tobytes() for i in range(n)]
        with tempfile.TemporaryDirectory() as td:
            m8_bytes = mk.oracle_m8(reads, td, case)
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
        lens = [len(r) for r in reads]
        doc = {"source": "training/training.py:311-334 classify_reads on oracle/rs_port's m8 of a simulated library in the reference read-length mode, read_length '%d'" % L,
               "library": {"genome": name, "genome_index": gk, "read_len": L, "nreads": n, "seed": seed, "library_id": lid, "kind": kind},
               "library_bases": int(vo[-1]), "min_len": min(lens), "max_len": max(lens), "reads_md5": hashlib.md5(vb.tobytes()).hexdigest(),
               "m8_md5": hashlib.md5(m8_bytes).hexdigest(), "m8_rows": m8_bytes.count(b"\n"),
               "aln_covs": aln_covs, "max_pids": max_pids, "min_scores": [float(v) for v in min_scores], "n_rows_with_hits": len(rows), "rows": rows}
        path = os.path.join(HERE, "training_varlen_%s.json.gz" % case)
        mk.write_gz(path, json.dumps(doc).encode())
        print("case %s: %s L=%d %d reads %s: lengths %d..%d, %d bases, %d m8 rows, %d table rows, %d bytes"
              % (case, name, L, n, kind, min(lens), max(lens), doc["library_bases"], doc["m8_rows"], len(rows), os.path.getsize(path)))


if __name__ == "__main__":
    main()
