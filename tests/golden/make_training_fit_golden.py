#!/usr/bin/env python3
"""Golden vector for the training workflow's parameter fit (optimize_parameters.py), produced by RUNNING THE REFERENCE's own
functions here: xvalidation, xfold_indexes, estimate_proportionality_constant, test_error and find_opt_pars of
training/training.py are read from /root/reference at generation time and exec'd UNCHANGED.  The Python 2 semantics they rely
on are supplied from outside their text: a `range` that returns a list (xfold_indexes removes from it), a fold count whose
division floors (`fold_size = n/x`), and a queue that collects what xvalidation puts.  find_opt_pars is fed the candidates in
the order microbecensus_amd/training.py fixes (min_score, max_pid, aln_cov ascending; rate type hits, aln, cov).

Inputs: seeded synthetic per-genome counts over 2 read lengths x 3 families x the full 4 x 6 x 27 grid x 3 rate types, with
zero counts and exact ties; rate = count / library bp.  Two cases: 12 genomes with x = 5 (two genomes never in a test fold) and
10 genomes with x = 10.

Output: tests/golden/training_fit.json.gz.  Only runs where /root/reference exists."""
import gzip
import json
import os
import re

import numpy

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ALN_COVS = [0.0, 0.25, 0.5, 0.75]
MAX_PIDS = [50, 60, 70, 80, 90, 100]
MIN_SCORES = list(range(23, 50))
RATE_TYPES = ["rate_hits", "rate_aln", "rate_cov"]


class FloorInt(int):
    """x of xvalidation: n / x floors, as Python 2's int division."""
    def __rtruediv__(self, n):
        return int(n) // int(self)

    def __truediv__(self, m):
        return int(self) // int(m)


class Queue(list):
    def put(self, v):
        self.append(v)


def reference_functions():
    src = open(os.path.join(REF, "training", "training.py")).read()
    blocks = {m.group(1): m.group(0) for m in re.finditer(r"^def (\w+)\(.*?(?=^\S)", src + "\n#", flags=re.S | re.M)}
    ns = {"numpy": numpy, "range": lambda *a: list(range(*a))}
    for name in ("xvalidation", "xfold_indexes", "estimate_proportionality_constant", "test_error", "find_opt_pars"):
        exec(blocks[name], ns)
    return ns


def make_case(rng, n_genomes, x, ns):
    genomes = ["genome%02d" % i for i in range(n_genomes)]
    sizes = {g: int(rng.integers(1_000_000, 8_000_000)) for g in genomes}
    lib_bp = {g: int(rng.integers(500_000, 5_000_000)) * 10 for g in genomes}
    cands = [(s, p, c, t) for s in MIN_SCORES for p in MAX_PIDS for c in ALN_COVS for t in range(3)]
    case = {"xfolds": x, "genomes": genomes, "sizes": sizes, "library_bp": lib_bp, "counts": {}, "expected": {}}
    for L in ("100", "150"):
        case["counts"][L], case["expected"][L] = {}, {}
        for fam in ("famA", "famB", "famC"):
            # counts shrink with the cut-offs; small integers make exact ties; a sparse family has zeros
            lam = rng.uniform(5, 40) * (0.05 if fam == "famC" else 1.0)
            counts = rng.poisson(lam, size=(n_genomes, len(cands))).astype(numpy.int64)
            counts[:, 1::7] = counts[:, 0::7][:, : counts[:, 1::7].shape[1]]        # duplicated columns: exact ties
            case["counts"][L][fam] = counts.tolist()
            xval, q = [], Queue()
            for k, (s, p, c, t) in enumerate(cands):
                rates = [float(counts[i, k]) / lib_bp[g] for i, g in enumerate(genomes)]
                ns["xvalidation"]((L, fam, s, p, c, RATE_TYPES[t]), FloorInt(x), genomes, rates, sizes, q)
            xval = list(q)
            opt = ns["find_opt_pars"](xval)[(L, fam)]
            s, p, c, t = opt["pars"]
            k = cands.index((s, p, c, RATE_TYPES.index(t)))
            rates = [float(counts[i, k]) / lib_bp[g] for i, g in enumerate(genomes)]
            coeff = ns["estimate_proportionality_constant"](genomes, rates, sizes)
            preds = [coeff / r if r > 0 else "NA" for r in rates]
            case["expected"][L][fam] = {"pars": [s, p, c, t], "index": k, "error": float(opt["error"]), "coefficient": float(coeff),
                                        "preds": preds, "errors": [float(e) for _, e in xval]}
    return case


def main():
    ns = reference_functions()
    rng = numpy.random.default_rng(20261015)
    out = {"candidates": "min_score ascending, max_pid ascending, aln_cov ascending, rate type hits / aln / cov",
           "cases": [make_case(rng, 12, 5, ns), make_case(rng, 10, 10, ns)]}
    path = os.path.join(HERE, "training_fit.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
