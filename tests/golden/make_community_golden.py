#!/usr/bin/env python3
"""The reference's own estimate of a simulated community library: tests/golden/community_golden.json.

  1. a community of 20 of the 30 genomes of tests/golden/genomes/genomes30.npz with uneven copies; its library (error-free, single
     end, 100 bp) is made on the CPU by tests/emul/community.cpp - the g++ build of the draw and the generator the device kernels
     run (csrc/mc_simlib.h); the md5 of the reads' bytes is recorded;
  2. the reads are written as a FASTA (">%d") and given to the REFERENCE's run_pipeline - its own Python and its own rapsearch
     binary, loaded as make_golden.py loads them - with -n = the library's reads and -l 100; its est_ags is recorded.

Only the JSON is committed (a recorded result; the reads are 30 MB and come back from the same command).  Needs /root/reference and
the built oracle (__graft_entry__.build()).
    python tests/golden/make_community_golden.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
sys.path.insert(0, REPO)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
import community_restated as cr  # noqa: E402
import make_golden  # noqa: E402
from microbecensus_amd import training, validation  # noqa: E402

NAME, L, NREADS, SEED = "golden20", 100, 300000, 20261016
INDICES = [0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15, 16, 18, 19, 21, 22, 24, 25, 27, 28]
ABUNDANCES = ["0.20", "0.01", "0.05", "0.12", "0.02", "0.08", "0.03", "0.10", "0.015", "0.06", "0.04", "0.005", "0.07", "0.025", "0.03", "0.05", "0.02", "0.04", "0.03", "0.01"]


def main():
    members = cr.fixture_members(INDICES)
    copies = validation.copies_of([m[0] for m in members], ABUNDANCES)
    bases, off, mfirst = cr.join_members([(b, o) for _, b, o in members])
    lid = training.library_id(NAME, L)
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "community")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(TESTS, "emul", "community.cpp")])
        files = {k: os.path.join(td, k + ".bin") for k in ("bases", "off", "mfirst", "copies", "out", "places")}
        for k, a in (("bases", bases), ("off", off.astype(np.int64)), ("mfirst", mfirst.astype(np.int32)), ("copies", np.array(copies, np.int64))):
            with open(files[k], "wb") as f:
                f.write(a.tobytes())
        subprocess.check_call([exe, files["bases"], files["off"], files["mfirst"], files["copies"], str(L), "0", "0", "0", "0.0", str(SEED), str(lid), "0", str(NREADS),
                               files["out"], files["places"]])
        reads = np.frombuffer(open(files["out"], "rb").read(), dtype=np.uint8).reshape(NREADS, L)
        fa = os.path.join(td, "%s_%d.fa" % (NAME, L))
        training.write_reads(fa, reads)
        mc, scratch = make_golden.load_reference()
        est, args = mc.run_pipeline({"seqfiles": [fa], "nreads": NREADS, "read_length": L, "threads": max(1, min(16, len(os.sched_getaffinity(0))))})
        assert args["sampled_reads"] == NREADS
    truth = validation.true_ags(copies, [int(o[-1]) for _, _, o in members])
    doc = {"source": "the reference's run_pipeline (its rapsearch binary) on the FASTA of a community library made by tests/emul/community.cpp",
           "library": {"name": NAME, "genome_indices": INDICES, "abundances": ABUNDANCES, "copies": copies, "read_len": L, "nreads": NREADS, "seed": SEED,
                       "library_id": lid, "kind": {}},
           "reads_md5": hashlib.md5(reads.tobytes()).hexdigest(), "true_ags": truth, "est_ags": est, "error": (est - truth) / truth}
    with open(os.path.join(HERE, "community_golden.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("%s: %d reads of %d bp, md5 %s; reference est_ags %r, true %r (%+.4f)" % (NAME, NREADS, L, doc["reads_md5"], est, truth, doc["error"]))


if __name__ == "__main__":
    main()
