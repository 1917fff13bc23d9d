#!/usr/bin/env python3
"""The records between run_abundance's stages, for every case of tests/abundance_table_cases.py: tests/golden/abundance_tables.npz.

Every case goes through abundance.resolve_sample and abundance.device_pass on the GPU; `sample` (of run_pipeline's args only what
build_table reads: no path, no thread count, no time) and `counts` are stored with np.savez_compressed.  Before the file is written,
build_table and write_outputs on the stored records must give the hashes of tests/golden/abundance_tables.json - which are NOT made
here: they are those of the files the commit before the split into stages wrote for the same cases (its run_abundance, run twice on
the GPU with equal hashes; the JSON's "source" names the commit), and "long_joined" in it names the three markers that
test_three_markers_joined_are_counted_as_one_long_gene's recipe picks (abundance_table_cases.pick_joined on the example reads).
Needs an MI355X and the built library (__graft_entry__.build()).
    python tests/golden/make_abundance_tables_golden.py [OUT.npz]"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import abundance_table_cases as TC  # noqa: E402
from microbecensus_amd import abundance, microbe_census  # noqa: E402


def main(out):
    want, records = TC.expected(), {}
    with tempfile.TemporaryDirectory() as d:
        for case in TC.CASES:
            args = TC.request(case, d)
            names, seqs, group_of, ags, source = abundance.check_request(args)
            microbe_census.check_input(args)
            sample = abundance.resolve_sample(args, ags, source)
            TC.pack(case, sample, abundance.device_pass(args, sample, names, seqs, group_of), records)
        np.savez_compressed(out, **records)
        with np.load(out) as npz:          # what the CPU test will do: the stored records alone give the files
            for case in TC.CASES:
                args = TC.request(case, d, reads=False)
                names, seqs, group_of, _, _ = abundance.check_request(args)
                sample, counts = TC.unpack(npz, case)
                abundance.write_outputs(args, abundance.build_table(args, sample, counts, names, seqs, group_of))
                got = TC.hashes_of(args)
                assert got == want[case], (case, got, want[case])
                print("%-10s %s" % (case, " ".join(sorted(got))))
    print("%s: %d arrays, %d bytes" % (out, len(records), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else TC.RECORDS)
