"""run_abundance end to end on every case of abundance_table_cases.py: the files are, byte for byte, those the commit before the split
into stages wrote (tests/golden/abundance_tables.json), and the device pass leaves, array for array, the records that the CPU test
builds its tables from (tests/golden/abundance_tables.npz) - the times aside."""
import numpy as np
import pytest

import abundance_table_cases as TC
from microbecensus_amd import abundance, microbe_census

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(TC.CASES))
def test_run_abundance_writes_the_parents_files_from_the_stored_counts(case, tmp_path):
    request = TC.request(case, tmp_path)
    table, args = abundance.run_abundance(dict(request))
    assert TC.hashes_of(args) == TC.expected()[case]
    args = dict(request)
    names, seqs, group_of, ags, source = abundance.check_request(args)
    microbe_census.check_input(args)
    sample = abundance.resolve_sample(args, ags, source)
    counts = abundance.device_pass(args, sample, names, seqs, group_of)
    with np.load(TC.RECORDS) as npz:
        want_sample, want = TC.unpack(npz, case)
    assert TC.same_counts(counts, want) == []
    assert (sample["ags"], sample["source"], sample["classes"], sample["L"]) == tuple(want_sample[k] for k in ("ags", "source", "classes", "L"))
