"""run_abundance behind the device, without one: abundance.build_table and abundance.write_outputs on the records that the device pass
left for every case of abundance_table_cases.py (tests/golden/abundance_tables.npz) give, byte for byte, the files that the commit
before the split into stages wrote for the same cases (tests/golden/abundance_tables.json; make_abundance_tables_golden.py says where
both come from) - and the refusals that compare the two records are build_table's."""
import copy

import numpy as np
import pytest

import abundance_table_cases as TC
from microbecensus_amd import _native, abundance, microbe_census


@pytest.fixture(scope="module")
def records():
    """every case's (sample, counts), loaded once; a test that changes one works on a copy"""
    with np.load(TC.RECORDS) as npz:
        return {case: TC.unpack(npz, case) for case in TC.CASES}


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", boom)
    monkeypatch.setattr(microbe_census, "run_pipeline", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _request(case, d):
    args = TC.request(case, d, reads=False)
    return (args,) + abundance.check_request(args)[:3]


@pytest.mark.parametrize("case", list(TC.CASES))
def test_the_stored_records_give_the_parents_files(case, records, no_engine, tmp_path):
    args, names, seqs, group_of = _request(case, tmp_path)
    sample, counts = copy.deepcopy(records[case])
    table = abundance.build_table(args, sample, counts, names, seqs, group_of)
    abundance.write_outputs(args, table)
    assert TC.hashes_of(args) == TC.expected()[case]
    assert args["sampled_reads"] == counts["sampled"] == table["sampled_reads"] and args["search_ms"] == counts["search_ms"]


def test_the_fixture_holds_every_case_and_no_path(records):
    assert set(TC.expected()) == set(TC.CASES) == set(records)
    for case, (sample, counts) in records.items():
        assert set(sample) == {"ags", "source", "pargs", "classes", "L"} and "seqfiles" not in sample["pargs"], case
        assert counts["ab"]["searched"] == counts["sampled"] > 0, case


def test_build_table_refuses_counts_that_contradict_the_sample(records, no_engine, tmp_path):
    args, names, seqs, group_of = _request("plain", tmp_path)
    sample, counts = copy.deepcopy(records["plain"])
    counts["ab"]["searched"] += 1
    with pytest.raises(abundance.AbundanceError, match=r"the gene search saw %d reads \(%d sampled\)" % (counts["sampled"] + 1, counts["sampled"])):
        abundance.build_table(args, sample, counts, names, seqs, group_of)
    args, names, seqs, group_of = _request("curve", tmp_path)
    sample, counts = copy.deepcopy(records["curve"])
    counts["cu"]["beyond"] = 1
    with pytest.raises(abundance.AbundanceError, match=r"the curve: 1 assigned reads lie behind the last point %d \(%d sampled\)" % (counts["sampled"], counts["sampled"])):
        abundance.build_table(args, sample, counts, names, seqs, group_of)
