"""tests/grid_restated.py (the training grid restated in plain Python over m8 text) against the .hits tables the REFERENCE's own
classify_reads made: the unit-test metagenome (training_grid_unittest.json.gz) and the simulated libraries of
make_training_library_golden.py (training_library_<case>.json.gz, with their m8).  Hits and aligned residues exactly, coverage
sums to 1e-12 relative.  This pins the restatement, so the GPU tests can use it where no golden exists.  No GPU, no reference."""
import gzip
import hashlib
import json
import os

import pytest

import grid_restated as gr
from microbecensus_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES = [("training_grid_unittest.json.gz", "unittest_metagenome.m8.gz", 100)] + [
    ("training_library_%s.json.gz" % c, "training_library_%s.m8.gz" % c, None) for c in "abc"]


@pytest.fixture(scope="module")
def markers():
    """gene2fam, gene2len, families of the packaged marker set (the reference's gene_fam.map / gene_len.map, restricted to the
    deduplicated markers the database holds)."""
    names, seqs = _native.load_markers()
    model = _native.load_model()
    fams = model["families"]
    return {n: fams[f] for n, f in zip(names, model["marker_family"])}, {n: len(s) for n, s in zip(names, seqs)}, fams


def check_against_golden(got, gold, fams):
    want = {}
    for fam, aln_cov, max_pid, min_score, hits, aln, cov in gold["rows"]:
        want[(gold["aln_covs"].index(aln_cov), gold["max_pids"].index(max_pid), gold["min_scores"].index(min_score), fam)] = (hits, aln, cov)
    assert len(want) == gold["n_rows_with_hits"]
    assert set(got) == set(want)
    for k, (hits, aln, cov) in want.items():
        g = got[k]
        assert g[0] == hits and g[1] == aln, (k, g, want[k])
        assert abs(g[2] - cov) <= 1e-12 * cov, (k, g, want[k])


@pytest.mark.parametrize("gold_file,m8_file,read_len", CASES, ids=["unittest", "a", "b", "c"])
def test_restatement_equals_reference(markers, gold_file, m8_file, read_len):
    gene2fam, gene2len, fams = markers
    gold = json.load(gzip.open(os.path.join(GOLD, gold_file), "rt"))
    raw = gzip.open(os.path.join(GOLD, m8_file), "rb").read()
    if "m8_md5" in gold:
        assert hashlib.md5(raw).hexdigest() == gold["m8_md5"] and raw.count(b"\n") == gold["m8_rows"]
        read_len = gold["library"]["read_len"]
    text = raw.decode()
    got = gr.classify(text, gold["aln_covs"], gold["max_pids"], gold["min_scores"], gene2len, gene2fam, fams, str(read_len))
    check_against_golden(got, gold, fams)
    assert sum(v[0] for v in got.values()) > 5000


def test_goldens_cover_what_training_feeds_the_grid(markers):
    """The three libraries span L mod 3 = 0, 1, 2, carry gapped and reverse-strand rows, and reads whose best-score tie is
    consequential (the tied rows differ in family, alignment length or target length)."""
    gene2fam, gene2len, _ = markers
    mods, kinds = set(), set()
    for c in "abc":
        gold = json.load(gzip.open(os.path.join(GOLD, "training_library_%s.json.gz" % c), "rt"))
        lib = gold["library"]
        mods.add(lib["read_len"] % 3)
        kinds.add((lib["kind"].get("error_model"), lib["kind"].get("paired_end", False)))
        text = gzip.open(os.path.join(GOLD, "training_library_%s.m8.gz" % c), "rt").read()
        rows = gr.parse_m8(text)
        gapped = sum(1 for line in text.splitlines() if int(line.split()[5]) > 0)
        reverse = sum(1 for r in rows if r[4] > r[5])
        ties = gr.consequential_ties(text, gene2fam, gene2len)
        print(c, lib, "rows", len(rows), "gapped", gapped, "reverse", reverse, "consequential ties", ties)
        assert reverse > 0 and ties > 0, c
        if lib["kind"].get("error_model"):
            assert gapped > 0, c
    assert mods == {0, 1, 2}
    assert kinds == {("illumina", True), ("uniform", False), (None, False)}
