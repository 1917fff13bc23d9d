"""Coverage breadth and depth, host side (no GPU): the restatement of csrc/k_coverage.h's statement on hand-made rows with known answers
and on the reference binary's two m8 goldens (figures computed from them beforehand), the new columns, the `detected` rule at its
boundary, the run-length encoding of the depth, every refusal before an engine is opened, the unchanged table without the switches,
and the four new symbols of the ABI."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import abundance_restated as R
import coverage_restated as V
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")

NAMES = ["gA", "gB", "gC", "gD"]
LENGTHS = [50, 60, 40, 30]


def _m8(rows):
    return "".join("%s\t%s\t%g\t%d\t0\t0\t1\t2\t%d\t%d\t%g\t%g\n" % r for r in rows)


# query, subject, identity, alnlen, sstart, send, log(e), bits
HAND = _m8([
    ("r0", "gA", 90.0, 30, 0, 0, -3.0, 60.0),          # [0, 0]; a tie on bits with the next row: the first row's span wins
    ("r0", "gB", 90.0, 30, 5, 9, -3.0, 60.0),
    ("r1", "gA", 90.0, 50, 0, 49, -3.0, 70.0),         # [0, len - 1]
    ("r2", "gA", 90.0, 30, 49, 49, -3.0, 50.0),        # [len - 1, len - 1]
    ("r3", "gB", 90.0, 30, 10, 30, -3.0, 50.0),        # two overlapping spans: 20 .. 30 twice
    ("r4", "gB", 90.0, 30, 20, 40, -3.0, 50.0),
    ("r5", "gC", 50.0, 40, 0, 39, -3.0, 90.0),         # the top row fails min_ident 60: the second row's span counts
    ("r5", "gD", 90.0, 30, 3, 12, -3.0, 40.0),
    ("r6", "gC", 20.0, 10, 5, 14, 0.9, 10.0),          # no passing row under the cut-offs
])


def _gene(cov, k):
    a = sum(LENGTHS[:k])
    return cov["depth"][a:a + LENGTHS[k]].tolist()


def test_restatement_on_hand_made_rows():
    rows = V.rows_from_m8(HAND, NAMES)
    assert [r[6:] for r in rows] == [(0, 0), (5, 9), (0, 49), (49, 49), (10, 30), (20, 40), (0, 39), (3, 12), (5, 14)]
    assert [r[:6] for r in rows] == R.rows_from_m8(HAND, NAMES)
    none = V.coverage(rows, LENGTHS)
    assert none["best"] == [(0, 0, 0), (0, 0, 49), (0, 49, 49), (1, 10, 30), (1, 20, 40), (2, 0, 39), (2, 5, 14)]
    assert _gene(none, 0) == [2] + [1] * 48 + [2]
    assert _gene(none, 1) == [0] * 10 + [1] * 10 + [2] * 11 + [1] * 10 + [0] * 19
    assert _gene(none, 2) == [1] * 5 + [2] * 10 + [1] * 25 and _gene(none, 3) == [0] * 30
    assert none["covered"].tolist() == [50, 31, 40, 0] and none["spanned"].tolist() == [52, 42, 50, 0] and none["max_depth"].tolist() == [2, 2, 2, 0]
    cut = V.coverage(rows, LENGTHS, min_ident=60, min_aln=25)
    assert cut["best"] == [(0, 0, 0), (0, 0, 49), (0, 49, 49), (1, 10, 30), (1, 20, 40), (3, 3, 12)]              # r5 by its second row; r6 lost
    assert cut["covered"].tolist() == [50, 31, 0, 10] and cut["spanned"].tolist() == [52, 42, 0, 10] and cut["max_depth"].tolist() == [2, 2, 0, 1]
    assert _gene(cut, 3) == [0] * 3 + [1] * 10 + [0] * 17
    # the tie the other way round: the first row in file order, whichever subject it names
    swapped = V.rows_from_m8(_m8([("r0", "gB", 90.0, 30, 5, 9, -3.0, 60.0), ("r0", "gA", 90.0, 30, 0, 0, -3.0, 60.0)]), NAMES)
    assert V.coverage(swapped, LENGTHS)["covered"].tolist() == [0, 5, 0, 0]
    # spanned is the sum of send - sstart + 1 over the best rows; the invariants hold with the restated counts
    for cov, kw in ((none, {}), (cut, dict(min_ident=60, min_aln=25))):
        per = np.zeros(4, np.int64)
        for s, a, b in cov["best"]:
            per[s] += b - a + 1
        assert per.tolist() == cov["spanned"].tolist()
        assert V.invariants(cov, R.abundance(R.rows_from_m8(HAND, NAMES), 4, **kw)["reads"], LENGTHS) == []
    # the same rows as an mc_row array
    arr = np.zeros(len(rows), _native.ROW_DTYPE)
    for i, (q, s, nm, al, bits, loge, a, b) in enumerate(rows):
        arr[i] = (int(q[1:]), s, nm * 100.0 / al, al, 0, 0, 1, 2, a, b, loge, bits, 0, nm)
    got = V.coverage(V.rows_from_array(arr), LENGTHS, min_ident=60, min_aln=25)
    assert all(np.array_equal(got[k], cut[k]) for k in ("covered", "spanned", "max_depth", "depth"))


def _figures(rows, lengths):
    for r in rows:                                                          # the fact the statement builds on
        assert 0 <= r[6] <= r[7] <= lengths[r[1]] - 1, r
    cov = V.coverage(rows, lengths)
    ab = R.abundance([r[:6] for r in rows], len(lengths))
    assert V.invariants(cov, ab["reads"], lengths) == [] and np.array_equal(np.bincount([b[0] for b in cov["best"]], minlength=len(lengths)), ab["reads"])
    return (len(cov["best"]), int((cov["covered"] > 0).sum()), int(cov["covered"].sum()), int(cov["spanned"].sum()), int(cov["max_depth"].max()),
            int((cov["max_depth"] > 1).sum()), sum(1 for s, a, b in cov["best"] if a == 0), sum(1 for s, a, b in cov["best"] if b == lengths[s] - 1))


def test_reference_m8_of_the_marker_database():
    """assigned reads, genes hit, sum covered, sum spanned, max depth, genes with depth > 1, best rows starting at 0, ending at len - 1 -
    from the reference binary's m8 of the example reads, no cut-offs"""
    names, seqs = _native.load_markers()
    rows = V.rows_from_m8(os.path.join(GOLD, "config1_example_fq.m8.gz"), names)
    assert len(rows) == 7286
    assert _figures(rows, [len(s) for s in seqs]) == (251, 239, 5167, 5288, 2, 6, 6, 4)


def test_reference_m8_of_the_generic_database():
    sys.path.insert(0, GOLD)
    import make_generic_db_golden as G
    from microbecensus_amd import synth
    meta = json.load(open(os.path.join(GOLD, "generic_db.json")))
    names, seqs = synth.random_proteins(G.CASE["db_residues"], seed=G.CASE["db_seed"])
    rows = V.rows_from_m8(os.path.join(GOLD, "generic_db.m8.gz"), names)
    assert len(rows) == meta["m8_rows"] == 12542 and len(names) == meta["sequences"]
    assert _figures(rows, [len(s) for s in seqs]) == (10502, 1614, 204416, 423613, 10, 879, 593, 549)


# ---- the columns, the detected rule, the depth file ------------------------------------------------------------------------------------
def test_columns_and_the_detected_rule_at_its_boundary():
    length = np.array([10, 10, 10, 3, 7], np.int64)
    covered = np.array([5, 4, 10, 0, 7], np.int64)
    spanned = np.array([15, 4, 25, 0, 7], np.int64)
    reads = np.array([3, 1, 4, 0, 1], np.int64)
    breadth, mean_depth = abundance.coverage_columns(length, covered, spanned)
    assert breadth.tolist() == [0.5, 0.4, 1.0, 0.0, 1.0] and mean_depth.tolist() == [1.5, 0.4, 2.5, 0.0, 1.0]
    assert abundance.detect(reads, covered, length, 0.5).tolist() == [1, 0, 1, 0, 1]         # 5 of 10 at F = 0.5 is detected, 4 of 10 is not
    assert abundance.detect(reads, covered, length, 1.0).tolist() == [0, 0, 1, 0, 1]
    assert abundance.detect(reads, covered, length, 0.4).tolist() == [1, 1, 1, 0, 1]
    assert abundance.detect(reads, covered, length, 1e-9).tolist() == [1, 1, 1, 0, 1]        # a gene without reads never, however small F
    assert abundance.detect([0, 2], [0, 0], [5, 5], 0.1).tolist() == [0, 0]
    assert abundance.detect([1, 1], [7, 6], [10, 10], 0.7).tolist() == [1, 0] and abundance.detect([1, 1], [2, 1], [3, 3], 0.6).tolist() == [1, 0]


def test_depth_run_length_encoding(tmp_path):
    names = ["g1", "g2", "g3", "g4", "g5"]
    length = [6, 4, 3, 1, 2]
    depth = np.array([0, 2, 2, 1, 0, 3,        # a run that ends at the gene's last residue ...
                      3, 3, 0, 0,              # ... and the next gene begins with the same depth: two runs
                      0, 0, 0,                 # a gene without reads: no line
                      70000,                   # one residue, a depth past 16 bits
                      1, 1], np.uint32)
    g, a, b, d = abundance.depth_runs(depth, length)
    assert list(zip(g.tolist(), a.tolist(), b.tolist(), d.tolist())) == [(0, 1, 3, 2), (0, 3, 4, 1), (0, 5, 6, 3), (1, 0, 2, 3), (3, 0, 1, 70000), (4, 0, 2, 1)]
    out = str(tmp_path / "depth.tsv")
    abundance.write_depth(out, names, length, depth)
    assert open(out).read() == "#gene\tstart\tend\tdepth\ng1\t1\t3\t2\ng1\t3\t4\t1\ng1\t5\t6\t3\ng2\t0\t2\t3\ng4\t0\t1\t70000\ng5\t0\t2\t1\n"
    assert np.array_equal(abundance.read_depth(out, names, length), depth)
    abundance.write_depth(out, names, length, np.zeros(16, np.uint32))
    assert open(out).read() == "#gene\tstart\tend\tdepth\n"
    with pytest.raises(ValueError, match="15 depths for genes of 16 residues"):
        abundance.depth_runs(depth[:15], length)
    # the restatement's depth of the hand-made rows, through the file and back
    cov = V.coverage(V.rows_from_m8(HAND, NAMES), LENGTHS)
    abundance.write_depth(out, NAMES, LENGTHS, cov["depth"])
    lines = open(out).read().split("\n")[1:-1]
    assert lines[:3] == ["gA\t0\t1\t2", "gA\t1\t49\t1", "gA\t49\t50\t2"] and lines[3] == "gB\t10\t20\t1" and not any(l.startswith("gD") for l in lines)
    assert np.array_equal(abundance.read_depth(out, NAMES, LENGTHS), cov["depth"])


def _table():
    ge = abundance.genome_equivalents(8672, 100, 3051745.7641809303)
    reads, length = np.array([5, 0, 7], np.int64), np.array([120, 300, 2047], np.int64)
    return {"gene": ["g1", "g2", "g3"], "length_aa": length, "reads": reads, "aligned_aa": np.array([150, 0, 231], np.int64), "rpkg": abundance.rpkg(reads, length, ge),
            "sampled_reads": 8672, "trimmed_length": 100, "ags": 3051745.7641809303, "ags_source": "run_pipeline", "genome_equivalents_sampled": ge, "reads_assigned": 12}


ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": "map.tsv"}
TODAY = ["# metagenome:\ta.fq.gz", "# genes:\tgenes.faa", "# sampled_reads:\t8672", "# trimmed_length:\t100", "# min_ident:\t60", "# min_aln:\t30", "# min_bits:\t35.5",
         "# average_genome_size:\t3051745.7641809303", "# ags_source:\trun_pipeline", "# genome_equivalents_sampled:\t%r" % (8672 * 100 / 3051745.7641809303),
         "# reads_assigned:\t12"]


def test_tables_without_the_switches_are_todays(tmp_path):
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11] == "gene\tlength_aa\treads\taligned_aa\trpkg"
    assert lines[12] == "g1\t120\t5\t150\t%r" % (5 / (3 * 120 / 1000.0) / t["genome_equivalents_sampled"]) and lines[13] == "g2\t300\t0\t0\t0.0"
    assert lines[14] == "g3\t2047\t7\t231\t%r" % float(t["rpkg"][2]) and lines[15:] == [""]
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    assert t["groups"] == [("X", 2, 12, float(t["rpkg"][0]) + float(t["rpkg"][2])), ("g2", 1, 0, 0.0)]
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    lines = open(out + ".groups.tsv").read().split("\n")
    assert lines[:11] == TODAY and lines[11:13] == ["# groups:\tmap.tsv", "group\tgenes\treads\trpkg"]
    assert lines[13:] == ["X\t2\t12\t%r" % (float(t["rpkg"][0]) + float(t["rpkg"][2])), "g2\t1\t0\t0.0", ""]


def test_tables_with_the_switches(tmp_path):
    t = _table()
    covered, spanned = np.array([60, 0, 100], np.int64), np.array([150, 0, 231], np.int64)
    breadth, mean_depth = abundance.coverage_columns(t["length_aa"], covered, spanned)
    t.update({"covered_aa": covered, "breadth": breadth, "mean_depth": mean_depth, "max_depth": np.array([4, 0, 7], np.int64)})
    out = str(tmp_path / "cov.tsv")
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11] == "# coverage:\ton" and lines[12] == "gene\tlength_aa\treads\taligned_aa\trpkg\tcovered_aa\tbreadth\tmean_depth\tmax_depth"
    assert lines[13] == "g1\t120\t5\t150\t%r\t60\t0.5\t1.25\t4" % float(t["rpkg"][0]) and lines[14] == "g2\t300\t0\t0\t0.0\t0\t0.0\t0.0\t0"
    assert lines[15] == "g3\t2047\t7\t231\t%r\t100\t%r\t%r\t7" % (float(t["rpkg"][2]), 100 / 2047, 231 / 2047) and lines[16:] == [""]
    t["min_breadth"] = 0.5
    t["detected"] = abundance.detect(t["reads"], covered, t["length_aa"], 0.5)
    assert t["detected"].tolist() == [1, 0, 0]
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"}, t["detected"])
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11:14] == ["# coverage:\ton", "# min_breadth:\t0.5", "# genes_detected:\t1"]
    assert lines[14].endswith("\tmax_depth\tdetected") and [l.rsplit("\t", 1)[1] for l in lines[15:18]] == ["1", "0", "0"]
    header, rows = abundance.read_table(out)
    assert len(rows) == 3 and [r[:5] for r in rows] == [[g, str(l), str(r), str(a), repr(float(v))] for g, l, r, a, v in zip(t["gene"], t["length_aa"], t["reads"], t["aligned_aa"], t["rpkg"])]
    assert [float(r[6]) for r in rows] == breadth.tolist() and header["genes_detected"] == "1"       # repr round-trips
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    lines = open(out + ".groups.tsv").read().split("\n")
    assert lines[11:16] == ["# coverage:\ton", "# min_breadth:\t0.5", "# genes_detected:\t1", "# groups:\tmap.tsv", "group\tgenes\treads\trpkg\tgenes_detected"]
    assert lines[16:] == ["X\t2\t12\t%r\t1" % (float(t["rpkg"][0]) + float(t["rpkg"][2])), "g2\t1\t0\t0.0\t0", ""]


# ---- refusals, before any engine is opened ----------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", boom)
    monkeypatch.setattr(microbe_census, "run_pipeline", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_refusals_and_what_the_switches_imply(tmp_path, no_engine):
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    faa = tmp_path / "good.faa"
    faa.write_text(">g1 d\n%s\n>g2 d\n%s\n" % ("MKV" * 20, "MLA" * 30))
    out = str(tmp_path / "out.tsv")

    def request(**kw):
        args = {"seqfiles": [fq], "genes": str(faa), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    for bad, shown in ((0, "0"), (0.0, "0.0"), (-0.25, "-0.25"), (1.0000001, "1.0000001"), (2, "2"), (float("nan"), "nan"), (float("inf"), "inf"), ("half", "half"), (True, "True")):
        with pytest.raises(abundance.AbundanceError, match="--min-breadth %s is not a fraction" % shown.replace(".", "\\.")):
            abundance.run_abundance(request(min_breadth=bad))
    for same in (out, os.path.join(str(tmp_path), ".", "out.tsv")):
        with pytest.raises(abundance.AbundanceError, match="--depth-out .*out.tsv is the path of the gene table itself"):
            abundance.run_abundance(request(depth_out=same))
    (tmp_path / "map.tsv").write_text("g1\tX\n")
    with pytest.raises(abundance.AbundanceError, match="--depth-out '' is an empty path"):
        abundance.run_abundance(request(depth_out=""))
    with pytest.raises(abundance.AbundanceError, match="--depth-out .*out.tsv.groups.tsv is the path of the groups table"):
        abundance.run_abundance(request(depth_out=out + ".groups.tsv", groups=str(tmp_path / "map.tsv")))
    assert not os.path.exists(out)
    # all three are off by default; min_breadth and depth_out imply coverage; F = 1 and a small F are taken
    a = request()
    abundance.check_request(a)
    assert (a["coverage"], a["min_breadth"], a["depth_out"]) == (False, None, None)
    for kw, f in ((dict(coverage=True), None), (dict(min_breadth=1), 1.0), (dict(min_breadth=1e-6), 1e-6), (dict(depth_out=str(tmp_path / "d.tsv")), None)):
        a = request(**kw)
        abundance.check_request(a)
        assert a["coverage"] is True and a["min_breadth"] == f
    with pytest.raises(AssertionError, match="GPU work was started"):          # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(min_breadth=0.5, depth_out=str(tmp_path / "d.tsv")))


def test_cli_switches():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])
    assert (a["coverage"], a["min_breadth"], a["depth_out"]) == (False, None, None)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--coverage", "--min-breadth", "0.1", "--depth-out", "d.tsv"])
    assert (a["coverage"], a["min_breadth"], a["depth_out"]) == (True, 0.1, "d.tsv")
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--min-breadth", "half"])


def test_coverage_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import re
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_set_coverage", "mc_coverage_read", "mc_coverage_depth", "mc_coverage_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("set_coverage", "coverage", "coverage_depth", "coverage_ms"):
        assert callable(getattr(_native.Engine, m))
