"""The rarefaction curve, host side (no GPU): the restatement of csrc/k_curve.h's statement (tests/curve_restated.py) on the reference
binary's m8 goldens the abundance tests use, under their three cut-off sets - point k against abundance_restated and coverage_restated on
the rows of the first n_k reads, the statement's invariants, and the condition that keeps it from passing empty -, the rules of
csrc/mc_curve.h themselves compiled by g++ (tests/emul/curve.cpp, once more under -fsanitize=address,undefined) on the cases the device
harness runs (tests/curve_cases.py), the new files' formats, every refusal before an engine is opened, NA points, the unchanged files
without the switch, and the new symbols of the ABI."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abundance_restated as R
import coverage_restated as V
import curve_cases as cc
import curve_restated as CR
import order_cases as oc
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
CUTS = [dict(), dict(min_ident=60, min_aln=30), dict(min_bits=27.1)]           # test_gpu_abundance.py's three
K_GOLDEN = 4                                                                     # (chosen here, on the CPU: the condition below holds on both goldens)


def _golden(case):
    """(rows with an int query, lengths, the reads the golden was made of) - the database cut down to the genes a row names, in their
    order: a gene without rows has zeros everywhere, and the restatements walk every residue in Python"""
    if case == "generic_db":
        sys.path.insert(0, GOLD)
        import make_generic_db_golden as G
        from microbecensus_amd import synth
        names, seqs = synth.random_proteins(G.CASE["db_residues"], seed=G.CASE["db_seed"])
        nreads = json.load(open(os.path.join(GOLD, case + ".json")))["reads"]
    else:
        names, seqs = _native.load_markers()
        nreads = json.load(open(os.path.join(GOLD, case + ".json")))["sampled_reads"]
    rows = V.rows_from_m8(os.path.join(GOLD, case + ".m8.gz"), names)
    used = sorted({r[1] for r in rows})
    new = {s: i for i, s in enumerate(used)}
    rows = [(int(r[0]), new[r[1]]) + tuple(r[2:]) for r in rows]
    assert all(0 <= r[0] < nreads for r in rows) and all(a[0] <= b[0] for a, b in zip(rows, rows[1:]))      # the query column is the read's id, ascending
    return rows, [len(seqs[s]) for s in used], nreads


@pytest.mark.parametrize("case", ["config1_example_fq", "generic_db"])
def test_restatement_on_the_reference_m8(case):
    rows, lengths, nreads = _golden(case)
    nseq = len(lengths)
    points = microbe_census.curve_points(nreads, K_GOLDEN)
    assert points[-1] == nreads and len(set(points)) == K_GOLDEN
    for cut in CUTS:
        cv = CR.curve(rows, lengths, points, **cut)
        for k, n_k in enumerate(points):
            head = [r for r in rows if r[0] < n_k]
            ab = R.abundance([r[:6] for r in head], nseq, **cut)
            cov = V.coverage(head, lengths, **cut)
            assert np.array_equal(cv["reads"][k], ab["reads"]) and np.array_equal(cv["aligned"][k], ab["aligned"]) and int(cv["assigned"][k]) == ab["assigned"], (case, cut, k)
            assert np.array_equal(cv["covered"][k], cov["covered"]), (case, cut, k)
        assert CR.invariants(cv, ab["reads"], ab["aligned"], cov["covered"]) == [] and cv["beyond"] == 0          # (ab, cov: the last point's - the whole golden)
        # not empty: the curve moves between the first and the last point
        assert 0 < (cv["reads"][0] > 0).sum() < (cv["reads"][-1] > 0).sum() and 0 < cv["covered"][0].sum() < cv["covered"][-1].sum(), (case, cut)
        # and a last point short of the sample leaves reads behind it, which the invariants name
        short = CR.curve(rows, lengths, points[:-1], **cut)
        assert short["beyond"] == int(cv["assigned"][-1] - cv["assigned"][-2]) > 0 and CR.invariants(short, ab["reads"], ab["aligned"], cov["covered"]) == []
        assert np.array_equal(short["reads"], cv["reads"][:-1]) and np.array_equal(short["covered"], cv["covered"][:-1])


def test_restatement_on_hand_made_rows():
    rows = cc.rows_of([(0, 0, 0, 9), (1, 1, 5, 19), (2, 0, 5, 29), (2, 1, 0, 0, 40.0), (5, 0, 0, 0)])
    cv = CR.curve(V.rows_from_array(rows), [30, 20], [1, 2, 2, 3])
    assert [CR.bin_of([1, 2, 2, 3], q) for q in (0, 1, 2, 3, 9)] == [0, 1, 3, 4, 4]
    assert cv["bin_reads"].tolist() == [[1, 0], [0, 1], [0, 0], [1, 0], [1, 0]] and cv["beyond"] == 1
    assert cv["reads"].tolist() == [[1, 0], [1, 1], [1, 1], [2, 1]] and cv["covered"].tolist() == [[10, 0], [10, 15], [10, 15], [30, 15]]
    assert cv["first"][0][:12] == [0] * 10 + [2, 2] and CR.first_flat(cv)[30:36].tolist() == [0xFFFFFFFF] * 5 + [1]
    ab = R.abundance(R.rows_from_array(rows), 2)
    assert CR.invariants(cv, ab["reads"], ab["aligned"]) == []
    broken = dict(cv, beyond=0)
    assert CR.invariants(broken, ab["reads"], ab["aligned"]) == ["a read behind the last point and beyond == 0"]
    off = CR.curve(V.rows_from_array(rows), [30, 20], [1, 2, 2, 3], coverage=False)
    assert not off["covered"].any() and np.array_equal(off["reads"], cv["reads"]) and CR.invariants(off, ab["reads"], ab["aligned"], coverage=False) == []


# ---- the rules of mc_curve.h on the CPU ---------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "curve")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(HERE, "emul", "curve.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "curve", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "curve_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _cpu(exe, c, coverage, tmp):
    name = "%s_%d" % (c["name"], coverage)
    oc.write_sections(tmp / (name + ".in"), cc.sections_in(c, coverage))
    p = subprocess.run([exe, "run", str(tmp / (name + ".in")), str(tmp / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and not p.stderr, (name, p.returncode, p.stderr.decode())
    o = oc.read_sections(tmp / (name + ".out"))
    return cc.compare(c, coverage, np.frombuffer(o[0], "<u8"), np.frombuffer(o[1], "<u4"), np.frombuffer(o[2], "<u8"))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rules_of_mc_curve_h_on_the_device_cases(which, driver, driver_san, tmp_path):
    exe = driver if which == "plain" else driver_san
    names = set()
    for c in cc.cases():
        for coverage in (1, 0):
            _cpu(exe, c, coverage, tmp_path)
        names.add(c["name"])
    assert {"k1", "k64", "repeats", "lengths", "genes1", "genes3", "genes4", "genes5", "straddle_0", "straddle_2", "hi_first", "lo_first"} <= names


def test_cases_reach_what_they_are_for():
    """the conditions of the cases, from the restatement alone: without them the device tests could pass empty"""
    by = {c["name"]: c for c in cc.cases()}
    k64 = cc.expect(by["k64"], 1)[0]
    assert len(by["k64"]["points"]) == 64 and all(int(by["k64"]["rows"]["query"][2 * k]) == n - 1 and int(by["k64"]["rows"]["query"][2 * k + 1]) == n for k, n in enumerate(by["k64"]["points"]))
    assert k64["beyond"] == 1 and (np.diff(k64["assigned"]) == 2).all() and by["k64"]["rows"]["query"].min() >= 1000
    assert cc.expect(by["k1"], 1)[0]["beyond"] == 3 and by["repeats"]["points"] == microbe_census.curve_points(3, 5) == [1, 2, 2, 3, 3]
    assert sorted(set(by["lengths"]["lengths"])) == [1, 5, 63, 64, 65, 70, 129, 2047] and [len(by["genes%d" % n]["lengths"]) for n in (1, 3, 4, 5)] == [1, 3, 4, 5]
    spans = {(int(r["sstart"]), int(r["send"])) for r in by["lengths"]["rows"] if r["subject"] == 15}
    assert spans == {(0, 0), (2046, 2046), (0, 2046)}
    hi, lo = by["hi_first"], by["lo_first"]
    assert hi["cuts"] == lo["cuts"] == [3, 6] and hi["rows"]["query"][0] > hi["rows"]["query"][3] and lo["rows"]["query"][0] < lo["rows"]["query"][3]


# ---- the figures, the files ---------------------------------------------------------------------------------------------------------------
NAMES = ["g1", "g2", "g3"]
LENGTH = np.array([120, 300, 2047], np.int64)
READS = np.array([[1, 0, 0], [3, 0, 2], [5, 0, 7]], np.int64)
ALIGNED = np.array([[30, 0, 0], [90, 0, 66], [150, 0, 231]], np.int64)
COVERED = np.array([[30, 0, 0], [55, 0, 60], [60, 0, 100]], np.int64)
ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": "map.tsv"}
TODAY = ["# metagenome:\ta.fq.gz", "# genes:\tgenes.faa", "# sampled_reads:\t8672", "# trimmed_length:\t100", "# min_ident:\t60", "# min_aln:\t30", "# min_bits:\t35.5",
         "# average_genome_size:\t3051745.7641809303", "# ags_source:\trun_pipeline", "# genome_equivalents_sampled:\t%r" % (8672 * 100 / 3051745.7641809303),
         "# reads_assigned:\t12"]


def _table():
    ge = abundance.genome_equivalents(8672, 100, 3051745.7641809303)
    return {"gene": list(NAMES), "length_aa": LENGTH, "reads": READS[-1], "aligned_aa": ALIGNED[-1], "rpkg": abundance.rpkg(READS[-1], LENGTH, ge),
            "sampled_reads": 8672, "trimmed_length": 100, "ags": 3051745.7641809303, "ags_source": "run_pipeline", "genome_equivalents_sampled": ge, "reads_assigned": 12}


def test_curve_figures_come_from_the_tables_own_lines():
    points = microbe_census.curve_points(8672, 3)
    cu = abundance.curve_figures(NAMES, LENGTH, 100, points, READS, ALIGNED, COVERED, [3.0e6, 3.1e6, 3051745.7641809303], 0.5, {"g1": "X", "g3": "X"})
    t = _table()
    assert cu["points"] == [2891, 5782, 8672] and cu["reads_assigned"] == [1, 5, 12] and cu["genes_with_reads"] == [1, 2, 2]
    assert cu["genome_equivalents_sampled"] == [abundance.genome_equivalents(n, 100, a) for n, a in zip(points, cu["ags"])]
    assert np.array_equal(cu["rpkg"][-1], t["rpkg"]) and cu["genome_equivalents_sampled"][-1] == t["genome_equivalents_sampled"]          # the last point is the table
    assert cu["detected"].tolist() == [abundance.detect(READS[k], COVERED[k], LENGTH, 0.5).tolist() for k in range(3)] == [[0, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert cu["genes_detected"] == [0, 0, 1] and cu["groups_with_reads"] == [1, 1, 1]
    assert cu["groups"][-1] == abundance.group_table(NAMES, READS[-1], t["rpkg"], {"g1": "X", "g3": "X"}, cu["detected"][-1])
    bare = abundance.curve_figures(NAMES, LENGTH, 100, points, READS, ALIGNED, None, [3.0e6] * 3)
    assert not {"covered_aa", "detected", "genes_detected", "groups", "groups_with_reads"} & set(bare)
    cov_only = abundance.curve_figures(NAMES, LENGTH, 100, points, READS, ALIGNED, COVERED, [3.0e6] * 3)
    assert "covered_aa" in cov_only and "detected" not in cov_only


def test_files_with_the_switch_and_na_points(tmp_path):
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, ARGS, t)
    before = open(out).read()
    points = microbe_census.curve_points(8672, 3)
    t["curve"] = abundance.curve_figures(NAMES, LENGTH, 100, points, READS, ALIGNED, COVERED, [None, 3.1e6, 3051745.7641809303], 0.5, {"g1": "X", "g3": "X"})
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11] == "# curve:\t3" and "\n".join(lines[:11] + lines[12:]) == before          # the gene table gains only the header line
    abundance.write_curve(out + ".curve.tsv", ARGS, t)
    lines = open(out + ".curve.tsv").read().split("\n")
    assert lines[:12] == TODAY + ["# curve:\t3"]
    assert lines[12] == "sampled_reads\taverage_genome_size\tgenome_equivalents_sampled\treads_assigned\tgenes_with_reads\tgenes_detected\tgroups_with_reads"
    assert lines[13] == "2891\tNA\tNA\t1\t1\t0\t1"                                                                   # a point without an estimate
    assert lines[14] == "5782\t3100000.0\t%r\t5\t2\t0\t1" % (5782 * 100 / 3.1e6)
    assert lines[15] == "8672\t3051745.7641809303\t%r\t12\t2\t1\t1" % t["genome_equivalents_sampled"] and lines[16:] == [""]
    assert np.isnan(t["curve"]["rpkg"][0]).all() and not np.isnan(t["curve"]["rpkg"][1:]).any() and t["curve"]["genome_equivalents_sampled"][0] is None
    abundance.write_curve_genes(out + ".genes.tsv", t)
    assert open(out + ".genes.tsv").read() == ("# curve_points:\t2891\t5782\t8672\n"
                                               "gene\treads_1\treads_2\treads_3\tcovered_aa_1\tcovered_aa_2\tcovered_aa_3\n"
                                               "g1\t1\t3\t5\t30\t55\t60\ng2\t0\t0\t0\t0\t0\t0\ng3\t0\t2\t7\t0\t60\t100\n")
    t["curve"] = abundance.curve_figures(NAMES, LENGTH, 100, points, READS, ALIGNED, None, [3.0e6] * 3)
    abundance.write_curve(out + ".curve.tsv", ARGS, t)
    abundance.write_curve_genes(out + ".genes.tsv", t)
    assert open(out + ".curve.tsv").read().split("\n")[12:14] == ["sampled_reads\taverage_genome_size\tgenome_equivalents_sampled\treads_assigned\tgenes_with_reads",
                                                                 "2891\t3000000.0\t%r\t1\t1" % (2891 * 100 / 3.0e6)]
    assert open(out + ".genes.tsv").read().split("\n")[1:3] == ["gene\treads_1\treads_2\treads_3", "g1\t1\t3\t5"]


def test_files_without_the_switch_are_todays(tmp_path):
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11] == "gene\tlength_aa\treads\taligned_aa\trpkg" and lines[13] == "g2\t300\t0\t0\t0.0" and lines[15:] == [""]
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    lines = open(out + ".groups.tsv").read().split("\n")
    assert lines[:11] == TODAY and lines[11:13] == ["# groups:\tmap.tsv", "group\tgenes\treads\trpkg"] and len(lines) == 16
    assert not any("curve" in l for l in abundance.header_lines(ARGS, t))


# ---- refusals, before any engine is opened ----------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", boom)
    monkeypatch.setattr(microbe_census, "run_pipeline", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_refusals(tmp_path, no_engine):
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    faa = tmp_path / "good.faa"
    faa.write_text(">g1 d\n%s\n>g2 d\n%s\n" % ("MKV" * 20, "MLA" * 30))
    (tmp_path / "map.tsv").write_text("g1\tX\n")
    out = str(tmp_path / "out.tsv")

    def request(**kw):
        args = {"seqfiles": [fq], "genes": str(faa), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    for bad, shown in ((0, "0"), (-1, "-1"), (65, "65"), (2.0, "2\\.0"), (2.5, "2\\.5"), ("ten", "ten"), (True, "True"), (False, "False")):
        with pytest.raises(abundance.AbundanceError, match="--curve %s is not an integer from 1 to 64" % shown):
            abundance.run_abundance(request(curve=bad))
    with pytest.raises(abundance.AbundanceError, match="--curve-genes '' is an empty path"):
        abundance.run_abundance(request(curve=4, curve_genes=""))
    with pytest.raises(abundance.AbundanceError, match="--curve-genes .*m.tsv needs --curve K"):
        abundance.run_abundance(request(curve_genes=str(tmp_path / "m.tsv")))
    for same, what in ((out, "the gene table itself"), (os.path.join(str(tmp_path), ".", "out.tsv"), "the gene table itself"), (out + ".curve.tsv", "the curve table"),
                       (out + ".groups.tsv", "the groups table"), (str(tmp_path / "d.tsv"), "the depth file")):
        with pytest.raises(abundance.AbundanceError, match="--curve-genes .* is the path of %s" % what):
            abundance.run_abundance(request(curve=4, curve_genes=same, groups=str(tmp_path / "map.tsv"), depth_out=str(tmp_path / "d.tsv")))
    assert not os.path.exists(out)
    # off by default; 1 and 64 are taken; <outfile>.groups.tsv is no other file without --groups
    a = request()
    abundance.check_request(a)
    assert (a["curve"], a["curve_genes"], a["coverage"]) == (None, None, False)
    for K in (1, 64, np.int64(7)):
        a = request(curve=K, curve_genes=out + ".groups.tsv")
        abundance.check_request(a)
        assert a["curve"] == int(K) and type(a["curve"]) is int and a["coverage"] is False          # (the curve implies nothing else)
    with pytest.raises(AssertionError, match="GPU work was started"):          # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(curve=10, curve_genes=str(tmp_path / "m.tsv"), min_breadth=0.5))


def test_cli_switches():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])
    assert (a["curve"], a["curve_genes"]) == (None, None)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--curve", "10", "--curve-genes", "m.tsv"])
    assert (a["curve"], a["curve_genes"]) == (10, "m.tsv")
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--curve", "ten"])


def test_curve_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_set_curve", "mc_curve_read", "mc_curve_k", "mc_curve_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("set_curve", "curve", "curve_ms"):
        assert callable(getattr(_native.Engine, m))
    assert abundance.MAX_CURVE == oc.define("MC_CURVE_MAXK", "mc_curve.h") == 64


def test_a_sample_without_reads_is_an_error_with_the_switch_too(tmp_path, monkeypatch):
    """--curve K on a sample of which the sampler takes no read: no search, no curve - and no silent table either: the run ends with the
    error it ends with without the switch, before any file is written."""
    class NoReads:
        def __init__(self, *a, **k):
            self.read_len = a[1]

        def run(self):
            return 0

        def stats(self):
            return {"sampled": 0}

        def close(self):
            pass

    class Idle:
        def __init__(self, **k):
            self.names = k["names"]

        def abundance(self):
            z = np.zeros(len(self.names), np.int64)
            return {"reads": z, "aligned": z, "searched": 0, "assigned": 0}

        def coverage(self):
            z = np.zeros(len(self.names), np.int64)
            return {"covered": z, "spanned": z, "max_depth": z}

        def stats(self):
            return {"ms_total": 0.0}

        def coverage_ms(self):
            return 0.0

        def abundance_ms(self):
            return 0.0

        def search_files(self, *a, **k):
            pass

        def set_curve(self, points):
            raise AssertionError("points of a sample without reads")

        def set_run(self, *a, **k):
            pass

        set_abundance = set_coverage = set_run
        close = set_run
    monkeypatch.setattr(_native, "Reader", NoReads)
    monkeypatch.setattr(_native, "Engine", Idle)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    faa = tmp_path / "good.faa"
    faa.write_text(">g1 d\n%s\n>g2 d\n%s\n" % ("MKV" * 20, "MLA" * 30))
    out = str(tmp_path / "out.tsv")
    for kw in (dict(curve=4, curve_genes=str(tmp_path / "m.tsv"), coverage=True), dict()):
        with pytest.raises(abundance.AbundanceError, match="No reads remaining after filtering"):
            abundance.run_abundance(dict({"seqfiles": [os.path.join(GOLD, "inputs", "example.fq.gz")], "genes": str(faa), "outfile": out, "nreads": 100, "ags": 3.0e6}, **kw))
    assert os.listdir(str(tmp_path)) == ["good.faa"]
