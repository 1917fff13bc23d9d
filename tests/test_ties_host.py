"""The tie accounting, host side (no GPU): the restatement of csrc/k_ties.h's statement (tests/ties_restated.py) on hand-computed cases and
on the reference binary's m8 goldens - with the conditions that keep the GPU tests from passing empty - the statement's invariants on
every golden under the three cut-off sets of test_gpu_abundance.py, the walk of csrc/mc_ties.h itself compiled by g++ (tests/emul/ties.cpp,
once more under -fsanitize=address,undefined) on the cases the device runs, the new columns and header lines of abundance.py, the
refusals, the unchanged files without the switch, and the four new symbols of the ABI."""
import collections
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import abundance_restated as R
import coverage_restated as V
import order_cases as oc
import ties_cases as tc
import ties_restated as T
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
ONE = 1 << 32
CUTS = [dict(), dict(min_ident=60, min_aln=30), dict(min_bits=27.1)]           # test_gpu_abundance.py's three


# ---- the restatement against answers worked out by hand ---------------------------------------------------------------------------------
def test_restatement_on_hand_computed_cases():
    c = tc.basics()
    rows = V.rows_from_array(c["rows"])
    t = T.ties(rows, c["lengths"], c["group_of"], c["ngroups"])
    sets = {q: [m[0] for m in members] for q, members in t["sets"]}
    assert sets == {0: [0], 1: [0, 2], 2: [2, 3, 5], 3: [0, 2, 3, 4, 5, 6], 4: [7, 0, 2, 3, 4, 5, 6], 5: [0, 1], 6: [5, 3], 7: [2, 3], 8: [4], 10: [1, 0], 11: [6, 7],
                    12: [0], 13: [4, 5]}                              # (read 9 adds nothing: its first-rule subject is nseq)
    assert dict(t["sets"])[5] == [(0, 0, 4), (1, 0, 0)] and dict(t["sets"])[6] == [(5, 0, 9), (3, 20, 29)]     # representative rows: the first of each subject
    # by hand: candidates per gene = the sets that hold it; unique = the sets of one
    assert t["candidates"].tolist() == [7, 2, 5, 5, 4, 5, 3, 2] and t["unique"].tolist() == [2, 0, 0, 0, 1, 0, 0, 0] and t["ambiguous"] == 10
    third, sixth, seventh, half = ONE // 3, ONE // 6, ONE // 7, ONE // 2
    assert (third, ONE - 3 * third, ONE - 6 * sixth, ONE - 7 * seventh) == (1431655765, 1, 4, 4)
    want = [0] * 8
    for q, s in sets.items():
        each = ONE // len(s)
        for g in s:
            want[g] += each
        want[s[0]] += ONE - each * len(s)
    assert t["share"].tolist() == want
    assert int(t["share"][7]) == seventh + 4 + half and int(t["share"][1]) == 2 * half                      # gene 7: first of read 4, second of read 11
    assert sum(want) == 13 * ONE
    # groups 0 0 1 1 2 2 3 3: reads 0, 5, 10, 12 lie in group 0, read 7 in group 1, reads 8 and 13 in group 2, read 11 in group 3
    assert t["group_unique"].tolist() == [4, 1, 2, 1] and t["group_ambiguous"] == 5
    # the any-depth: gene 1 (one residue) twice; gene 5's span 10 .. 25 of read 13 lies outside its 20 residues and marks nothing
    assert t["covered_any"][1] == 1 and t["max_depth_any"][1] == 2 and t["spanned_any"][5] == 18 + 6 + 6 + 10
    assert t["depth_any"][29] == 2 and t["depth_any"][31 + 39] == 1         # spans ending at len - 1: reads 0 and 10 on gene 0, read 1 on gene 2
    ab = R.abundance(R.rows_from_array(c["rows"]), 32768)
    cv = V.coverage(rows, c["lengths"])
    assert int(ab["reads"][:8].sum()) == 13 and T.invariants(t, ab["reads"][:8], 13, c["group_of"], cv["depth"]) == []
    # under the cut-offs: read 7's tied row fails min_ident (k = 1), read 8's top row fails (T falls to 50: genes 5 and 6), read 12 is lost
    cut = T.ties(rows, c["lengths"], c["group_of"], c["ngroups"], **tc.CUT)
    cs = {q: [m[0] for m in members] for q, members in cut["sets"]}
    assert cs[7] == [2] and cs[8] == [5, 6] and 12 not in cs and len(cs) == 12 and cut["ambiguous"] == 10 and cut["group_ambiguous"] == 6
    # row order does not matter for the set: the same read with its rows reversed has the same tied set, another first subject
    rev = T.ties([r for r in reversed(rows) if r[0] == 4], c["lengths"])
    assert sorted(m[0] for m in rev["sets"][0][1]) == sorted(sets[4]) and rev["sets"][0][1][0][0] == 6 and int(rev["share"][6]) == seventh + 4
    # no map: the group counters are empty and zero
    none = T.ties(rows, c["lengths"])
    assert len(none["group_unique"]) == 0 and none["group_ambiguous"] == 0 and np.array_equal(none["share"], t["share"])


# ---- the reference binary's goldens ---------------------------------------------------------------------------------------------------
MARKER_GOLDENS = ("unittest_metagenome", "c2_100bp", "training_library_a", "config1_example_fq")
_golden = {}


def golden(case):
    """(rows, lengths) of a golden - parsed once, shared, never changed"""
    if case not in _golden:
        if case == "generic_db":
            sys.path.insert(0, GOLD)
            import make_generic_db_golden as G
            from microbecensus_amd import synth
            names, seqs = synth.random_proteins(G.CASE["db_residues"], seed=G.CASE["db_seed"])
        else:
            names, seqs = _native.load_markers()
        _golden[case] = (V.rows_from_m8(os.path.join(GOLD, case + ".m8.gz"), names), [len(s) for s in seqs])
    return _golden[case]


def _tied_rows(rows):
    """per read: (the subjects of the rows that have the read's top score, whether the first row has it) - no cut-offs"""
    by = {}
    for r in rows:
        by.setdefault(r[0], []).append(r)
    out = []
    for rs in by.values():
        top = max(r[4] for r in rs)
        out.append(([r[1] for r in rs if r[4] == top], rs[0][4] == top))
    return out


def test_goldens_hold_the_ties_the_gpu_tests_rest_on():
    """The conditions without which the GPU tests could pass empty.  (In generic_db the four reads that tie with the SAME subject twice
    are reads of k = 1 - two tied rows, one subject - and so not among the 22 ambiguous ones: they are what a count of tied ROWS would
    get wrong, and the test asserts exactly that.)"""
    rows, lengths = golden("config1_example_fq")
    t = T.ties(rows, lengths)
    assert len(t["k"]) == 251 and t["ambiguous"] == 57 and max(t["k"]) == 6
    assert sorted(collections.Counter(t["k"]).items()) == [(1, 194), (2, 32), (3, 17), (4, 4), (5, 2), (6, 2)]
    rows, lengths = golden("generic_db")
    t = T.ties(rows, lengths)
    assert len(t["k"]) == 10502 and t["ambiguous"] == 22 and sorted(collections.Counter(t["k"]).items()) == [(1, 10480), (2, 21), (3, 1)]
    tied = _tied_rows(rows)
    repeated = [subs for subs, _ in tied if len(subs) != len(set(subs))]
    assert len(repeated) >= 4 and all(len(set(subs)) == 1 for subs in repeated)
    assert sum(1 for _, first in tied if not first) >= 300
    for case, reads, amb, largest in (("unittest_metagenome", 3273, 643, 28), ("c2_100bp", 1200, 207, None), ("training_library_a", 1006, 183, None)):
        rows, lengths = golden(case)
        t = T.ties(rows, lengths)
        assert (len(t["k"]), t["ambiguous"]) == (reads, amb) and (largest is None or max(t["k"]) == largest), case


@pytest.mark.parametrize("case", MARKER_GOLDENS + ("generic_db",))
def test_invariants_on_every_golden_under_the_three_cutoff_sets(case):
    rows, lengths = golden(case)
    nseq = len(lengths)
    group_of = np.arange(nseq) % 97                                   # (any map will do for the invariants)
    seen = []
    for cut in CUTS:
        t = T.ties(rows, lengths, group_of, 97, **cut)
        ab = R.abundance([r[:6] for r in rows], nseq, **cut)
        cv = V.coverage(rows, lengths, **cut)
        assert T.invariants(t, ab["reads"], ab["assigned"], group_of, cv["depth"]) == [], (case, cut)
        assert len(t["sets"]) == ab["assigned"] and all(ab["reads"][m[0][0]] > 0 for _, m in t["sets"])      # the first tied subject is the one the read is assigned to
        assert np.array_equal(np.bincount([m[0][0] for _, m in t["sets"]], minlength=nseq), ab["reads"])
        assert (t["covered_any"] >= cv["covered"]).all() and ((t["candidates"] > 0) == (t["covered_any"] > 0)).all()
        seen.append(ab["assigned"])
    assert seen[0] > seen[1] > 0 and seen[0] >= seen[2] > 0            # (the cut-offs cut, and leave something)


# ---- the walk of mc_ties.h on the CPU ---------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "ties")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(HERE, "emul", "ties.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "ties", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "ties_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _walk(exe, name, c, tmp):
    oc.write_sections(tmp / (name + ".in"), tc.sections_in(c))
    p = subprocess.run([exe, "run", str(tmp / (name + ".in")), str(tmp / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    err = p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    out = oc.read_sections(tmp / (name + ".out"))
    assert len(out) == 4
    return tc.check_ties(c, tc.expected(name, c), np.frombuffer(out[0], "<u8"), np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<u8"), np.frombuffer(out[3], "<u4"))


def cpu_cases():
    """the cases of test_gpu_ties_units.py (the 100,000 reads at 20,000: the sums past 2^32 are there all the same)"""
    cases = {"basics": tc.basics(), "basics_cut": tc.basics(cut=tc.CUT), "basics_no_map": tc.basics(groups=False), "basics_no_cov": tc.basics(cov=False),
             "basics_counts_only": tc.basics(groups=False, cov=False, cut=tc.CUT), "boundaries": tc.boundaries(), "long_span": tc.long_span(), "wide_500": tc.wide(1, 500), "wide_250_twice": tc.wide(64, 250),
             "many": tc.many(20_000)}
    for n in (1, 256, 257):
        cases["rows%d" % n] = tc.row_counts(n)
    return cases


def test_the_walk_of_the_header_on_the_cpu(driver, driver_san, tmp_path):
    for name, c in cpu_cases().items():
        got = _walk(driver, name, c, tmp_path)
        san = _walk(driver_san, name, c, tmp_path)
        assert all(np.array_equal(got[k], san[k]) for k in got), name
    t = tc.expected("wide_500", None)[0]
    assert t["k"] == [500] and int(t["share"][0]) == ONE // 500 + ONE % 500 and set(t["share"][1:].tolist()) == {ONE // 500}
    t = tc.expected("wide_250_twice", None)[0]
    assert t["k"] == [250] * 64 and t["candidates"].tolist() == [64] * 250 and t["max_depth_any"].tolist() == [64] * 250
    t = tc.expected("many", None)[0]
    assert t["share"].tolist() == [0, 20_000 * (ONE // 2), 20_000 * (ONE // 2)] and t["group_unique"].tolist() == [0, 20_000]
    t = tc.expected("long_span", None)[0]
    assert dict(t["sets"])[1] == [(0, 3, 13), (1, 3, 13), (2, 0, 10), (3, 1, 11), (4, 2, 12), (5, 3, 13)] and t["k"] == [2, 6, 1]
    t = tc.expected("boundaries", None)[0]
    assert dict(t["sets"])[250] == [(0, 2, 22), (1, 5, 25), (3, 10, 30)] and dict(t["sets"])[500] == [(1, 0, 9), (3, 5, 39)] and dict(t["sets"])[501] == [(3, 39, 39)]


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def _table():
    ge = abundance.genome_equivalents(8672, 100, 3051745.7641809303)
    reads, length = np.array([5, 0, 7], np.int64), np.array([120, 300, 2047], np.int64)
    return {"gene": ["g1", "g2", "g3"], "length_aa": length, "reads": reads, "aligned_aa": np.array([150, 0, 231], np.int64), "rpkg": abundance.rpkg(reads, length, ge),
            "sampled_reads": 8672, "trimmed_length": 100, "ags": 3051745.7641809303, "ags_source": "run_pipeline", "genome_equivalents_sampled": ge, "reads_assigned": 12}


ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": "map.tsv"}
TODAY = ["# metagenome:\ta.fq.gz", "# genes:\tgenes.faa", "# sampled_reads:\t8672", "# trimmed_length:\t100", "# min_ident:\t60", "# min_aln:\t30", "# min_bits:\t35.5",
         "# average_genome_size:\t3051745.7641809303", "# ags_source:\trun_pipeline", "# genome_equivalents_sampled:\t%r" % (8672 * 100 / 3051745.7641809303),
         "# reads_assigned:\t12"]


def test_tables_with_ties(tmp_path):
    t = _table()
    out = str(tmp_path / "plain.tsv")
    abundance.write_table(out, ARGS, t)
    plain = open(out).read().split("\n")
    # 12 reads: 3 + 6 unique; three reads tied over all three genes (two of them given to g1 first, one to g2: the remainders of 1)
    third = ONE // 3
    share = np.array([3 * ONE + 3 * third + 2, 3 * third + 1, 6 * ONE + 3 * third], np.uint64)
    sh = abundance.shared_reads(share)
    assert sh.tolist() == [float(np.float64(v) / 4294967296.0) for v in share] and sh.dtype == np.float64 and int(share.sum()) == 12 * ONE
    t.update({"unique_reads": np.array([3, 0, 6], np.int64), "candidate_reads": np.array([6, 3, 9], np.int64), "shared_reads": sh,
              "rpkg_shared": abundance.rpkg(sh, t["length_aa"], t["genome_equivalents_sampled"]), "reads_ambiguous": 3})
    out = str(tmp_path / "ties.tsv")
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11:13] == ["# ties:\ton", "# reads_ambiguous:\t3"]
    assert lines[13] == "gene\tlength_aa\treads\taligned_aa\trpkg\tunique_reads\tcandidate_reads\tshared_reads\trpkg_shared"
    assert [l.split("\t")[:5] for l in lines[14:17]] == [l.split("\t") for l in plain[12:15]]           # the existing columns: byte for byte
    assert lines[14].split("\t")[5:] == ["3", "6", repr(float(sh[0])), repr(float(sh[0]) / (3 * 120 / 1000.0) / t["genome_equivalents_sampled"])]
    assert lines[15].split("\t")[5:] == ["0", "3", repr(float(sh[1])), repr(float(t["rpkg_shared"][1]))] and lines[17:] == [""]
    # with coverage and min_breadth: behind ALL existing columns
    covered, spanned = np.array([60, 0, 100], np.int64), np.array([150, 0, 231], np.int64)
    breadth, mean_depth = abundance.coverage_columns(t["length_aa"], covered, spanned)
    t.update({"covered_aa": covered, "breadth": breadth, "mean_depth": mean_depth, "max_depth": np.array([4, 0, 7], np.int64), "min_breadth": 0.5,
              "detected": abundance.detect(t["reads"], covered, t["length_aa"], 0.5)})
    cany = np.array([90, 150, 100], np.int64)
    t.update({"covered_any_aa": cany, "breadth_any": abundance.coverage_columns(t["length_aa"], cany, cany)[0],
              "detected_any": abundance.detect(t["candidate_reads"], cany, t["length_aa"], 0.5)})
    assert t["detected"].tolist() == [1, 0, 0] and t["detected_any"].tolist() == [1, 1, 0]              # 150 of 300 at F = 0.5 is detected
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[11:16] == ["# coverage:\ton", "# min_breadth:\t0.5", "# genes_detected:\t1", "# ties:\ton", "# reads_ambiguous:\t3"]
    assert lines[16] == ("gene\tlength_aa\treads\taligned_aa\trpkg\tcovered_aa\tbreadth\tmean_depth\tmax_depth\tdetected\tunique_reads\tcandidate_reads\tshared_reads\trpkg_shared"
                         "\tcovered_any_aa\tbreadth_any\tdetected_any")
    assert lines[17].split("\t")[9:] == ["1", "3", "6", repr(float(sh[0])), repr(float(t["rpkg_shared"][0])), "90", "0.75", "1"]
    assert lines[18].split("\t")[9:] == ["0", "0", "3", repr(float(sh[1])), repr(float(t["rpkg_shared"][1])), "150", "0.5", "1"]
    # the groups: g1 and g3 in X, g2 alone.  unique_reads of X is the device's group_unique - NOT 3 + 6
    ids, gnames = abundance.group_ids(t["gene"], {"g1": "X", "g3": "X"})
    assert ids.tolist() == [0, 1, 0] and ids.dtype == np.int32 and gnames == ["X", "g2"]
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"}, t["detected"])
    assert [g[0] for g in t["groups"]] == gnames                      # numbered in the order group_table lists them
    t["reads_ambiguous_across_groups"] = 3
    t["groups_ties"] = abundance.group_ties_table(ids, 2, np.array([9, 0], np.int64), share, t["rpkg_shared"], t["detected_any"])
    x_share = (int(share[0]) + int(share[2])) / 4294967296.0
    assert t["groups_ties"] == [(9, x_share, float(t["rpkg_shared"][0]) + float(t["rpkg_shared"][2]), 1), (0, float(sh[1]), float(t["rpkg_shared"][1]), 1)]
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    lines = open(out + ".groups.tsv").read().split("\n")
    assert lines[14:18] == ["# ties:\ton", "# reads_ambiguous:\t3", "# reads_ambiguous_across_groups:\t3", "# groups:\tmap.tsv"]
    assert lines[18] == "group\tgenes\treads\trpkg\tgenes_detected\tunique_reads\tshared_reads\trpkg_shared\tgenes_detected_any"
    assert lines[19] == "X\t2\t12\t%r\t1\t9\t%r\t%r\t1" % (float(t["rpkg"][0]) + float(t["rpkg"][2]), x_share, float(t["rpkg_shared"][0]) + float(t["rpkg_shared"][2]))
    assert lines[20] == "g2\t1\t0\t0.0\t0\t0\t%r\t%r\t1" % (float(sh[1]), float(t["rpkg_shared"][1])) and lines[21:] == [""]
    # without min_breadth the groups table has no genes_detected_any; without ties it is today's
    del t["detected_any"], t["detected"]
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    t["groups_ties"] = abundance.group_ties_table(ids, 2, np.array([9, 0], np.int64), share, t["rpkg_shared"])
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    assert open(out + ".groups.tsv").read().split("\n")[16] == "group\tgenes\treads\trpkg\tunique_reads\tshared_reads\trpkg_shared"


def test_tables_without_the_switch_are_todays(tmp_path):
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11] == "gene\tlength_aa\treads\taligned_aa\trpkg"
    assert lines[12] == "g1\t120\t5\t150\t%r" % (5 / (3 * 120 / 1000.0) / t["genome_equivalents_sampled"]) and lines[13] == "g2\t300\t0\t0\t0.0" and lines[15:] == [""]
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    lines = open(out + ".groups.tsv").read().split("\n")
    assert lines[:11] == TODAY and lines[11:13] == ["# groups:\tmap.tsv", "group\tgenes\treads\trpkg"]
    assert lines[13:] == ["X\t2\t12\t%r" % (float(t["rpkg"][0]) + float(t["rpkg"][2])), "g2\t1\t0\t0.0", ""]


# ---- refusals, before any engine is opened ----------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", boom)
    monkeypatch.setattr(microbe_census, "run_pipeline", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_refusals_and_the_default(tmp_path, no_engine, monkeypatch):
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    faa = tmp_path / "good.faa"
    faa.write_text(">g1 d\n%s\n>g2 d\n%s\n" % ("MKV" * 20, "MLA" * 30))

    def request(**kw):
        args = {"seqfiles": [fq], "genes": str(faa), "outfile": str(tmp_path / "out.tsv"), "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    a = request()
    abundance.check_request(a)
    assert a["ties"] is False                                        # off by default
    for on in (True, 1):
        a = request(ties=on)
        abundance.check_request(a)
        assert a["ties"] is True and a["coverage"] is False          # ties does not imply coverage
    for bad in ("yes", 2, None, 0.5):
        with pytest.raises(abundance.AbundanceError, match="ties .* is not a switch"):
            abundance.run_abundance(request(ties=bad))
    with pytest.raises(abundance.AbundanceError, match="not computed by a distributed run"):      # ties in a distributed run stay refused
        abundance.run_abundance(request(ties=True, distributed=True))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(abundance.AbundanceError, match="not computed by a distributed run"):
        abundance.run_abundance(request(ties=True))
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(AssertionError, match="GPU work was started"):  # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(ties=True, min_breadth=0.5))
    assert not os.path.exists(str(tmp_path / "out.tsv"))


def test_cli_switch():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])["ties"] is False
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--ties", "--min-breadth", "0.1", "--groups", "m.tsv"])
    assert (a["ties"], a["min_breadth"], a["groups"], a["coverage"]) == (True, 0.1, "m.tsv", False)


def test_ties_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import re
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_set_ties", "mc_ties_read", "mc_ties_coverage_read", "mc_ties_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("set_ties", "ties", "ties_coverage", "ties_ms"):
        assert callable(getattr(_native.Engine, m))
