"""The bootstrap of the groups table, host side (no GPU): the rules of csrc/mc_groupboot.h compiled by g++ (tests/emul/groupboot.cpp, once
more under -fsanitize=address,undefined) against the numpy restatement (tests/groupboot_restated.py) on the cases the device harness runs
(tests/groupboot_cases.py) - values and six doubles bit for bit, counts and the plan as exact integers; that the restatement's addition
order is under test; the host part in abundance.py against numpy.std and numpy.percentile for every number of used replicates from 1 to 200;
the two consequences of the rule - a singleton group's interval is its gene's bit for bit, and a group's standard error never exceeds the
sum of its members'; every refusal of the front end before an engine is opened; the groups table with and without the switch; and the
new symbols of the ABI."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import geneboot_restated as GR
import groupboot_cases as grc
import groupboot_restated as GRR
import order_cases as oc
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
CASES = {c["name"]: c for c in grc.cases()}


# ---- the rules of mc_groupboot.h on the CPU -----------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "groupboot")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(HERE, "emul", "groupboot.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "groupboot", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "groupboot_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _run(exe, c, tmp):
    e = grc.expect(c)
    arrays = [np.int32([c["nseq"], c["B"], c["ngroups"]]), e["counts"].astype(np.uint64), c["scale"], c["group_of"], c["gene_kb"], e["reads"].astype(np.uint64)]
    oc.write_sections(tmp / (c["name"] + ".in"), arrays)
    p = subprocess.run([exe, "run", str(tmp / (c["name"] + ".in")), str(tmp / (c["name"] + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and not p.stderr, (c["name"], p.returncode, p.stderr.decode())
    return oc.read_sections(tmp / (c["name"] + ".out"))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rules_of_mc_groupboot_h_on_the_device_cases(which, driver, driver_san, tmp_path):
    exe = driver if which == "plain" else driver_san
    for c in grc.cases():
        o = _run(exe, c, tmp_path)
        e = grc.compare(c, np.frombuffer(o[0], "<f8"), np.frombuffer(o[1], "<u8").astype(np.int64), np.frombuffer(o[2], "<f8"))
        gidx, start, member, kb = e["plan"]
        assert int(np.frombuffer(o[3], "<i4")[0]) == len(e["live"]) and np.array_equal(np.frombuffer(o[4], "<i4"), gidx), c["name"]
        assert np.array_equal(np.frombuffer(o[5], "<u4"), start) and np.array_equal(np.frombuffer(o[6], "<u4"), member) and GR.same_bits(np.frombuffer(o[7], "<f8"), kb), c["name"]
    assert len(grc.cases()) >= 15


def test_cases_reach_what_they_are_for():
    """the conditions of the cases, from the restatement alone: without them the device tests could pass empty"""
    assert [CASES["grp_b%d" % B]["B"] for B in grc.BS] == [1, 63, 64, 65, 257, 4096]
    has = lambda c: grc.expect(c)["reads"] > 0
    one = CASES["grp_one_group"]
    assert one["ngroups"] == 1 and has(one).sum() == 4 and not has(one).all()
    sg = CASES["grp_singletons"]
    assert sg["ngroups"] == sg["nseq"] == 5 and np.array_equal(sg["group_of"], np.arange(5)) and not has(sg)[1]
    il = CASES["grp_interleave"]
    assert il["group_of"].tolist() == [0, 1, 0, 1, 0, 1] and has(il).all()
    eb = CASES["grp_empty_between"]
    assert grc.expect(eb)["plan"][0].tolist() == [0, -1, 1]
    of = CASES["grp_one_of_five"]
    assert has(of)[of["group_of"] == 0].tolist() == [False, False, True, False, False] and grc.expect(of)["plan"][2].tolist() == [0, 1]
    sv = CASES["grp_seventy"]
    assert int((has(sv) & (sv["group_of"] == 0)).sum()) == 70 > 64 and np.diff(grc.expect(sv)["plan"][1]).tolist() == [70, 5]
    assert grc.expect(CASES["grp_m_none"])["m"] == 0 and grc.expect(CASES["grp_m_one"])["m"] == 1
    holes = CASES["grp_b65"]["scale"]
    assert np.isnan(holes).any() and (holes == 0).any() and (holes < 0).any() and np.isinf(holes).any() and 0 < grc.expect(CASES["grp_b65"])["m"] < 65
    km = CASES["grp_kb_mixed"]
    assert km["gene_kb"][0] == 0.003 and km["gene_kb"][1] == 196.605 and km["ngroups"] == 1 and has(km).all()
    assert {c["counts_first"] for c in grc.cases()} == {True, False}
    for c in grc.cases():               # an unused replicate's value is 0.0, its count is counted all the same
        e = grc.expect(c)
        unused = ~GR.used(c["scale"])
        assert not e["y"][:, unused].any() and (not unused.any() or e["C"][:, unused].any())


def test_the_addition_order_is_under_test():
    """the members of the mixed-gene_kb group added in descending gene index give other bits in at least one replicate, and the same counts"""
    c = CASES["grp_kb_mixed"]
    e = grc.expect(c)
    y, C = GRR.values(e["counts"], c["scale"], c["group_of"], c["ngroups"], c["gene_kb"], reverse=True)
    assert np.array_equal(C, e["C"])
    assert (y.view(np.uint64) != e["y"].view(np.uint64)).any()
    assert np.allclose(y, e["y"], rtol=1e-14, atol=0.0)


# ---- the host part: standard error and interval from the six doubles ---------------------------------------------------------------------
def test_columns_are_numpy_std_and_percentile_for_every_m():
    """m = 1 .. 200 used replicates (of m + 3: three are unused), two groups of two and three genes: group_boot_columns gives
    numpy.percentile(y, [2.5, 97.5]) exactly and numpy.std(y, ddof=1) within a relative 1e-12, y the restated group values"""
    rng = np.random.default_rng(26)
    length = np.array([7, 120, 2047, 65535, 301], np.int64)
    group_of = np.array([0, 1, 0, 1, 1], np.int32)
    for m in range(1, 201):
        for ties in (False, True):
            B = m + 3
            scale = rng.uniform(1e-3, 1e-2, B) if not ties else np.full(B, 0.015625)
            scale[[0, B // 2, B - 1]] = [np.nan, 0.0, -1.0]
            c = rng.integers(0, 5 if ties else 4000, (5, B))
            use = GR.used(scale)
            assert int(use.sum()) == m
            y, _ = GRR.values(c, scale, group_of, 2, grc.gene_kb(length))
            se, lo, hi = abundance.group_boot_columns(GRR.stats(y, scale), m)
            for G in range(2):
                want = np.percentile(y[G][use], [2.5, 97.5])
                assert lo[G] == want[0] and hi[G] == want[1], (m, ties, G)
                if m > 1:
                    assert se[G] == pytest.approx(np.std(y[G][use], ddof=1), rel=1e-12, abs=1e-300), (m, ties, G)
                else:
                    assert np.isnan(se[G])
    se, lo, hi = abundance.group_boot_columns(np.full((2, 6), np.nan), 0)
    assert np.isnan(se).all() and np.isnan(lo).all() and np.isnan(hi).all()


def test_singleton_groups_and_the_triangle_inequality():
    """On every case: a group with one member has its gene's interval bit for bit and its standard error within a relative 1e-12 (the
    squares are taken after the division by gene_kb, not before); no group's standard error exceeds the sum of its members' (the standard
    deviation obeys the triangle inequality; a relative 1e-9 for rounding)."""
    singles = bound = 0
    for c in grc.cases():
        e = grc.expect(c)
        m = e["m"]
        gse, glo, ghi = abundance.boot_columns(e["stats"], m, c["length_aa"])
        se, lo, hi = abundance.group_boot_columns(e["gstats"], m)
        for G in range(c["ngroups"]):
            members = np.flatnonzero(c["group_of"] == G)
            if len(members) == 1:
                s = members[0]
                assert GR.same_bits(lo[G], glo[s]) and GR.same_bits(hi[G], ghi[s]), (c["name"], G)
                assert m < 2 or se[G] == pytest.approx(gse[s], rel=1e-12, abs=0.0), (c["name"], G)
                singles += 1
            if m >= 2:
                assert se[G] <= gse[members].sum() * (1.0 + 1e-9), (c["name"], G, se[G], gse[members].sum())
                bound += len(members) > 1 and se[G] > 0
    assert singles >= 5 and bound >= 15


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
NAMES = ["g1", "g2", "g3"]
LENGTH = np.array([120, 300, 2047], np.int64)
READS = np.array([5, 0, 7], np.int64)
ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": "map.tsv"}


def test_groups_table_with_and_without_the_switch(tmp_path):
    ge = abundance.genome_equivalents(8672, 100, 3051745.7641809303)
    t = {"gene": list(NAMES), "length_aa": LENGTH, "reads": READS, "aligned_aa": np.array([150, 0, 231], np.int64), "rpkg": abundance.rpkg(READS, LENGTH, ge),
         "sampled_reads": 8672, "trimmed_length": 100, "ags": 3051745.7641809303, "ags_source": "run_pipeline", "genome_equivalents_sampled": ge, "reads_assigned": 12}
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    out = str(tmp_path / "out.groups.tsv")
    abundance.write_groups(out, ARGS, t)
    before = open(out).read()
    lines = before.split("\n")
    assert lines[11] == "# groups:\tmap.tsv" and lines[12] == "group\tgenes\treads\trpkg" and [l.split("\t")[:3] for l in lines[13:15]] == [["X", "2", "12"], ["g2", "1", "0"]] and lines[15:] == [""]
    # the gene bootstrap alone: the groups table is what it was
    t.update({"rpkg_boot_se": np.array([0.25, 0.0, 0.125]), "rpkg_ci95_low": np.array([1.5, 0.0, 0.5]), "rpkg_ci95_high": np.array([2.5, 0.0, np.nan]), "boot_used": 97,
              "bootstrap": 100, "bootstrap_seed": 5, "bootstrap_denominator": "replicate_ags"})
    abundance.write_groups(out, ARGS, t)
    assert open(out).read() == before
    abundance.write_table(str(tmp_path / "out.tsv"), ARGS, t)
    gene_before = open(str(tmp_path / "out.tsv")).read()
    # with the switch: five header lines behind the existing ones, three columns behind the existing ones
    t["groups_boot"] = [(0.5, 1.25, 4.0), (0.0, 0.0, 0.0)]
    abundance.write_groups(out, ARGS, t)
    after = open(out).read().split("\n")
    assert after[:12] == lines[:12]
    assert after[12:17] == ["# bootstrap:\t100", "# bootstrap_seed:\t5", "# bootstrap_replicates:\t97/100", "# bootstrap_denominator:\treplicate_ags", "# bootstrap_groups:\ton"]
    assert after[17] == lines[12] + "\trpkg_boot_se\trpkg_ci95_low\trpkg_ci95_high"
    assert [l.rsplit("\t", 3)[0] for l in after[18:20]] == lines[13:15] and [l.split("\t")[-3:] for l in after[18:20]] == [["0.5", "1.25", "4.0"], ["0.0", "0.0", "0.0"]] and after[20:] == [""]
    header, rows = abundance.read_table(out)
    assert header["bootstrap_groups"] == "on" and header["bootstrap_replicates"] == "97/100" and len(rows) == 2 and len(rows[0]) == 7
    abundance.write_table(str(tmp_path / "out.tsv"), ARGS, t)
    assert open(str(tmp_path / "out.tsv")).read() == gene_before                     # the gene table does not see the switch


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
    (tmp_path / "map.tsv").write_text("g1\tX\ng2\tX\n")
    out = str(tmp_path / "out.tsv")

    def request(**kw):
        args = {"seqfiles": [fq], "genes": str(faa), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-groups needs --bootstrap B \(--bootstrap None\)"):
        abundance.run_abundance(request(bootstrap_groups=True, groups=str(tmp_path / "map.tsv")))
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-groups needs --groups map.tsv \(--groups None\)"):
        abundance.run_abundance(request(bootstrap_groups=True, bootstrap=10))
    for bad, shown in (("yes", "'yes'"), (2, "2"), (0.5, "0\\.5"), (None, "None")):
        with pytest.raises(abundance.AbundanceError, match="bootstrap_groups %s is not a switch" % shown):
            abundance.run_abundance(request(bootstrap_groups=bad, bootstrap=10, groups=str(tmp_path / "map.tsv")))
    assert not os.path.exists(out)
    a = request()
    abundance.check_request(a)
    assert a["bootstrap_groups"] is False                                        # off by default
    a = request(bootstrap_groups=1, bootstrap=10, groups=str(tmp_path / "map.tsv"), coverage=True, ties=True, long_genes=True)
    abundance.check_request(a)
    assert a["bootstrap_groups"] is True
    with pytest.raises(AssertionError, match="GPU work was started"):          # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(bootstrap_groups=True, bootstrap=10, groups=str(tmp_path / "map.tsv")))


def test_cli_switch():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])["bootstrap_groups"] is False
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--bootstrap", "100", "--groups", "m.tsv", "--bootstrap-groups"])
    assert a["bootstrap_groups"] is True and a["bootstrap"] == 100 and a["groups"] == "m.tsv"


def test_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_group_bootstrap", "mc_group_bootstrap_ms", "mc_group_bootstrap_kernels_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("group_bootstrap", "group_bootstrap_ms", "group_bootstrap_kernels_ms"):
        assert callable(getattr(_native.Engine, m))
