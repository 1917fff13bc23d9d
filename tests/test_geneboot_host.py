"""The bootstrap of the gene counts, host side (no GPU): the host part of csrc/mc_geneboot.h's statement in abundance.py against
numpy.percentile for every number of used replicates from 1 to 200; the header's addition order compiled by g++ (tests/emul/geneboot.cpp,
once more under -fsanitize=address,undefined) against the numpy restatement (tests/geneboot_restated.py) bit for bit; the replicate
counts on the cases the device harness runs (tests/geneboot_cases.py); the sanity of the restatement itself; every refusal before an
engine is opened; the table with and without the switch; and the new symbols of the ABI."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import boot_restated as br
import geneboot_cases as gc
import geneboot_restated as GR
import order_cases as oc
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


# ---- the host part: standard error and interval from the six doubles ---------------------------------------------------------------------
def test_interval_is_numpy_percentile_for_every_m():
    """m = 1 .. 200 used replicates (of m + 3: three are unused): the order-statistic indices and the interpolation of boot_columns give
    numpy.percentile(values / kb, [2.5, 97.5]) exactly, on values with and without ties; the standard error is numpy.std(ddof=1)."""
    rng = np.random.default_rng(25)
    length = np.array([7, 120, 2047], np.int64)
    kb = 3.0 * length / 1000.0
    for m in range(1, 201):
        for ties in (False, True):
            B = m + 3
            scale = rng.uniform(1e-3, 1e-2, B) if not ties else np.full(B, 0.015625)
            scale[[0, B // 2, B - 1]] = [np.nan, 0.0, -1.0]
            c = rng.integers(0, 5 if ties else 4000, (3, B))
            st = GR.stats(c, scale)
            use = GR.used(scale)
            assert int(use.sum()) == m
            se, lo, hi = abundance.boot_columns(st, m, length)
            for g in range(3):
                v = (c[g].astype(np.float64) * scale)[use] / kb[g]
                want = np.percentile(v, [2.5, 97.5])
                assert lo[g] == want[0] and hi[g] == want[1], (m, ties, g)
                assert [GR.index(m, k) for k in (2, 3, 4, 5)] == [int(np.floor((m - 1) * 0.025)), min(int(np.floor((m - 1) * 0.025)) + 1, m - 1),
                                                                  int(np.floor((m - 1) * 0.975)), min(int(np.floor((m - 1) * 0.975)) + 1, m - 1)]
                if m > 1:
                    assert se[g] == pytest.approx(np.std(v, ddof=1), rel=1e-9, abs=1e-300), (m, ties, g)
                else:
                    assert np.isnan(se[g])
    se, lo, hi = abundance.boot_columns(np.full((3, 6), np.nan), 0, length)
    assert np.isnan(se).all() and np.isnan(lo).all() and np.isnan(hi).all()


def test_scale_of_replicate_ags():
    s = abundance.boot_scale([3.0e6, None, 2.5e6, 1.0e6], [1000, 900, 0, 250], 100)
    assert s[0] == 3.0e6 / (100.0 * 1000.0) and np.isnan(s[1]) and np.isnan(s[2]) and s[3] == 1.0e6 / 25000.0
    assert s[0] == 1.0 / abundance.genome_equivalents(1000, 100, 3.0e6) or abs(s[0] * abundance.genome_equivalents(1000, 100, 3.0e6) - 1.0) < 1e-15
    assert GR.used(s).tolist() == [True, False, False, True]


# ---- the rules of mc_geneboot.h on the CPU ------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "geneboot")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(HERE, "emul", "geneboot.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "geneboot", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "geneboot_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _run(exe, verb, name, arrays, tmp):
    oc.write_sections(tmp / (name + ".in"), arrays)
    p = subprocess.run([exe, verb, str(tmp / (name + ".in")), str(tmp / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and not p.stderr, (name, p.returncode, p.stderr.decode())
    return oc.read_sections(tmp / (name + ".out"))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000, 4096])
def test_the_stated_addition_order_bit_for_bit(B, driver, tmp_path):
    """sum and m2 of g++'s build of the header == the numpy restatement, bit for bit - with every replicate used, with holes, with values
    of very different magnitudes (where another order of additions gives other bits)"""
    rng = np.random.default_rng(B)
    for k, kind in enumerate(("plain", "holes", "one", "none", "constant")):
        scale = gc._scale(B, kind, seed=k)
        c = rng.integers(0, 1 << int(rng.integers(1, 40)), B).astype(np.uint64)
        got = np.frombuffer(_run(driver, "sums", "b%d_%s" % (B, kind), [c, scale], tmp_path)[0], "<f8")
        want = GR.gene_stats(c.astype(np.int64), scale)
        assert GR.same_bits(got, want), (B, kind, got.tolist(), want.tolist())


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rules_of_mc_geneboot_h_on_the_device_cases(which, driver, driver_san, tmp_path):
    exe = driver if which == "plain" else driver_san
    names = set()
    for c in gc.cases():
        o = _run(exe, "run", c["name"], gc.sections_in(c), tmp_path)
        gc.compare(c, np.frombuffer(o[0], "<u8").astype(np.int64), np.frombuffer(o[1], "<f8"))
        names.add(c["name"])
    assert len(names) == len(gc.cases()) >= 18


def test_cases_reach_what_they_are_for():
    """the conditions of the cases, from the restatement alone: without them the device tests could pass empty"""
    by = {c["name"]: c for c in gc.cases()}
    assert [by["b%d" % B]["B"] for B in gc.BS] == [1, 63, 64, 65, 257, 4096] and GR.MAXB == 4096
    for nseq in (1, 3, 4, 5):
        e = gc.expect(by["genes%d" % nseq])
        have = np.bincount(e["s"], minlength=nseq) > 0
        assert have[0] and (nseq < 3 or (not have[1] and have[2]))               # a gene without reads between genes with reads
    one = gc.expect(by["one_gene"])
    assert len(one["q"]) > 2 * GR.per_tile(len(one["q"]), 64) and set(one["s"].tolist()) == {1}
    bd = gc.expect(by["boundary"])
    assert np.bincount(bd["s"], minlength=4).tolist() == [64, 0, 64, 7] and GR.per_tile(135, 65) == 64
    for k in (0, 2):
        c = by["launches_%d" % k]
        e = gc.expect(c)
        q = c["rows"]["query"]
        assert len(c["cuts"]) == 3 and all(q[cut - 1] != q[cut] for cut in c["cuts"][:-1]) and q[c["cuts"][0]] == 5000 and e["q"].max() == 2 ** 31 - 1
        assert int(e["s"][e["q"] == 2 ** 31 - 1][0]) == 2                        # (the higher bits win on the last read)
    assert len(gc.expect(by["launches_0"])["q"]) > len(gc.expect(by["launches_2"])["q"]) > 256
    for name, m in (("b65", 65 - 22), ("m_one", 1), ("m_none", 0), ("tied", 257)):
        assert gc.expect(by[name])["m"] == m, name
    assert np.isnan(by["b65"]["scale"]).any() and (by["b65"]["scale"] == 0).any() and (by["b65"]["scale"] < 0).any() and np.isinf(by["b65"]["scale"]).any()
    tied = gc.expect(by["tied"])
    assert len(np.unique(tied["counts"][0])) < 12 and tied["stats"][0][2] == tied["stats"][0][3]          # equal values across replicates
    assert all(gc.capacity(c) == len(gc.expect(c)["q"]) for c in gc.cases() if c["name"] != "short")
    assert gc.capacity(by["short"]) == len(gc.expect(by["short"])["q"]) - 1 and not by["off"]["launch"]


def test_the_restatement_draws_poisson_weights():
    """A gene with c = 400 reads, B = 4096: every replicate count is a sum of 400 Poisson(1) weights, mean 400 and variance 400.  The mean
    over the replicates has the standard deviation sqrt(c / B): within five of them of c.  The sample variance has the relative standard
    deviation sqrt(2 / (B - 1) + 1 / (c B)) = 2.2 %: within 15 % of c."""
    c, B = 400, 4096
    for seed in (0, 7, 20240917):
        q = np.arange(1000, 1000 + 3 * c, 3)
        cm = GR.counts(q, np.zeros(c, np.int64), 1, B, seed)[0]
        assert abs(cm.mean() - c) <= 5 * np.sqrt(c / B), (seed, cm.mean())
        assert abs(cm.var(ddof=1) - c) <= 0.15 * c, (seed, cm.var(ddof=1))
        assert np.array_equal(cm, br.weights(seed, np.arange(B, dtype=np.uint64)[:, None], q.astype(np.uint64)[None, :]).sum(axis=1))


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
NAMES = ["g1", "g2", "g3"]
LENGTH = np.array([120, 300, 2047], np.int64)
READS = np.array([5, 0, 7], np.int64)
ALIGNED = np.array([150, 0, 231], np.int64)
ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": "map.tsv"}
TODAY = ["# metagenome:\ta.fq.gz", "# genes:\tgenes.faa", "# sampled_reads:\t8672", "# trimmed_length:\t100", "# min_ident:\t60", "# min_aln:\t30", "# min_bits:\t35.5",
         "# average_genome_size:\t3051745.7641809303", "# ags_source:\trun_pipeline", "# genome_equivalents_sampled:\t%r" % (8672 * 100 / 3051745.7641809303),
         "# reads_assigned:\t12"]


def _table():
    ge = abundance.genome_equivalents(8672, 100, 3051745.7641809303)
    return {"gene": list(NAMES), "length_aa": LENGTH, "reads": READS, "aligned_aa": ALIGNED, "rpkg": abundance.rpkg(READS, LENGTH, ge),
            "sampled_reads": 8672, "trimmed_length": 100, "ags": 3051745.7641809303, "ags_source": "run_pipeline", "genome_equivalents_sampled": ge, "reads_assigned": 12}


def test_files_with_and_without_the_switch(tmp_path):
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, ARGS, t)
    before = open(out).read()
    lines = before.split("\n")
    assert lines[:11] == TODAY and lines[11] == "gene\tlength_aa\treads\taligned_aa\trpkg" and lines[13] == "g2\t300\t0\t0\t0.0" and lines[15:] == [""]      # the writer's output as it was
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    groups_before = open(out + ".groups.tsv").read()
    t.update({"rpkg_boot_se": np.array([0.25, 0.0, 0.125]), "rpkg_ci95_low": np.array([1.5, 0.0, 0.5]), "rpkg_ci95_high": np.array([2.5, 0.0, np.nan]), "boot_used": 97,
              "bootstrap": 100, "bootstrap_seed": 5, "bootstrap_denominator": "replicate_ags"})
    abundance.write_table(out, ARGS, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == TODAY and lines[11:15] == ["# bootstrap:\t100", "# bootstrap_seed:\t5", "# bootstrap_replicates:\t97/100", "# bootstrap_denominator:\treplicate_ags"]
    assert lines[15] == "gene\tlength_aa\treads\taligned_aa\trpkg\trpkg_boot_se\trpkg_ci95_low\trpkg_ci95_high"
    assert [l.rsplit("\t", 3)[0] for l in lines[15:19]] == before.split("\n")[11:15]                                  # the existing columns keep their text
    assert [l.split("\t")[-3:] for l in lines[16:19]] == [["0.25", "1.5", "2.5"], ["0.0", "0.0", "0.0"], ["0.125", "0.5", "nan"]] and lines[19:] == [""]
    header, rows = abundance.read_table(out)
    assert header["bootstrap"] == "100" and header["bootstrap_replicates"] == "97/100" and len(rows) == 3 and len(rows[0]) == 8
    abundance.write_groups(out + ".groups.tsv", ARGS, t)
    assert open(out + ".groups.tsv").read() == groups_before                                                          # the groups table does not bootstrap


# ---- refusals, before any engine is opened ----------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", boom)
    monkeypatch.setattr(microbe_census, "run_pipeline", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_refusals(tmp_path, no_engine, monkeypatch):
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    faa = tmp_path / "good.faa"
    faa.write_text(">g1 d\n%s\n>g2 d\n%s\n" % ("MKV" * 20, "MLA" * 30))
    out = str(tmp_path / "out.tsv")

    def request(**kw):
        args = {"seqfiles": [fq], "genes": str(faa), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    for bad, shown in ((0, "0"), (-1, "-1"), (4097, "4097"), (2.0, "2\\.0"), (2.5, "2\\.5"), ("ten", "ten"), (True, "True"), (False, "False")):
        with pytest.raises(abundance.AbundanceError, match="--bootstrap %s is not an integer from 1 to 4096" % shown):
            abundance.run_abundance(request(bootstrap=bad))
    with pytest.raises(abundance.AbundanceError, match="--bootstrap-seed 5 needs --bootstrap B"):
        abundance.run_abundance(request(bootstrap_seed=5))
    for bad, shown in ((-1, "-1"), (1 << 64, str(1 << 64)), (1.5, "1\\.5"), (True, "True")):
        with pytest.raises(abundance.AbundanceError, match="--bootstrap-seed %s is not an integer from 0 to 2\\^64 - 1" % shown):
            abundance.run_abundance(request(bootstrap=10, bootstrap_seed=bad))
    with pytest.raises(abundance.AbundanceError, match="--bootstrap 10 cannot be combined with --curve 4"):
        abundance.run_abundance(request(bootstrap=10, curve=4))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(abundance.AbundanceError, match="not computed by a distributed run"):
        abundance.run_abundance(request(bootstrap=10))
    monkeypatch.delenv("WORLD_SIZE")
    assert not os.path.exists(out)
    a = request()
    abundance.check_request(a)
    assert (a["bootstrap"], a["bootstrap_seed"]) == (None, None)                 # off by default
    for B in (1, 4096, np.int64(7)):
        a = request(bootstrap=B, bootstrap_seed=np.int64(3), coverage=True, ties=True)
        abundance.check_request(a)
        assert a["bootstrap"] == int(B) and type(a["bootstrap"]) is int and a["bootstrap_seed"] == 3 and a["curve"] is None
    with pytest.raises(AssertionError, match="GPU work was started"):          # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(bootstrap=10, min_breadth=0.5, ties=True))


def test_cli_switches():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])
    assert (a["bootstrap"], a["bootstrap_seed"]) == (None, None)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--bootstrap", "100", "--bootstrap-seed", "9"])
    assert (a["bootstrap"], a["bootstrap_seed"]) == (100, 9)
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--bootstrap", "ten"])


def test_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_set_gene_bootstrap", "mc_gene_bootstrap", "mc_gene_bootstrap_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("set_gene_bootstrap", "gene_bootstrap", "gene_bootstrap_ms"):
        assert callable(getattr(_native.Engine, m))
    assert abundance.MAX_BOOT == GR.MAXB == 4096


def test_replicate_read_counts_are_exposed_additively():
    """bootstrap_replicates(..., reads_out) appends every replicate's W[b] + N0[b] and returns what it returned"""
    import inspect
    sig = inspect.signature(microbe_census.bootstrap_replicates)
    assert list(sig.parameters)[-1] == "reads_out" and sig.parameters["reads_out"].default is None
    assert inspect.signature(microbe_census.bootstrap_ags).parameters["reads_out"].default is None
