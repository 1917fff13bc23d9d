"""The bootstrap of the coverage columns, host side (no GPU): the rules of csrc/mc_covboot.h compiled by g++ (tests/emul/covboot.cpp, once
more under -fsanitize=address,undefined) against the numpy restatement (tests/covboot_restated.py) on the cases the device harness runs
(tests/covboot_cases.py) - the entries, the cursor and dropped, the covered residues and det exactly, the six doubles bit for bit; the
statement's three invariants; need against abundance.detect; the conditions of the cases; every refusal before an engine is opened; the
table with and without the switch; and the new symbols of the ABI."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import covboot_cases as cbc
import covboot_restated as CR
import geneboot_restated as GR
import order_cases as oc
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


# ---- the rules of mc_covboot.h on the CPU -------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "covboot")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(HERE, "emul", "covboot.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "covboot", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "covboot_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _run(exe, name, arrays, tmp):
    oc.write_sections(tmp / (name + ".in"), arrays)
    p = subprocess.run([exe, "run", str(tmp / (name + ".in")), str(tmp / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and not p.stderr, (name, p.returncode, p.stderr.decode())
    return oc.read_sections(tmp / (name + ".out"))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rules_of_mc_covboot_h_on_the_device_cases(which, driver, driver_san, tmp_path):
    """every case: the entries in row order (the emulation reserves slots by a running count), the cursor, dropped, and - where every
    entry fitted - the covered residues and det exactly and the six doubles bit for bit, with the three invariants (covboot_cases.compare)"""
    exe = driver if which == "plain" else driver_san
    names = set()
    for c in cbc.cases():
        o = _run(exe, c["name"], cbc.sections_in(c), tmp_path)
        x, cap = cbc.expect(c), cbc.capacity(c)
        lst, cur = np.frombuffer(o[0], CR.ENTRY), np.frombuffer(o[1], "<u8")
        n = len(x["q"])
        assert int(cur[0]) == n == int(x["ab"]["reads"][:c["nseq"]].sum()) and int(cur[1]) == max(0, n - cap) and len(lst) == min(n, cap), c["name"]
        m = len(lst)
        for f, want in (("q", x["q"]), ("gene", x["g"]), ("s", x["s"]), ("e", x["e"])):
            assert np.array_equal(lst[f].astype(np.int64), want[:m]), (c["name"], f)
        det = np.frombuffer(o[4], "<u8")
        assert len(det) == (0 if c["F"] is None else c["nseq"])
        if cap >= n:
            cbc.compare(c, np.frombuffer(o[2], "<u8"), np.frombuffer(o[3], "<f8"), det)
        names.add(c["name"])
    assert len(names) == len(cbc.cases()) >= 15


def test_invariants_hold_on_the_restatement():
    """cov <= covered of the whole sample; cov > 0 implies a read of the gene in the replicate, and the converse where every span is valid; a
    gene with one read covers nothing or its one span"""
    for c in cbc.cases():
        x = cbc.expect(c)
        cbc.invariants(c, x["cov"], x["cv"]["covered"], x["counts"])
        assert np.array_equal(np.bincount(x["g"], minlength=c["nseq"]), x["ab"]["reads"][:c["nseq"]])         # the count table's reads size the slices
        assert (x["cov"].max(axis=1) <= x["cv"]["covered"]).all() and (x["stats"][:, 5] <= x["cv"]["covered"]).all()
        if x["det"] is not None:
            assert (x["det"] <= c["B"]).all() and not x["det"][x["ab"]["reads"][:c["nseq"]] == 0].any()
    # a broken cov is caught: more than the sample covers; covered residues without a read in the replicate
    c = {k["name"]: k for k in cbc.cases()}["b64"]
    x = cbc.expect(c)
    bad = x["cov"].copy()
    bad[0, 3] = x["cv"]["covered"][0] + 1
    with pytest.raises(AssertionError, match="covers more than the sample"):
        cbc.invariants(c, bad, x["cv"]["covered"], x["counts"])
    gene5 = np.flatnonzero(x["counts"][5] == 0)
    assert len(gene5) > 5
    bad = x["cov"].copy()
    bad[5, gene5[0]] = 1
    with pytest.raises(AssertionError, match="without a read of the gene"):
        cbc.invariants(c, bad, x["cv"]["covered"], x["counts"])


def test_need_is_the_integer_form_of_detect():
    """need = max(1, ceil(F x length_aa)) in float64: for every length 1 .. 2,047, every F and every covered 0 .. length, covered >= need
    exactly when abundance.detect says 1 for a gene with reads"""
    lengths = np.arange(1, 2048, dtype=np.int64)
    for F in (0.001, 1.0 / 3.0, 0.5, 0.9, 1.0):
        need = abundance.coverage_need(lengths, F)
        assert need.dtype == np.uint32 and (need >= 1).all() and np.array_equal(need.astype(np.int64), CR.need(lengths, F))
        for ln, nd in zip(lengths.tolist(), need.tolist()):
            covered = np.arange(0, ln + 1, dtype=np.int64)
            want = abundance.detect(np.ones(ln + 1, np.int64), covered, np.full(ln + 1, ln, np.int64), F)
            want[0] = 0                                                # (no residue covered: no read of the gene in the replicate)
            assert np.array_equal((covered >= nd).astype(np.int64), want), (F, ln, nd)


def test_cases_reach_what_they_are_for():
    """the conditions of the cases, from the restatement alone: without them the device tests could pass empty"""
    by = {c["name"]: c for c in cbc.cases()}
    assert [by["b%d" % B]["B"] for B in cbc.BS] == [1, 63, 64, 65, 257, 4096]
    x = cbc.expect(by["b64"])
    span = {int(q): (int(s), int(e)) for q, s, e in zip(x["q"], x["s"], x["e"])}
    gene = {int(q): int(g) for q, g in zip(x["q"], x["g"])}
    assert span[0] == (5, 5) and span[1][0] == 0 and span[2][1] == cbc.SPAN_LENGTHS[0] - 1                      # a single residue, from 0, to len - 1
    assert span[3][1] + 1 == span[4][0] and span[4][0] < span[5][0] <= span[4][1] < span[5][1]                  # two that abut, one that overlaps
    assert span[5][0] <= span[6][0] and span[6][1] <= span[5][1] and span[6] == span[7]                         # one that nests, two identical
    assert span[8][0] < 64 <= span[8][1] and span[9][0] < 128 <= span[9][1] and gene[9] == 0                    # crossing a multiple of 64 words; read 9's top row fails min_ident
    assert span[11] == CR.EMPTY == span[13] and gene[11] == gene[13] == 2 and span[12] == (10, 20)              # send == len, sstart > send: the empty entry, and the read keeps its entry
    assert span[14] == (0, 0) and cbc.SPAN_LENGTHS[3] == 1
    reads = np.bincount(x["g"], minlength=7)
    assert reads.tolist() == [10, 1, 3, 1, 0, 1, 0]                                                              # genes without reads between genes with reads, and at the end
    assert int(cbc.expect(by["b1"])["g"][9]) == 4                                                                  # without the cut-off read 9 goes to gene 4
    x1 = cbc.expect(by["b4096"])
    assert 0 < x1["det"][0] < 4096 and len(set(x1["cov"][0].tolist())) > 10 and set(x1["cov"][5].tolist()) == {0, 64}   # some replicates detect gene 0, some do not
    x = cbc.expect(by["window"])
    W, L = CR.WINDOW, by["window"]["lengths"][1]
    span = {int(q): (int(s), int(e)) for q, s, e in zip(x["q"], x["s"], x["e"])}
    assert L == W + 100 and span[2][1] < W - 1 and span[3][0] < W <= span[3][1] and span[4][1] == W - 1 and span[5][0] == W and span[6][1] == L - 1
    assert span[7][0] < W < span[7][1] and span[9] == CR.EMPTY and int(x["cv"]["covered"][1]) > 400 and len(set(x["cov"][1].tolist())) > 10
    x = cbc.expect(by["one_gene"])
    assert int((x["g"] == 1).sum()) == 200 and len(x["q"]) == 200 and 0 < x["det"][1] < 64
    c = by["workgroups"]
    x, q = cbc.expect(c), c["rows"]["query"]
    heads = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
    adds = set(x["q"].tolist())
    assert len(heads) > 256 and len(c["rows"]) > 3 * 256 and len(adds) > 256
    assert 255 in heads and q[255] in adds and 512 in heads and q[512] in adds
    assert not any(q[h] in adds for h in heads if 256 <= h < 512) and any(q[h] in adds for h in heads if h >= 768)
    c = by["launches"]
    q = c["rows"]["query"]
    assert len(c["cuts"]) == 3 and all(q[cut - 1] != q[cut] for cut in c["cuts"][:-1])
    assert np.array_equal(cbc.expect(c)["cov"][:, :63], cbc.expect(by["b63"])["cov"])                            # replicate b depends neither on B nor on the launches
    assert int(cbc.expect(by["big_ids"])["q"].max()) == 2 ** 31 - 1
    n = len(cbc.expect(by["short"])["q"])
    assert cbc.capacity(by["short"]) == n - 1 and not by["off"]["launch"] and by["no_need"]["F"] is None and cbc.expect(by["no_need"])["det"] is None
    assert all(cbc.capacity(c) == len(cbc.expect(c)["q"]) for c in cbc.cases() if c["name"] != "short")         # exactly full
    perm, base = by["idmap"]["idmap"]
    x = cbc.expect(by["idmap"])
    assert base > 0 and set(x["q"].tolist()) == {base + int(perm[p]) for p in cbc.expect(by["b64"])["q"].tolist()} and not np.array_equal(x["cov"], cbc.expect(by["b64"])["cov"])


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
NAMES = ["g1", "g2", "g3"]
LENGTH = np.array([120, 300, 2047], np.int64)
ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": None}
B = 4


def _records(cov_boot, min_breadth):
    """the two records between the stages (abundance.build_table's input), as a device pass of --min-breadth 0.5 --bootstrap 4 would leave them"""
    sample = {"ags": 3.0e6, "source": "--ags", "pargs": {"nreads": 1000, "read_length": 100}, "classes": None, "L": 100}
    stats = np.arange(18, dtype=np.float64).reshape(3, 6) / 7.0
    counts = {"ab": {"reads": np.array([3, 0, 7], np.int64), "aligned": np.array([90, 0, 231], np.int64), "assigned": 10, "searched": 1000}, "ac": None,
              "cov": {"covered": np.array([70, 0, 200], np.int64), "spanned": np.array([90, 0, 231], np.int64), "max_depth": np.array([2, 0, 3], np.int64)}, "depth": None,
              "ti": None, "tcov": None, "cu": None, "points": None, "gb": {"stats": stats, "used": 4, "dropped": 0}, "gbg": None, "scale": np.full(4, 1.0 / 30.0), "fold_stats": None,
              "sampled": 1000, "gids": None, "gnames": None, "search_ms": 1.0, "abundance_ms": 0.5}
    if cov_boot:
        cb = {"stats": np.array([[240.0, 50.0, 55.0, 60.0, 65.0, 70.0], [0.0] * 6, [600.0, 5000.0, 100.0, 120.0, 180.0, 200.0]]), "dropped": 0}
        if min_breadth is not None:
            cb["detected"] = np.array([3, 0, 0], np.int64)
        counts.update({"cb": cb, "coverage_bootstrap_ms": 0.25})
    return sample, counts


def _args(min_breadth, **kw):
    return dict(ARGS, coverage=True, min_breadth=min_breadth, depth_out=None, ties=False, curve=None, curve_genes=None, bootstrap=B, bootstrap_seed=None, bootstrap_groups=False,
                mixed_lengths=None, long_genes=False, gene_fold=None, bootstrap_ties=False, tie_list_factor=None, **kw)


def test_files_with_and_without_the_switch(tmp_path):
    """the same records with and without the coverage bootstrap's part: without it the file is byte for byte the file the writer wrote
    before the switch existed (its lines are spelled out here); with it, five columns behind every column and one header line behind the
    four bootstrap lines - and write_table / read_table round-trip them; without min_breadth four columns"""
    seqs = ["A" * int(n) for n in LENGTH]
    sample, counts = _records(False, 0.5)
    a = _args(0.5, bootstrap_coverage=False)
    plain = abundance.build_table(a, sample, counts, NAMES, seqs, None)
    out = str(tmp_path / "plain.tsv")
    abundance.write_table(out, a, plain)
    before = open(out).read()
    lines = before.split("\n")
    assert lines[11:19] == ["# coverage:\ton", "# min_breadth:\t0.5", "# genes_detected:\t1", "# bootstrap:\t4", "# bootstrap_seed:\t0", "# bootstrap_replicates:\t4/4",
                            "# bootstrap_denominator:\tfixed_ags",
                            "gene\tlength_aa\treads\taligned_aa\trpkg\tcovered_aa\tbreadth\tmean_depth\tmax_depth\tdetected\trpkg_boot_se\trpkg_ci95_low\trpkg_ci95_high"]
    assert lines[19].split("\t")[:10] == ["g1", "120", "3", "90", lines[19].split("\t")[4], "70", repr(70 / 120), "0.75", "2", "1"] and lines[22:] == [""]
    assert "coverage_bootstrap_ms" not in a and "breadth_boot_se" not in plain and [c for c, _ in abundance.table_columns(plain)][-1] == "rpkg_ci95_high"
    # a record from before the switch (no "cb" key at all) and args that never heard of it give the same bytes
    old_args = {k: v for k, v in _args(0.5).items() if k != "bootstrap_coverage"}
    abundance.write_table(out, old_args, abundance.build_table(old_args, sample, {k: v for k, v in counts.items() if k != "cb"}, NAMES, seqs, None))
    assert open(out).read() == before
    sample, counts = _records(True, 0.5)
    a = _args(0.5, bootstrap_coverage=True)
    t = abundance.build_table(a, sample, counts, NAMES, seqs, None)
    assert a["coverage_bootstrap_ms"] == 0.25 and t["cov_boot_stats"] is counts["cb"]["stats"] and t["cov_boot_detected"] is counts["cb"]["detected"]
    st = counts["cb"]["stats"]
    # B = 4: the 2.5th percentile lies 0.075 of the way from x[0] to x[1], the 97.5th 0.925 of the way from x[2] to x[3]
    assert np.array_equal(t["breadth_boot_mean"], st[:, 0] / 4 / LENGTH) and GR.same_bits(t["breadth_boot_se"], np.sqrt(st[:, 1] / 3) / LENGTH)
    assert np.allclose(t["breadth_ci95_low"], (st[:, 2] + 0.075 * (st[:, 3] - st[:, 2])) / LENGTH, rtol=1e-15, atol=0)
    assert np.allclose(t["breadth_ci95_high"], (st[:, 4] + 0.925 * (st[:, 5] - st[:, 4])) / LENGTH, rtol=1e-15, atol=0)
    vals = np.array([55.0, 60.0, 65.0, 70.0])                                                # gene 1's order statistics ARE its four values
    assert np.allclose([t["breadth_ci95_low"][0], t["breadth_ci95_high"][0]], np.percentile(vals / 120.0, [2.5, 97.5]), rtol=1e-15, atol=0)
    assert t["detected_support"].tolist() == [0.75, 0.0, 0.0]
    assert [c for c, _ in abundance.table_columns(t)][-8:] == list(abundance.BOOT_COLUMNS + abundance.COV_BOOT_COLUMNS) + ["detected_support"]
    out2 = str(tmp_path / "cov.tsv")
    abundance.write_table(out2, a, t)
    new = open(out2).read().split("\n")
    assert new[:18] == lines[:18] and new[18] == "# bootstrap_coverage:\ton"
    assert new[19] == lines[18] + "\t" + "\t".join(abundance.COV_BOOT_COLUMNS + ("detected_support",))
    assert [l.rsplit("\t", 5)[0] for l in new[20:23]] == lines[19:22] and new[23:] == [""]                            # the existing columns keep their text
    assert new[20].split("\t")[-5:] == [repr(0.5), repr(float(np.sqrt(50.0 / 3) / 120)), repr(float(t["breadth_ci95_low"][0])), repr(float(t["breadth_ci95_high"][0])), "0.75"]
    header, rows = abundance.read_table(out2)
    assert header["bootstrap_coverage"] == "on" and len(rows) == 3 and len(rows[0]) == 18
    assert [r[-5:] for r in rows] == [[repr(float(x)) for x in v] for v in zip(*(t[c] for c in abundance.COV_BOOT_COLUMNS + ("detected_support",)))]
    # without min_breadth: no need, no detected, no detected_support
    sample, counts = _records(True, None)
    a = _args(None, bootstrap_coverage=True)
    t = abundance.build_table(a, sample, counts, NAMES, seqs, None)
    assert "detected_support" not in t and "cov_boot_detected" not in t and [c for c, _ in abundance.table_columns(t)][-4:] == list(abundance.COV_BOOT_COLUMNS)
    # with the tie bootstrap's columns too, the new ones come last
    sample, counts = _records(True, 0.5)
    counts.update({"ti": {"unique": np.array([2, 0, 7], np.int64), "candidates": np.array([3, 1, 8], np.int64), "share": np.array([5 << 31, 0, 15 << 31], np.uint64), "ambiguous": 1,
                          "group_unique": np.zeros(0, np.int64), "group_ambiguous": 0},
                   "tcov": {"covered_any": np.array([70, 5, 200], np.int64), "spanned_any": np.array([90, 5, 240], np.int64)},
                   "tb": {"stats": counts["gb"]["stats"] * 0.5, "used": 4, "dropped": 0}, "tie_list": (12, 4000)})
    a = dict(_args(0.5, bootstrap_coverage=True), ties=True, bootstrap_ties=True)
    cols = [c for c, _ in abundance.table_columns(abundance.build_table(a, sample, counts, NAMES, seqs, None))]
    assert cols[-8:] == list(abundance.TIE_BOOT_COLUMNS + abundance.COV_BOOT_COLUMNS) + ["detected_support"]


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
    out = str(tmp_path / "out.tsv")

    def request(**kw):
        args = {"seqfiles": [fq], "genes": str(faa), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-coverage needs --bootstrap B \(--bootstrap None\)"):
        abundance.run_abundance(request(bootstrap_coverage=True, coverage=True))
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-coverage needs --coverage, --min-breadth or --depth-out \(--coverage False\)"):
        abundance.run_abundance(request(bootstrap_coverage=True, bootstrap=10))
    with pytest.raises(abundance.AbundanceError, match="bootstrap_coverage 'yes' is not a switch"):
        abundance.run_abundance(request(bootstrap_coverage="yes", bootstrap=10, coverage=True))
    with pytest.raises(abundance.AbundanceError, match="--bootstrap 10 cannot be combined with --curve 4"):      # --curve stays refused
        abundance.run_abundance(request(bootstrap_coverage=True, bootstrap=10, coverage=True, curve=4))
    assert not os.path.exists(out)
    a = request()
    abundance.check_request(a)
    assert a["bootstrap_coverage"] is False                                        # off by default
    for more in (dict(coverage=True), dict(min_breadth=0.5), dict(depth_out=str(tmp_path / "d.tsv")), dict(coverage=True, ties=True, bootstrap_ties=True, long_genes=True)):
        a = request(bootstrap_coverage=1, bootstrap=10, **more)
        abundance.check_request(a)
        assert a["bootstrap_coverage"] is True and a["coverage"] is True
    with pytest.raises(AssertionError, match="GPU work was started"):          # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(bootstrap_coverage=True, bootstrap=10, min_breadth=0.5))


def test_lists_are_sized_at_one_moment_by_one_count():
    """_size_lists: the coverage list has the gene list's entries, set behind it; without the switch the engine never hears of it"""
    calls = []

    class Eng:
        def set_gene_bootstrap(self, n):
            calls.append(("gene", n))

        def set_tie_bootstrap(self, n):
            calls.append(("tie", n))

        def set_coverage_bootstrap(self, n):
            calls.append(("coverage", n))
    abundance._size_lists(Eng(), {"bootstrap_ties": False, "tie_list_factor": None, "bootstrap_coverage": True}, 5000)
    abundance._size_lists(Eng(), {"bootstrap_ties": True, "tie_list_factor": 2, "bootstrap_coverage": True}, 70)
    abundance._size_lists(Eng(), {"bootstrap_ties": False, "tie_list_factor": None, "bootstrap_coverage": False}, 9)
    abundance._size_lists(Eng(), {"bootstrap_ties": False, "tie_list_factor": None, "bootstrap_coverage": True}, 0)
    assert calls == [("gene", 5000), ("coverage", 5000), ("gene", 70), ("tie", 140), ("coverage", 70), ("gene", 9), ("gene", 0)]


def test_cli_switch():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])["bootstrap_coverage"] is False
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--min-breadth", "0.5", "--bootstrap", "100", "--bootstrap-coverage"])
    assert (a["bootstrap_coverage"], a["min_breadth"], a["bootstrap"]) == (True, 0.5, 100)


def test_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_set_coverage_bootstrap", "mc_coverage_bootstrap", "mc_coverage_bootstrap_ms", "mc_coverage_bootstrap_kernels_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("set_coverage_bootstrap", "coverage_bootstrap", "coverage_bootstrap_ms", "coverage_bootstrap_kernels_ms"):
        assert callable(getattr(_native.Engine, m))
    assert CR.MAXCAP == 2 ** 31 - 1 and CR.WINDOW == 2048 and abundance.COV_BOOT_COLUMNS[0] == "breadth_boot_mean"
