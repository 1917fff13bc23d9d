"""The bootstrap of the tie shares, host side (no GPU): the rules of csrc/mc_tieboot.h compiled by g++ (tests/emul/tieboot.cpp, once more
under -fsanitize=address,undefined) against the numpy restatement (tests/tieboot_restated.py) on the cases the device harness runs
(tests/tieboot_cases.py) - the entries, the cursor and dropped, the replicate shares exactly, the six doubles bit for bit; the statement's
two invariants; the conditions of the cases; every refusal before an engine is opened; the table with and without the switch; and the
new symbols of the ABI."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import geneboot_restated as GR
import order_cases as oc
import tieboot_cases as tbc
import tieboot_restated as TR
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


# ---- the rules of mc_tieboot.h on the CPU -------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "tieboot")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(HERE, "emul", "tieboot.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "tieboot", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "tieboot_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _run(exe, name, arrays, tmp):
    oc.write_sections(tmp / (name + ".in"), arrays)
    p = subprocess.run([exe, "run", str(tmp / (name + ".in")), str(tmp / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0 and not p.stderr, (name, p.returncode, p.stderr.decode())
    return oc.read_sections(tmp / (name + ".out"))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rules_of_mc_tieboot_h_on_the_device_cases(which, driver, driver_san, tmp_path):
    """every case: the entries in row order (the emulation reserves slots by a running count), the cursor, dropped, and - where every
    entry fitted - the shares exactly and the six doubles bit for bit, with the two invariants (tieboot_cases.compare)"""
    exe = driver if which == "plain" else driver_san
    names = set()
    for c in tbc.cases():
        o = _run(exe, c["name"], tbc.sections_in(c), tmp_path)
        e, cap = tbc.expect(c), tbc.capacity(c)
        lst, cur = np.frombuffer(o[0], TR.ENTRY), np.frombuffer(o[1], "<u8")
        n = len(e["q"])
        assert int(cur[0]) == n == sum(e["k"]) and int(cur[1]) == max(0, n - cap) and len(lst) == min(n, cap), c["name"]
        m = len(lst)
        assert np.array_equal(lst["q"], e["q"][:m].astype(np.uint32)) and np.array_equal(lst["gene"], e["s"][:m].astype(np.uint32)), c["name"]
        assert np.array_equal(lst["share_m1"].astype(np.uint64) + np.uint64(1), e["share"][:m]), c["name"]
        if cap >= n:
            tbc.compare(c, np.frombuffer(o[2], "<u8"), np.frombuffer(o[3], "<f8"))
        names.add(c["name"])
    assert len(names) == len(tbc.cases()) >= 18


def test_invariants_hold_on_the_restatement():
    """sum_s cs[b][s] = 2^32 x sum_s c[b][s] for every b; and without a tied read cs = c x 2^32 and the six doubles are the gene bootstrap's"""
    seen_ties = seen_none = False
    for c in tbc.cases():
        e = tbc.expect(c)
        tbc.invariants(c, e["shares"], e["stats"])
        assert sum(int(v) for v in e["share"]) == len(e["k"]) * TR.ONE == int(e["ab"]["reads"][:c["nseq"]].sum()) * TR.ONE   # a read's shares add up to one read
        assert np.array_equal(np.bincount(e["s"], minlength=c["nseq"]), e["ties"]["candidates"])                   # the tie table's candidates size the slices
        assert np.array_equal(np.bincount(e["s"], weights=None, minlength=c["nseq"]) > 0, e["shares"].any(axis=1) | (e["ties"]["candidates"] > 0))
        seen_ties |= max(e["k"]) > 1
        seen_none |= max(e["k"]) == 1
    assert seen_ties and seen_none
    e = tbc.expect({c["name"]: c for c in tbc.cases()}["no_ties"])
    assert np.array_equal(e["shares"], e["counts"].astype(np.uint64) << np.uint64(32)) and e["counts"].any()


def test_cases_reach_what_they_are_for():
    """the conditions of the cases, from the restatement alone: without them the device tests could pass empty"""
    by = {c["name"]: c for c in tbc.cases()}
    assert [by["b%d" % B]["B"] for B in tbc.BS] == [1, 63, 64, 65, 257, 4096]
    e = tbc.expect(by["b64"])
    sets = dict(e["ties"]["sets"])
    ks = {q: len(m) for q, m in sets.items()}
    assert {1, 2, 3, 6, 7} <= set(ks.values())
    assert ks[5] == 2 and [s for s, _, _ in sets[5]] == [0, 1]                    # a subject that ties twice is one entry
    assert ks[6] == 2 and [s for s, _, _ in sets[6]] == [5, 3]                    # tied rows that are not adjacent
    assert ks[10] == 2 and [s for s, _, _ in sets[10]] == [1, 0]                  # tied rows whose subject is >= nseq are no entries
    assert 9 not in sets and 12 not in sets                                        # a first-rule subject >= nseq; no passing row
    assert ks[8] == 2 and [s for s, _, _ in sets[8]] == [5, 6] and ks[7] == 1     # a top row, a tied row that fails a cut-off
    assert int(e["share"][e["q"] == 2][0]) == TR.ONE // 3 + 1 and int(e["share"][e["q"] == 0][0]) == TR.ONE
    assert np.isnan(by["b65"]["scale"]).any() and (by["b65"]["scale"] == 0).any() and (by["b65"]["scale"] < 0).any() and np.isinf(by["b65"]["scale"]).any()
    assert tbc.expect(by["m_one"])["m"] == 1 and tbc.expect(by["m_none"])["m"] == 0 and tbc.expect(by["b65"])["m"] == 65 - 22
    e = tbc.expect(by["k500"])
    assert e["k"] == [500, 1] and TR.ONE - 500 * (TR.ONE // 500) == 296 and int(e["share"][0]) == TR.ONE // 500 + 296 and int(e["s"][0]) == 499
    assert set(e["share"][1:500].tolist()) == {TR.ONE // 500}
    e = tbc.expect(by["gaps"])
    assert (np.bincount(e["s"], minlength=7) > 0).tolist() == [True, False, True, True, False, False, True]
    e = tbc.expect(by["one_gene"])
    per = GR.per_tile(len(e["q"]), 64)
    assert per == tbc.PER_TILE and int((e["s"] == 1).sum()) == 200 > 2 * per and all(1 in [s for s, _, _ in m] for _, m in e["ties"]["sets"])
    c = by["workgroups"]
    e, q = tbc.expect(c), c["rows"]["query"]
    heads = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
    adds = set(dict(e["ties"]["sets"]))
    assert len(heads) > 256 and len(c["rows"]) > 3 * 256
    assert 255 in heads and q[255] in adds and 512 in heads and q[512] in adds and dict(zip(dict(e["ties"]["sets"]), e["k"]))[255] == 3
    assert not any(q[h] in adds for h in heads if 256 <= h < 512) and any(q[h] in adds for h in heads if h < 256) and any(q[h] in adds for h in heads if h >= 512)
    c = by["launches"]
    q = c["rows"]["query"]
    assert len(c["cuts"]) == 3 and all(q[cut - 1] != q[cut] for cut in c["cuts"][:-1])
    n = len(tbc.expect(by["short"])["q"])
    assert tbc.capacity(by["short"]) == n - 1 and tbc.capacity(by["zero"]) == 0 and not by["off"]["launch"]
    assert all(tbc.capacity(c) == len(tbc.expect(c)["q"]) for c in tbc.cases() if c["name"] not in ("short", "zero"))   # exactly full
    perm, base = by["idmap"]["idmap"]
    e = tbc.expect(by["idmap"])
    assert base > 0 and not np.array_equal(perm, np.arange(len(perm))) and set(e["q"].tolist()) == {base + int(perm[x]) for x in dict(tbc.expect(by["b64"])["ties"]["sets"])}
    assert max(tbc.expect(by["no_ties"])["k"]) == 1


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
NAMES = ["g1", "g2", "g3"]
LENGTH = np.array([120, 300, 2047], np.int64)
ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": None}


def _records(tie_boot):
    """the two records between the stages (abundance.build_table's input), as a device pass of --ties --bootstrap 4 would leave them"""
    sample = {"ags": 3.0e6, "source": "--ags", "pargs": {"nreads": 1000, "read_length": 100}, "classes": None, "L": 100}
    stats = np.arange(18, dtype=np.float64).reshape(3, 6) / 7.0
    share = np.array([5 * TR.ONE // 2, 0, 15 * TR.ONE // 2], np.uint64)
    counts = {"ab": {"reads": np.array([3, 0, 7], np.int64), "aligned": np.array([90, 0, 231], np.int64), "assigned": 10, "searched": 1000}, "ac": None, "cov": None, "depth": None,
              "ti": {"unique": np.array([2, 0, 7], np.int64), "candidates": np.array([3, 1, 8], np.int64), "share": share, "ambiguous": 1, "group_unique": np.zeros(0, np.int64), "group_ambiguous": 0},
              "tcov": None, "cu": None, "points": None, "gb": {"stats": stats, "used": 4, "dropped": 0}, "gbg": None, "scale": np.full(4, 1.0 / 30.0), "fold_stats": None,
              "sampled": 1000, "gids": None, "gnames": None, "search_ms": 1.0, "abundance_ms": 0.5}
    if tie_boot:
        counts.update({"tb": {"stats": stats * 0.5, "used": 4, "dropped": 0}, "tie_list": (12, 4000), "tie_bootstrap_ms": 0.25})
    return sample, counts


def _args(**kw):
    return dict(ARGS, coverage=False, min_breadth=None, depth_out=None, ties=True, curve=None, curve_genes=None, bootstrap=4, bootstrap_seed=None, bootstrap_groups=False,
                mixed_lengths=None, long_genes=False, gene_fold=None, **kw)


def test_files_with_and_without_the_switch(tmp_path):
    """the same records with and without the tie bootstrap's part: without it the file is byte for byte the file the writer wrote before the
    switch existed (its lines are spelled out here); with it, three columns behind every column and two header lines behind the four
    bootstrap lines - and write_table / read_table round-trip them"""
    seqs = ["A" * int(n) for n in LENGTH]
    sample, counts = _records(False)
    a = _args(bootstrap_ties=False, tie_list_factor=None)
    plain = abundance.build_table(a, sample, counts, NAMES, seqs, None)
    out = str(tmp_path / "plain.tsv")
    abundance.write_table(out, a, plain)
    before = open(out).read()
    lines = before.split("\n")
    assert lines[11:18] == ["# ties:\ton", "# reads_ambiguous:\t1", "# bootstrap:\t4", "# bootstrap_seed:\t0", "# bootstrap_replicates:\t4/4", "# bootstrap_denominator:\tfixed_ags",
                            "gene\tlength_aa\treads\taligned_aa\trpkg\tunique_reads\tcandidate_reads\tshared_reads\trpkg_shared\trpkg_boot_se\trpkg_ci95_low\trpkg_ci95_high"]
    assert "tie_bootstrap_ms" not in a and "rpkg_shared_boot_se" not in plain and [c for c, _ in abundance.table_columns(plain)][-1] == "rpkg_ci95_high"
    # a record from before the switch (no "tb" key at all) gives the same bytes
    old = {k: v for k, v in counts.items() if k != "tb"}
    abundance.write_table(out, _args(), abundance.build_table(_args(), sample, old, NAMES, seqs, None))
    assert open(out).read() == before
    sample, counts = _records(True)
    a = _args(bootstrap_ties=True, tie_list_factor=None)
    t = abundance.build_table(a, sample, counts, NAMES, seqs, None)
    assert a["tie_bootstrap_ms"] == 0.25 and t["tie_boot_used"] == 4 and t["tie_boot_stats"] is counts["tb"]["stats"]
    se, lo, hi = abundance.boot_columns(counts["tb"]["stats"], 4, LENGTH)
    for name, col in zip(abundance.TIE_BOOT_COLUMNS, (se, lo, hi)):
        assert GR.same_bits(t[name], col), name
    assert [c for c, _ in abundance.table_columns(t)][-6:] == list(abundance.BOOT_COLUMNS + abundance.TIE_BOOT_COLUMNS)
    out2 = str(tmp_path / "ties.tsv")
    abundance.write_table(out2, a, t)
    new = open(out2).read().split("\n")
    assert new[:17] == lines[:17] and new[17:19] == ["# bootstrap_ties:\ton", "# tie_list:\t12/4000"]
    assert new[19] == lines[17] + "\t" + "\t".join(abundance.TIE_BOOT_COLUMNS)
    assert [l.rsplit("\t", 3)[0] for l in new[20:23]] == lines[18:21] and new[23:] == [""] == lines[21:]            # the existing columns keep their text
    header, rows = abundance.read_table(out2)
    assert header["bootstrap_ties"] == "on" and header["tie_list"] == "12/4000" and len(rows) == 3 and len(rows[0]) == 15
    assert [r[-3:] for r in rows] == [[repr(float(x)) for x in v] for v in zip(se, lo, hi)]


def test_list_capacity_and_the_overflow_message():
    assert abundance.tie_list_capacity(1000, None) == 4000 and abundance.tie_list_capacity(1000, 1) == 1000 and abundance.tie_list_capacity(1 << 26, 500) == 1 << 27 == TR.MAXCAP
    assert abundance.MAX_TIE_LIST == TR.MAXCAP and abundance.MAX_TIE_FACTOR == oc.MAX_M8 == 500 and abundance.TIE_FACTOR == 4
    e = abundance.tie_list_overflow(2001 - 1000, 2001, 1000, 1)
    assert isinstance(e, abundance.AbundanceError)
    assert str(e) == "--bootstrap-ties: 1001 tie entries did not fit the list of 1000 (--tie-list-factor 1 x 1000 reads): --tie-list-factor 3 fits all 2001"
    assert "--tie-list-factor 2 fits all 2000" in str(abundance.tie_list_overflow(1000, 2000, 1000, 1))


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
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-ties needs --bootstrap B \(--bootstrap None\)"):
        abundance.run_abundance(request(bootstrap_ties=True, ties=True))
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-ties needs --ties \(--ties False\)"):
        abundance.run_abundance(request(bootstrap_ties=True, bootstrap=10))
    with pytest.raises(abundance.AbundanceError, match="--tie-list-factor 8 needs --bootstrap-ties"):
        abundance.run_abundance(request(tie_list_factor=8, bootstrap=10, ties=True))
    for bad, shown in ((0, "0"), (-1, "-1"), (501, "501"), (2.0, "2\\.0"), ("four", "four"), (True, "True")):
        with pytest.raises(abundance.AbundanceError, match="--tie-list-factor %s is not an integer from 1 to 500" % shown):
            abundance.run_abundance(request(bootstrap_ties=True, bootstrap=10, ties=True, tie_list_factor=bad))
    with pytest.raises(abundance.AbundanceError, match="bootstrap_ties 'yes' is not a switch"):
        abundance.run_abundance(request(bootstrap_ties="yes", bootstrap=10, ties=True))
    with pytest.raises(abundance.AbundanceError, match="--bootstrap 10 cannot be combined with --curve 4"):      # --curve stays refused
        abundance.run_abundance(request(bootstrap_ties=True, bootstrap=10, ties=True, curve=4))
    assert not os.path.exists(out)
    a = request()
    abundance.check_request(a)
    assert (a["bootstrap_ties"], a["tie_list_factor"]) == (False, None)          # off by default
    for f in (1, 500, np.int64(7), None):
        a = request(bootstrap_ties=True, bootstrap=10, ties=True, tie_list_factor=f, coverage=True)
        abundance.check_request(a)
        assert a["bootstrap_ties"] is True and a["tie_list_factor"] == (None if f is None else int(f))
    with pytest.raises(AssertionError, match="GPU work was started"):          # nothing to refuse: the request reaches the reader
        abundance.run_abundance(request(bootstrap_ties=True, bootstrap=10, ties=True, tie_list_factor=3))


def test_cli_switches():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv"])
    assert (a["bootstrap_ties"], a["tie_list_factor"]) == (False, None)
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--ties", "--bootstrap", "100", "--bootstrap-ties", "--tie-list-factor", "9"])
    assert (a["bootstrap_ties"], a["tie_list_factor"], a["ties"], a["bootstrap"]) == (True, 9, True, 100)
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--tie-list-factor", "four"])


def test_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mcensus.h")).read(), flags=re.S)
    for s in ("mc_set_tie_bootstrap", "mc_tie_bootstrap", "mc_tie_bootstrap_ms", "mc_tie_bootstrap_kernels_ms"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s), s
    for m in ("set_tie_bootstrap", "tie_bootstrap", "tie_bootstrap_ms", "tie_bootstrap_kernels_ms"):
        assert callable(getattr(_native.Engine, m))
    assert TR.MAXCAP == 1 << 27
