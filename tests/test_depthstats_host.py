"""The depth statistics, host side (no GPU): the rules of csrc/mc_depthstats.h compiled by g++ (tests/emul/depthstats.cpp, once more under
-fsanitize=address,undefined) against Python integers and the numpy restatement (tests/depthstats_restated.py) - cut, lo and hi for every
length 1 .. 600 and every P 1 .. 100, and the boundary arithmetic of a selection on the four counts of constant, two-valued and random depth
vectors; the restatement on fixed figures; the columns, their order, the gene without reads, the header lines, the round trip and the groups
and curve files through abundance's table builder and writers; every refusal before an engine is opened; the command line; and the new symbols
of the ABI."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import depthstats_restated as D
import order_cases as oc
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FQ = os.path.join(HERE, "golden", "inputs", "example.fq.gz")


# ---- the rules of mc_depthstats.h on the CPU -----------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "depthstats")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(HERE, "emul", "depthstats.cpp")])
    return exe


@pytest.fixture(scope="module", params=["O2", "sanitized"])
def driver(request, tmp_path_factory):
    return _build(tmp_path_factory, request.param, ["-O2"] if request.param == "O2" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, tmp, pairs, records, keeps):
    oc.write_sections(tmp / "in", [np.uint32(pairs).reshape(-1, 2), np.uint64(records).reshape(-1, 8), np.int64(keeps)])
    subprocess.check_call([exe, "run", str(tmp / "in"), str(tmp / "out")])
    out = oc.read_sections(tmp / "out")
    assert np.frombuffer(out[3], "<i4").tolist() == [4]
    return np.frombuffer(out[0], "<u4").reshape(-1, 4), np.frombuffer(out[1], "<u8"), np.frombuffer(out[2], "<i4").tolist()


def test_cut_lo_and_hi_for_every_length_and_percent(driver, tmp_path):
    pairs = [(n, P) for n in list(range(1, 601)) + [2047, 4095, 4096, 4097, 65535] for P in range(1, 101)]
    ranks, _, _ = _run(driver, tmp_path, pairs, [], [])
    for (n, P), (cut, lo, hi, med) in zip(pairs, ranks.tolist()):
        want = n * (100 - P) // 200
        assert (cut, lo, hi, med) == (want, want, n - want, (n - 1) // 2), (n, P)
        assert hi > lo and lo <= (n - 1) // 2 <= hi - 1, (n, P)
        assert (cut, lo, hi) == D.cut_lo_hi(n, P)
    at = {p: r for p, r in zip(pairs, ranks.tolist())}
    assert [at[(n, 99)][0] for n in (199, 200, 201)] == [0, 1, 1] and at[(400, 80)][:3] == [40, 40, 360] and at[(1, 1)][:3] == [0, 0, 1]
    assert all(at[(n, 100)][0] == 0 for n in range(1, 601))


def test_the_percents_that_are_refused(driver, tmp_path):
    keeps = [-1, 0, 1, 50, 80, 100, 101, 200, 1 << 40, -(1 << 40)]
    assert _run(driver, tmp_path, [], [], keeps)[2] == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0]


def _counts_of(d, keep):
    """what a selection ends with: low, high, lo, hi and the four exact counts of the header's boundary function"""
    d = np.asarray(d, np.uint64)
    x = np.sort(d)
    _, lo, hi = D.cut_lo_hi(len(d), keep)
    low, high = int(x[lo]), int(x[hi - 1])
    between = int(d[(d > low) & (d < high)].sum(dtype=np.uint64))
    return [low, high, lo, hi, int((d < low).sum()), int((d <= low).sum()), int((d < high).sum()), between]


def test_the_boundary_arithmetic_against_the_sorted_slice(driver, tmp_path):
    """constant, two-valued and random vectors of every length 1 .. 300; values around 0, 255 / 256 and 65,535 / 65,536; P of 1, 50, 80, 99, 100"""
    rng = np.random.default_rng(20261021)
    records, want = [], []
    for n in range(1, 301):
        vectors = [np.full(n, v) for v in (0, 255, 65536)]
        vectors += [rng.choice(pair, n) for pair in ((0, 1), (255, 256), (65535, 65536), (0, 70000))]
        vectors += [rng.integers(0, hi, n) for hi in (2, 7, 300, 70000, 1 << 32)]
        vectors += [np.concatenate([np.zeros(n - n // 10, np.int64), rng.integers(250, 260, n // 10)])]          # a pile on a tenth of the gene
        for d in vectors:
            for P in (1, 50, 80, 99, 100):
                records.append(_counts_of(d, P))
                want.append(D.of_depth(d, P)[1])
    _, sums, _ = _run(driver, tmp_path, [], records, [])
    assert sums.tolist() == want and len(want) == 300 * 13 * 5
    assert max(want) > 1 << 36, "sums far past 32 bits are among them"


def test_the_restatement_on_fixed_figures():
    """so that a restatement that degenerates is seen: a pile of 300 reads on 30 residues of a 400-residue gene; a staircase; the difference array"""
    pile = D.depth_of_spans([(0, 100, 129)] * 300, [400])
    assert D.of_depth(pile, 80) == (0, 0, 0, 0) and D.of_depth(pile, 100) == (0, 9000, 0, 300) and int(pile.max()) == 300
    stairs = np.repeat([0, 1, 2, 3, 4], [10, 30, 20, 30, 10])                  # 100 residues: lo = 10, hi = 90 at P = 80
    assert D.of_depth(stairs, 80) == (2, 30 + 40 + 90, 1, 3) and D.of_depth(stairs, 100) == (2, 200, 0, 4) and D.of_depth(stairs, 1) == (2, 4, 2, 2)
    assert D.of_depth([5], 80) == (5, 5, 5, 5) and D.of_depth([7, 3], 80) == (3, 10, 3, 7)
    diff = np.zeros(7 + 4, np.uint32)                                           # genes of 7 and 2 residues: 9 + 2 slots
    diff[[1, 4]] = (2, 0xFFFFFFFF)                                              # two reads on residues 1 .. 3, one of them to the gene's end
    diff[7] = 0xFFFFFFFF
    diff[8] = 1
    diff[10] = 0xFFFFFFFF
    depth = D.depth_of_diff(diff, [7, 2])
    assert depth.tolist() == [0, 2, 2, 2, 1, 1, 1, 1, 1]
    st = D.depth_stats(depth, [7, 2], [True, False], 100)
    assert [st[k].tolist() for k in D.FIGURES] == [[1, 0], [9, 0], [0, 0], [2, 0]], "a gene whose table holds no read has four zeros"
    assert D.invariants(st, [9, 0], [2, 0]) == [] and D.invariants(st, [8, 0], [2, 0]) == ["trimmed_sum <= spanned", "keep 100: trimmed_sum == spanned"]
    assert D.tad([9, 0], [7, 2], 100).tolist() == [9 / 7, 0.0] and D.tad([4], [100], 1).tolist() == [2.0]


# ---- the table -------------------------------------------------------------------------------------------------------------------------------------
NAMES, SEQS = ["g1", "g2", "g3"], ["M" * 120, "K" * 300, "V" * 50]
ARGS = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 0, "min_aln": 0, "min_bits": 0.0, "min_breadth": None, "bootstrap": None, "gene_fold": None, "groups": None,
        "curve": None}


def _records(keep=80, ties=False, curve=False, stats=True):
    """the two records build_table takes, made by hand: three genes, the second without reads"""
    z = lambda *v: np.array(v, np.int64)
    sample = {"ags": 2.6e6, "source": "--ags", "pargs": {}, "classes": None, "L": 100}
    c = dict.fromkeys(("ac", "gb", "gbg", "scale", "tb", "cb", "idn", "ds", "ds_any", "depth", "ti", "tcov", "cu", "points", "fold_stats", "gids", "gnames"))
    c.update({"ab": {"reads": z(5, 0, 2), "aligned": z(150, 0, 61), "searched": 10, "assigned": 7}, "sampled": 10,
              "cov": {"covered": z(100, 0, 31), "spanned": z(150, 0, 61), "max_depth": z(3, 0, 2)}})
    if ties:
        c["ti"] = {"unique": z(4, 0, 2), "candidates": z(5, 1, 2), "share": np.array([5 << 32, 0, 2 << 32], np.uint64) - np.array([1 << 31, 0, 0], np.uint64) + np.array([0, 1 << 31, 0], np.uint64),
                   "ambiguous": 1, "group_ambiguous": 0, "group_unique": z()}
        c["tcov"] = {"covered_any": z(100, 30, 31), "spanned_any": z(150, 30, 61), "max_depth_any": z(3, 1, 2)}
    if curve:
        c["cu"] = {"reads": np.array([[2, 0, 1], [5, 0, 2]], np.int64), "aligned": np.array([[60, 0, 30], [150, 0, 61]], np.int64), "covered": np.array([[50, 0, 20], [100, 0, 31]], np.int64), "beyond": 0}
        c["points"] = [5, 10]
    if stats:
        c["ds"] = {"median": z(1, 0, 2), "trimmed_sum": z(131, 0, 47), "low": z(0, 0, 0), "high": z(2, 0, 2), "keep": keep}
        if ties:
            c["ds_any"] = {"median": z(1, 0, 2), "trimmed_sum": z(133, 3, 47), "low": z(0, 0, 0), "high": z(2, 1, 2), "keep": keep}
    return sample, c


def _built(group_of=None, **kw):
    sample, c = _records(**kw)
    args = dict(ARGS)
    return args, abundance.build_table(args, sample, c, NAMES, SEQS, group_of)


def test_columns_their_order_and_a_gene_without_reads(tmp_path):
    args, t = _built()
    _, plain = _built(stats=False)
    out, out0 = str(tmp_path / "out.tsv"), str(tmp_path / "out0.tsv")
    abundance.write_table(out, args, t)
    abundance.write_table(out0, args, plain)
    lines, lines0 = open(out).read().split("\n"), open(out0).read().split("\n")
    nh = 12                                                          # (the eleven lines of every table and coverage: on)
    assert lines0[nh].startswith("gene\t") and lines[:nh] == lines0[:nh] and lines[nh:nh + 2] == ["# depth_stats:\ton", "# tad_keep:\t80"]
    assert lines[nh + 2] == lines0[nh] + "\tmedian_depth\ttad80\ttad80_per_ge", "behind every other column, no _any column without ties"
    body, body0 = [l.split("\t") for l in lines[nh + 3:-1]], [l.split("\t") for l in lines0[nh + 1:-1]]
    ncol = len(lines0[nh].split("\t"))
    assert [r[:ncol] for r in body] == body0, "the columns of a run without the switch: byte for byte"
    ge = t["genome_equivalents_sampled"]
    kept = [120 - 2 * (120 * 20 // 200), 300 - 2 * (300 * 20 // 200), 50 - 2 * (50 * 20 // 200)]
    assert kept == [96, 240, 40] and abundance.tad_kept([120, 300, 50], 80).tolist() == kept
    assert body[0][ncol:] == ["1", repr(131 / 96), repr(131 / 96 / ge)] and body[2][ncol:] == ["2", repr(47 / 40), repr(47 / 40 / ge)]
    assert body[1][ncol:] == ["0", "0.0", "0.0"], "a gene without reads"
    assert t["depth_stats"]["trimmed_sum"].tolist() == [131, 0, 47] and t["tad_keep"] == 80 and "depth_stats" not in plain and "tad_keep" not in plain
    assert np.array_equal(t["tad80"], D.tad([131, 0, 47], [120, 300, 50], 80))
    header, rows = abundance.read_table(out)
    assert header["depth_stats"] == "on" and header["tad_keep"] == "80" and header["coverage"] == "on" and rows == body
    header0, _ = abundance.read_table(out0)
    assert "depth_stats" not in header0 and "tad_keep" not in header0


def test_another_percent_names_the_columns(tmp_path):
    args, t = _built(keep=100)
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, args, t)
    header, rows = abundance.read_table(out)
    cols = open(out).read().split("\n")[14].split("\t")
    assert header["tad_keep"] == "100" and cols[-3:] == ["median_depth", "tad100", "tad100_per_ge"] and rows[0][-2] == repr(131 / 120)


def test_the_any_columns_appear_only_with_ties(tmp_path):
    args, t = _built(ties=True)
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, args, t)
    lines = open(out).read().split("\n")
    head = next(l for l in lines if l.startswith("gene\t")).split("\t")
    assert head[-5:] == ["median_depth", "tad80", "tad80_per_ge", "median_depth_any", "tad80_any"] and "breadth_any" in head[:-5]
    rows = abundance.read_table(out)[1]
    assert [r[-2:] for r in rows] == [["1", repr(133 / 96)], ["0", repr(3 / 240)], ["2", repr(47 / 40)]]
    assert t["depth_stats_any"]["trimmed_sum"].tolist() == [133, 3, 47]
    _, t0 = _built(ties=False)
    assert "median_depth_any" not in t0 and "tad80_any" not in t0 and "depth_stats_any" not in t0


def test_the_groups_and_curve_files_are_untouched(tmp_path):
    group_of = {"g1": "A", "g3": "A"}
    files = []
    for stats in (False, True):
        args, t = _built(group_of=group_of, curve=True, stats=stats)
        args["groups"] = "map.tsv"
        g, cu = str(tmp_path / ("g%d.tsv" % stats)), str(tmp_path / ("c%d.tsv" % stats))
        abundance.write_groups(g, args, t)
        abundance.write_curve(cu, args, t)
        files.append((open(g, "rb").read(), open(cu, "rb").read()))
        assert ("depth_stats" in t) == stats
    assert files[0] == files[1] and b"group\tgenes\treads\trpkg" in files[0][0] and b"sampled_reads\t" in files[0][1]


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------------
class _Started(AssertionError):
    pass


@pytest.fixture
def no_engine(monkeypatch):
    """an engine, a reader or run_pipeline: the first one that is asked for ends the run"""
    def boom(*a, **k):
        raise _Started("GPU work was started")

    class NoReader:
        def __init__(self, *a, **k):
            boom()

        @classmethod
        def with_classes(cls, paths, class_len, *a, **k):
            raise _Started("class reader %s" % list(class_len))
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", NoReader)
    monkeypatch.setattr(microbe_census, "run_pipeline", lambda a: (_ for _ in ()).throw(_Started("run_pipeline")))
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_refusals_before_any_gpu_work(tmp_path, no_engine, monkeypatch):
    good = tmp_path / "good.faa"
    good.write_text(">g1 x\n%s\n>g2 y\n%s\n" % ("MKV" * 20, "MLA" * 30))
    out = str(tmp_path / "out.tsv")

    def base(**kw):
        args = {"seqfiles": [FQ], "genes": str(good), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return args
    for bad, shown in ((0, "0"), (101, "101"), (-80, "-80"), (True, "True"), (80.0, r"80\.0"), ("80", "80"), ([80], r"\[80\]")):
        with pytest.raises(abundance.AbundanceError, match=r"--tad-keep %s is not an integer from 1 to 100" % shown):
            abundance.run_abundance(base(tad_keep=bad))
    for bad in ("yes", 2, None, 1.5):
        with pytest.raises(abundance.AbundanceError, match=r"depth_stats %s is not a switch: True or False" % repr(bad).replace(".", r"\.")):
            abundance.run_abundance(base(depth_stats=bad))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(abundance.AbundanceError, match=r"not computed by a distributed run \(WORLD_SIZE 2\)"):
        abundance.run_abundance(base(depth_stats=True))
    monkeypatch.delenv("WORLD_SIZE")
    assert not os.path.exists(out)
    # what is accepted reaches the device: tad_keep implies depth_stats, both imply coverage, and the default percent is 80
    for kw, keep in ((dict(depth_stats=True), 80), (dict(tad_keep=1), 1), (dict(tad_keep=100), 100), (dict(depth_stats=True, tad_keep=np.int64(50)), 50), (dict(depth_stats=1), 80)):
        args = base(**kw)
        with pytest.raises(_Started, match="GPU work was started"):
            abundance.run_abundance(args)
        assert args["depth_stats"] is True and args["coverage"] is True and args["tad_keep"] == keep and type(args["tad_keep"]) is int
    # the switches off leave the request as it was: no coverage, no percent
    for kw in (dict(), dict(depth_stats=False), dict(depth_stats=0)):
        args = base(**kw)
        with pytest.raises(_Started, match="GPU work was started"):
            abundance.run_abundance(args)
        assert args["depth_stats"] is False and args["tad_keep"] is None and args["coverage"] is False and args["identity"] is False


def test_cli_switches(capsys):
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["x.fq", "g.faa", "o.tsv"]
    a = cli.parse_arguments(base)
    assert a["depth_stats"] is False and a["tad_keep"] is None
    a = cli.parse_arguments(base + ["--depth-stats"])
    assert a["depth_stats"] is True and a["tad_keep"] is None
    a = cli.parse_arguments(base + ["--tad-keep", "90"])
    assert a["depth_stats"] is False and a["tad_keep"] == 90        # (check_request turns the switch on)
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--tad-keep", "80.0"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.parse_arguments(["--help"])
    text = capsys.readouterr().out
    assert e.value.code == 0 and "--depth-stats" in text and "--tad-keep P" in text


def test_the_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "mcensus.h")).read()
    for name in ("mc_depth_stats", "mc_depth_stats_ms"):
        assert name + "(" in text and name in _native.EXPORTED_SYMBOLS
    for m in ("depth_stats", "depth_stats_ms"):
        assert hasattr(_native.Engine, m)
    src = open(os.path.join(REPO, "microbecensus_amd", "csrc", "mc_depthstats.h")).read()
    assert "#include <hip" not in src and "hip_runtime" not in src, "mc_depthstats.h is shared with g++"
