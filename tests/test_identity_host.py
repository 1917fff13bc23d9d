"""The identity of the assigned reads, host side (no GPU): the rules of csrc/mc_identity.h compiled by g++ (tests/emul/identity.cpp, once more
under -fsanitize=address,undefined) against the plain-Python restatement (tests/identity_restated.py) - the bin function and the median, min /
max and level functions on the histograms that can go wrong; the restatement on the reference binary's m8 golden under the cut-off sets of
tests/test_gpu_coverage.py, with the figures it must give; the columns, NA rows, header lines, groups columns and the --ident-out round trip;
every refusal before an engine is opened; the command line; and the new symbols of the ABI."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import identity_restated as I
import order_cases as oc
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
FQ = os.path.join(GOLD, "inputs", "example.fq.gz")
CUTS = [dict(), dict(min_ident=60, min_aln=30)]                    # test_gpu_coverage.py's two


# ---- the rules of mc_identity.h on the CPU ---------------------------------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "identity")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(HERE, "emul", "identity.cpp")])
    return exe


@pytest.fixture(scope="module", params=["O2", "sanitized"])
def driver(request, tmp_path_factory):
    return _build(tmp_path_factory, request.param, ["-O2"] if request.param == "O2" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, tmp, pairs, hists, levels):
    oc.write_sections(tmp / "in", [np.int32(pairs).reshape(-1, 2), np.uint32(hists).reshape(-1, I.BINS), np.int32(levels)])
    subprocess.check_call([exe, "run", str(tmp / "in"), str(tmp / "out")])
    out = oc.read_sections(tmp / "out")
    bad, nbins, nlev = np.frombuffer(out[2], "<i4").tolist()
    assert nbins == I.BINS == abundance.IDENT_BINS and nlev == abundance.MAX_IDENT_LEVELS
    nl = len(levels) if bad < 0 else 0
    return np.frombuffer(out[0], "<i4").tolist(), np.frombuffer(out[1], "<i8").reshape(-1, 4 + nl), bad


def _hist(**bins):
    h = np.zeros(I.BINS, np.uint32)
    for b, c in bins.items():
        h[int(b[1:])] = c
    return h


def test_the_bin_function(driver, tmp_path):
    pairs = [(0, 30), (30, 30), (0, 0), (5, 0), (99, 100), (199, 200), (1, 3), (2, 3), (59, 60), (29, 30), (1, 170), (170, 170), (35, 30), (-1, 30)]
    bins, _, _ = _run(driver, tmp_path, pairs, [], [])
    assert bins[:6] == [0, 100, 0, 0, 99, 99] and bins[6:12] == [33, 66, 98, 96, 0, 100]
    assert bins == [I.bin_of(m, a) for m, a in pairs]
    assert bins[12:] == [100, 0]                                   # (no row of the engine: the nearest bin, never one outside the gene's)
    grid = [(m, a) for a in range(0, 171) for m in range(0, a + 1)]
    bins, _, _ = _run(driver, tmp_path, grid, [], [])
    assert bins == [0 if a < 1 else (100 * m) // a for m, a in grid] and min(bins) == 0 and max(bins) == 100


def test_the_figures_of_one_histogram(driver, tmp_path):
    """one read; two reads in one bin; two reads in bins 0 and 100; n even and n odd; counts only in bins 63, 64 and 65; no read; a level of 0
    (which equals reads) and a level of 100"""
    hists = [_hist(b90=1), _hist(b77=2), _hist(b0=1, b100=1), _hist(b10=1, b20=1, b30=1, b40=1), _hist(b10=1, b20=1, b30=1, b40=1, b50=1), _hist(b63=2, b64=1, b65=2),
             _hist(b63=3, b64=2, b65=1), _hist(b63=1, b65=3), _hist(b63=1, b64=1), _hist(), _hist(b0=7), _hist(b100=9), _hist(b99=4000000000, b100=4000000000)]
    levels = [0, 1, 63, 64, 65, 66, 100]
    _, figs, bad = _run(driver, tmp_path, [], hists, levels)
    assert bad == -1
    want = [I.figures_of_hist(h, levels) for h in hists[:-1]]       # (the last: 8e9 reads, not restated read by read)
    assert [tuple(r[1:4]) for r in figs[:-1].tolist()] == [w[:3] for w in want]
    assert [r[4:] for r in figs[:-1].tolist()] == [w[3] for w in want] and figs[:-1, 0].tolist() == [int(h.sum()) for h in hists[:-1]]
    assert [tuple(r[1:4]) for r in figs.tolist()[:10]] == [(90, 90, 90), (77, 77, 77), (0, 0, 100), (10, 20, 40), (10, 30, 50), (63, 64, 65), (63, 63, 65), (63, 65, 65), (63, 63, 64), (-1, -1, -1)]
    assert figs[9].tolist() == [0, -1, -1, -1] + [0] * 7
    assert figs[5, 4:].tolist() == [5, 5, 5, 3, 2, 0, 0] and figs[10, 4:].tolist() == [7, 0, 0, 0, 0, 0, 0] and figs[11, 4:].tolist() == [9] * 7
    assert (figs[:, 4] == figs[:, 0]).all(), "a level of 0 equals reads"
    assert figs[12].tolist() == [8000000000, 99, 99, 100, 8000000000, 8000000000, 8000000000, 8000000000, 8000000000, 8000000000, 4000000000]   # (64-bit on the host)


def test_the_levels_that_are_refused(driver, tmp_path):
    for levels, bad in (([], -1), ([0], -1), ([100], -1), ([0, 1, 2, 3, 4, 5, 6, 100], -1), ([-1], 0), ([101], 0), ([50, 50], 1), ([50, 40], 1), ([10, 20, 30, 25], 3), ([10, 200], 1)):
        assert _run(driver, tmp_path, [], [_hist(b5=1)], levels)[2] == bad, levels


# ---- the restatement on the reference binary's m8 ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    names, seqs = _native.load_markers()
    rows = I.rows_from_m8(os.path.join(GOLD, "config1_example_fq.m8.gz"), names)
    return names, rows


def test_the_restatement_on_the_reference_m8(golden):
    """the figures the issue fixed, so that a restatement that degenerates is seen"""
    import abundance_restated as R
    names, rows = golden
    levels = [0, 50, 90, 100]
    none, cut = (I.identity(rows, len(names), levels, **c) for c in CUTS)
    ab = [R.abundance([r[:6] for r in rows], len(names), **c) for c in CUTS]
    h = none["hist"].astype(np.int64)
    per_bin = h.sum(axis=0)
    assert int(h.sum()) == 251 == ab[0]["assigned"] and int((h.sum(axis=1) > 0).sum()) == 239
    assert int((per_bin > 0).sum()) == 50 and np.flatnonzero(per_bin).tolist()[0] == 28 and np.flatnonzero(per_bin).tolist()[-1] == 100 and int(per_bin[100]) == 20
    assert int(((h > 0).sum(axis=1) >= 2).sum()) == 6 and int(((h.sum(axis=1) > 0) & (h.sum(axis=1) % 2 == 0)).sum()) == 10
    hc = cut["hist"].astype(np.int64)
    assert int(hc.sum()) == 23 == ab[1]["assigned"] and int((hc.sum(axis=1) > 0).sum()) == 22
    assert np.flatnonzero(hc.sum(axis=0)).tolist()[0] == 66 and np.flatnonzero(hc.sum(axis=0)).tolist()[-1] == 100
    for idn, a in ((none, ab[0]), (cut, ab[1])):
        assert I.invariants(idn, a["reads"], a["aligned"], levels) == []
        assert [I.figures_of_hist(hh, levels) for hh in idn["hist"][idn["hist"].any(axis=1)]] == [
            (int(lo), int(md), int(hi), g.tolist()) for lo, md, hi, g, n in zip(idn["ident_min"], idn["ident_median"], idn["ident_max"], idn["ge"], idn["hist"].sum(axis=1)) if n]
        assert int(idn["matched"].sum()) + int(idn["mismatched"].sum()) <= int(a["aligned"].sum())      # (the rest lies opposite gaps)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def _table(levels=(50, 90)):
    length = np.array([120, 300, 50], np.int64)
    ge = 10 * 100 / 2.6e6
    reads, aligned = np.array([5, 0, 2], np.int64), np.array([150, 0, 61], np.int64)
    idn = {"matched": np.array([140, 0, 33], np.int64), "mismatched": np.array([9, 0, 27], np.int64), "gap_opens": np.array([1, 0, 0], np.int64),
           "ident_min": np.array([80, -1, 50], np.int32), "ident_median": np.array([95, -1, 50], np.int32), "ident_max": np.array([100, -1, 58], np.int32),
           "levels": list(levels), "ge": np.array([[5, 4], [0, 0], [2, 0]], np.int64)[:, :len(levels)],
           "hist": np.zeros((3, 101), np.uint32)}
    idn["hist"][0, [80, 95, 100]] = (1, 2, 2)
    idn["hist"][2, [50, 58]] = (1, 1)
    t = {"gene": ["g1", "g2", "g3"], "length_aa": length, "reads": reads, "aligned_aa": aligned, "rpkg": abundance.rpkg(reads, length, ge), "sampled_reads": 10,
         "trimmed_length": 100, "ags": 2.6e6, "ags_source": "--ags", "genome_equivalents_sampled": ge, "reads_assigned": 7}
    with_id = dict(t)
    with_id.update(abundance.identity_columns(idn, reads, aligned, length, ge))
    with_id.update({"identity": idn, "ident_levels": list(levels)})
    return t, with_id, ge


def test_columns_na_rows_and_header_lines(tmp_path):
    args = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 0, "min_aln": 0, "min_bits": 0.0}
    plain, t, ge = _table()
    out, out0 = str(tmp_path / "out.tsv"), str(tmp_path / "out0.tsv")
    abundance.write_table(out, args, t)
    abundance.write_table(out0, args, plain)
    lines, lines0 = open(out).read().split("\n"), open(out0).read().split("\n")
    nh = 11
    assert lines[:nh] == lines0[:nh] and lines[nh:nh + 2] == ["# identity:\ton", "# ident_levels:\t50,90"]
    assert lines[nh + 2] == lines0[nh] + "\tmatched_aa\tmismatched_aa\tgap_opens\tident_mean\tident_median\tident_min\tident_max\treads_ident_ge50\trpkg_ident_ge50\treads_ident_ge90\trpkg_ident_ge90"
    body, body0 = [l.split("\t") for l in lines[nh + 3:-1]], [l.split("\t") for l in lines0[nh + 1:-1]]
    assert [r[:5] for r in body] == body0, "the columns of a run without the switch: byte for byte"
    assert body[0][5:] == ["140", "9", "1", repr(100.0 * 140 / 150), "95", "80", "100", "5", repr(float(abundance.rpkg(5, 120, ge))), "4", repr(float(abundance.rpkg(4, 120, ge)))]
    assert body[1][5:] == ["0", "0", "0", "NA", "NA", "NA", "NA", "0", "0.0", "0", "0.0"], "a gene without reads"
    assert body[2][5:9] == ["33", "27", "0", repr(100.0 * 33 / 61)] and body[2][9:12] == ["50", "50", "58"]
    header, rows = abundance.read_table(out)
    assert header["identity"] == "on" and header["ident_levels"] == "50,90" and len(rows) == 3
    # without levels: no level line, no level columns
    _, t0, _ = _table(levels=())
    abundance.write_table(out, args, t0)
    lines = open(out).read().split("\n")
    assert lines[nh] == "# identity:\ton" and lines[nh + 1].endswith("\tident_min\tident_max") and not any(l.startswith("# ident_levels") for l in lines)


def test_groups_columns(tmp_path):
    args = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 0, "min_aln": 0, "min_bits": 0.0, "groups": "map.tsv"}
    plain, t, ge = _table()
    group_of = {"g1": "A", "g3": "A"}                             # g2: a group of its own name, without reads
    for tab in (plain, t):
        tab["groups"] = abundance.group_table(tab["gene"], tab["reads"], tab["rpkg"], group_of)
    t["groups_ident"] = abundance.group_ident_table(t["gene"], group_of, t)
    out, out0 = str(tmp_path / "g.tsv"), str(tmp_path / "g0.tsv")
    abundance.write_groups(out, args, t)
    abundance.write_groups(out0, args, plain)
    lines, lines0 = open(out).read().split("\n"), open(out0).read().split("\n")
    nh = 12
    assert lines[:nh] == lines0[:nh] and lines[nh:nh + 2] == ["# identity:\ton", "# ident_levels:\t50,90"]
    assert lines[nh + 2] == lines0[nh] + "\tmatched_aa\tident_mean\treads_ident_ge50\trpkg_ident_ge50\treads_ident_ge90\trpkg_ident_ge90"
    body, body0 = [l.split("\t") for l in lines[nh + 3:-1]], [l.split("\t") for l in lines0[nh + 1:-1]]
    assert [r[:4] for r in body] == body0 and [r[0] for r in body] == ["A", "g2"]
    r50 = float(abundance.rpkg(5, 120, ge)) + float(abundance.rpkg(2, 50, ge))          # the members' values, added in FASTA order
    assert body[0][4:] == ["173", repr(100.0 * 173 / 211), "7", repr(r50), "4", repr(float(abundance.rpkg(4, 120, ge)) + 0.0)]
    assert body[1][4:] == ["0", "NA", "0", "0.0", "0", "0.0"]


def test_ident_out_round_trip(tmp_path):
    _, t, _ = _table()
    path = str(tmp_path / "ident.tsv")
    abundance.write_ident(path, t["gene"], t["identity"]["hist"])
    assert open(path).read() == "#gene\tident\treads\ng1\t80\t1\ng1\t95\t2\ng1\t100\t2\ng3\t50\t1\ng3\t58\t1\n"      # FASTA order, bins ascending, only genes with reads
    back = abundance.read_ident(path, t["gene"])
    assert back.dtype == np.uint32 and np.array_equal(back, t["identity"]["hist"])
    assert [I.figures_of_hist(h, (50, 90))[:3] for h in back] == [(80, 95, 100), (-1, -1, -1), (50, 50, 58)]


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------
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
    (tmp_path / "map.tsv").write_text("g1\tA\n")
    out = str(tmp_path / "out.tsv")

    def run(**kw):
        args = {"seqfiles": [FQ], "genes": str(good), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return abundance.run_abundance(args), args
    for lv, shown in (([], ""), (list(range(9)), "0,1,2,3,4,5,6,7,8"), ([101], "101"), ([-1, 5], "-1,5"), ([50, 50], "50,50"), ([90, 80], "90,80"), ([50.0], "50.0"), ([True], "True"),
                      ("50", "50"), (50, "50")):
        with pytest.raises(abundance.AbundanceError, match=r"--ident-levels %s is not a list of 1 to 8 integer percents from 0 to 100, strictly ascending" % shown.replace(".", r"\.")):
            run(ident_levels=lv)
    with pytest.raises(abundance.AbundanceError, match=r"--ident-out '' is an empty path"):
        run(ident_out="")
    with pytest.raises(abundance.AbundanceError, match=r"--ident-out .*out\.tsv is the path of the gene table itself: two files"):
        run(ident_out=out)
    with pytest.raises(abundance.AbundanceError, match=r"--ident-out .*out\.tsv\.groups\.tsv is the path of the groups table"):
        run(ident_out=out + ".groups.tsv", groups=str(tmp_path / "map.tsv"))
    with pytest.raises(abundance.AbundanceError, match=r"--ident-out .*out\.tsv\.curve\.tsv is the path of the curve table"):
        run(ident_out=out + ".curve.tsv", curve=4)
    with pytest.raises(abundance.AbundanceError, match=r"--ident-out .*d\.tsv is the path of the depth file \(--depth-out\)"):
        run(ident_out=str(tmp_path / "d.tsv"), depth_out=str(tmp_path / "x" / ".." / "d.tsv"))
    with pytest.raises(abundance.AbundanceError, match=r"--ident-out .*m\.tsv is the path of the curve's per-gene matrix \(--curve-genes\)"):
        run(ident_out=str(tmp_path / "m.tsv"), curve=4, curve_genes=str(tmp_path / "m.tsv"))
    for bad in ("yes", 2, None, 1.5):
        with pytest.raises(abundance.AbundanceError, match=r"identity %s is not a switch: True or False" % repr(bad).replace(".", r"\.")):
            run(identity=bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(abundance.AbundanceError, match=r"not computed by a distributed run \(WORLD_SIZE 2\)"):
        run(identity=True)
    monkeypatch.delenv("WORLD_SIZE")
    assert not os.path.exists(out)
    # what is accepted reaches the device - and the two other switches imply the first
    for kw in (dict(identity=True), dict(ident_levels=[0, 100]), dict(ident_out=str(tmp_path / "i.tsv")), dict(ident_out=out + ".groups.tsv"), dict(ident_out=out + ".curve.tsv"), dict()):
        args = {"seqfiles": [FQ], "genes": str(good), "outfile": out, "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        with pytest.raises(_Started, match="GPU work was started"):
            abundance.run_abundance(args)
        assert args["identity"] is bool(kw)


def test_cli_switches():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["x.fq", "g.faa", "o.tsv"]
    a = cli.parse_arguments(base)
    assert a["identity"] is False and a["ident_levels"] is None and a["ident_out"] is None
    a = cli.parse_arguments(base + ["--identity", "--ident-levels", "50,90", "--ident-out", "i.tsv"])
    assert a["identity"] is True and a["ident_levels"] == [50, 90] and a["ident_out"] == "i.tsv"
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--ident-levels", "50,x"])


def test_the_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "mcensus.h")).read()
    for name in ("mc_set_identity", "mc_identity_read", "mc_identity_hist", "mc_identity_ms", "mc_identity_scan_ms"):
        assert name + "(" in text and name in _native.EXPORTED_SYMBOLS
    for m in ("set_identity", "identity", "identity_hist", "identity_ms"):
        assert hasattr(_native.Engine, m)
    src = open(os.path.join(REPO, "microbecensus_amd", "csrc", "mc_identity.h")).read()
    assert "#include <hip" not in src and "hip_runtime" not in src, "mc_identity.h is shared with g++"
