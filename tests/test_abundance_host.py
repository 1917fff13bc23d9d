"""Gene abundances, host side (no GPU): the restatement of the statement on a hand-made m8, the RPKG and group arithmetic, the table
and header format, --ags-report parsing, every refusal of run_abundance before an engine is opened, and the command line."""
import gzip
import importlib.util
import os

import numpy as np
import pytest

import abundance_restated as R
from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

NAMES = ["gA", "gB", "gC", "gD"]


def _m8(rows):
    return "".join("%s\t%s\t%g\t%d\t0\t0\t1\t2\t3\t4\t%g\t%g\n" % r for r in rows)


# query, subject, identity, alnlen, log(e), bits
HAND = _m8([
    ("r0", "gA", 50.0, 40, -3.0, 60.0),        # tie on bits with the next row: the first wins
    ("r0", "gB", 100.0, 45, -3.0, 60.0),
    ("r0", "gC", 80.0, 30, -1.0, 40.0),
    ("r1", "gB", 59.5238, 42, -2.0, 55.0),     # 25 / 42 identical: fails min_ident 60 only
    ("r1", "gC", 61.9048, 42, -2.0, 50.0),     # 26 / 42
    ("r2", "gD", 90.0, 20, -2.0, 70.0),        # fails min_aln 25 only
    ("r2", "gA", 90.0, 30, -2.0, 45.0),
    ("r3", "gD", 90.0, 30, -2.0, 29.5),        # fails min_bits 30 only
    ("r3", "gB", 90.0, 30, -2.0, 30.0),        # bits == min_bits: passes (>=)
    ("r4", "gC", 90.0, 30, 0.5, 80.0),         # fails max_loge 0 only
    ("r4", "gC", 87.0968, 31, 0.0, 35.0),        # loge == max_loge: passes (<=)
    ("r5", "gA", 20.0, 10, 0.9, 10.0),         # no passing row under the cut-offs
])


def test_restatement_on_a_hand_made_m8():
    rows = R.rows_from_m8(HAND, NAMES)
    assert [r[2] for r in rows] == [20, 45, 24, 25, 26, 18, 27, 27, 27, 27, 27, 2]
    none = R.abundance(rows, 4)
    #   r0: gA (the tie's first row)   r1: gB   r2: gD   r3: gB (30.0 over 29.5)   r4: gC (80 bits)   r5: gA
    assert none["reads"].tolist() == [2, 2, 1, 1] and none["aligned"].tolist() == [40 + 10, 42 + 30, 30, 20] and none["assigned"] == 6
    cut = R.abundance(rows, 4, min_ident=60, min_aln=25, min_bits=30.0, max_loge=0.0)
    #   r0: gB (gA's 50 % fails, gB 60 bits first among the rest)   r1: gC   r2: gA   r3: gB   r4: gC (35 bits)   r5: none
    assert cut["reads"].tolist() == [1, 2, 2, 0] and cut["aligned"].tolist() == [30, 45 + 30, 42 + 31, 0] and cut["assigned"] == 5
    # each cut-off on its own moves exactly the read built for it
    assert R.abundance(rows, 4, min_ident=60)["reads"].tolist() == [0, 2, 2, 1]       # r0 -> gB, r1 -> gC, r5 lost
    assert R.abundance(rows, 4, min_aln=25)["reads"].tolist() == [2, 2, 1, 0]         # r2 -> gA, r5 lost
    assert R.abundance(rows, 4, min_bits=29.75)["reads"].tolist() == [1, 2, 1, 1]     # r3 stays gB, r5 lost
    assert R.abundance(rows, 4, min_bits=30.0)["aligned"].tolist() == [40, 72, 30, 20]
    assert R.abundance(rows, 4, max_loge=0.0)["reads"].tolist() == [1, 2, 1, 1]       # r4 stays gC, by its 35-bit row of 31 residues; r5 lost
    assert R.abundance(rows, 4, max_loge=0.0)["aligned"].tolist() == [40, 72, 31, 20]
    assert R.abundance(rows, 4, min_bits=60.5)["reads"].tolist() == [0, 0, 1, 1]      # r2's 70 and r4's 80 bits alone
    # the tie: the first row in file order wins, whichever subject it names
    swapped = R.rows_from_m8(_m8([("r0", "gB", 100.0, 45, -3.0, 60.0), ("r0", "gA", 50.0, 40, -3.0, 60.0)]), NAMES)
    assert R.abundance(swapped, 4)["reads"].tolist() == [0, 1, 0, 0]
    # the same rows as an mc_row array
    arr = np.zeros(len(rows), _native.ROW_DTYPE)
    for i, (q, s, nm, al, bits, loge) in enumerate(rows):
        arr[i] = (int(q[1:]), s, nm * 100.0 / al, al, 0, 0, 1, 2, 3, 4, loge, bits, 0, nm)
    got = R.abundance(R.rows_from_array(arr), 4, min_ident=60, min_aln=25, min_bits=30.0, max_loge=0.0)
    assert got["reads"].tolist() == cut["reads"].tolist() and got["aligned"].tolist() == cut["aligned"].tolist() and got["assigned"] == 5
    assert not R.cutoffs_clear_of_printed_values(rows, min_bits=30.0) and R.cutoffs_clear_of_printed_values(rows, min_bits=31.0, max_loge=2.0)


def test_rpkg_and_group_arithmetic_by_hand():
    ge = abundance.genome_equivalents(1000, 100, 4.0e6)
    assert ge == 0.025
    v = abundance.rpkg([3, 0, 10], [100, 50, 1000], ge)
    assert v.tolist() == [3 / 0.3 / 0.025, 0.0, 10 / 3.0 / 0.025] and v.tolist()[0] == 400.0
    names = ["a", "b", "c", "d"]
    rp = [0.1, 0.2, 0.3, 0.7]
    groups = abundance.group_table(names, [1, 2, 3, 4], rp, {"c": "G1", "a": "G1", "d": "G2"})
    assert groups == [("G1", 2, 4, 0.1 + 0.3), ("b", 1, 2, 0.2), ("G2", 1, 4, 0.7)]
    assert abundance.group_table(names, [1, 2, 3, 4], rp, {n: "all" for n in names}) == [("all", 4, 10, ((0.1 + 0.2) + 0.3) + 0.7)]


def _table():
    ge = abundance.genome_equivalents(8672, 100, 3051745.7641809303)
    reads, length = np.array([5, 0, 7], np.int64), np.array([120, 300, 2047], np.int64)
    return {"gene": ["g1", "g2", "g3"], "length_aa": length, "reads": reads, "aligned_aa": np.array([150, 0, 231], np.int64), "rpkg": abundance.rpkg(reads, length, ge),
            "sampled_reads": 8672, "trimmed_length": 100, "ags": 3051745.7641809303, "ags_source": "run_pipeline", "genome_equivalents_sampled": ge, "reads_assigned": 12}


def test_table_and_header_format(tmp_path):
    args = {"seqfiles": ["a.fq.gz", "b.fq.gz"], "genes": "genes.faa", "min_ident": 60, "min_aln": 30, "min_bits": 35.5, "groups": "map.tsv"}
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, args, t)
    lines = open(out).read().split("\n")
    assert lines[:11] == ["# metagenome:\ta.fq.gz,b.fq.gz", "# genes:\tgenes.faa", "# sampled_reads:\t8672", "# trimmed_length:\t100", "# min_ident:\t60", "# min_aln:\t30",
                          "# min_bits:\t35.5", "# average_genome_size:\t3051745.7641809303", "# ags_source:\trun_pipeline",
                          "# genome_equivalents_sampled:\t%r" % (8672 * 100 / 3051745.7641809303), "# reads_assigned:\t12"]
    assert lines[11] == "gene\tlength_aa\treads\taligned_aa\trpkg"
    assert lines[12] == "g1\t120\t5\t150\t%r" % (5 / (3 * 120 / 1000.0) / t["genome_equivalents_sampled"])
    assert lines[13] == "g2\t300\t0\t0\t0.0" and lines[14].startswith("g3\t2047\t7\t231\t") and lines[15:] == [""]
    header, rows = abundance.read_table(out)
    assert float(header["average_genome_size"]) == t["ags"] and float(header["genome_equivalents_sampled"]) == t["genome_equivalents_sampled"]
    assert [float(r[4]) for r in rows] == t["rpkg"].tolist()              # repr round-trips: the file holds the values bit for bit
    t["groups"] = abundance.group_table(t["gene"], t["reads"], t["rpkg"], {"g1": "X", "g3": "X"})
    abundance.write_groups(out + ".groups.tsv", args, t)
    header, rows = abundance.read_table(out + ".groups.tsv")
    assert header["groups"] == "map.tsv" and header["reads_assigned"] == "12"
    assert rows == [["X", "2", "12", repr(float(t["rpkg"][0]) + float(t["rpkg"][2]))], ["g2", "1", "0", "0.0"]]


def test_ags_report_parsing(tmp_path):
    rep = str(tmp_path / "report.txt")
    args = {"outfile": rep, "seqfiles": ["x.fq"], "sampled_reads": 8672, "read_length": 100, "min_quality": -5, "mean_quality": -5, "filter_dups": False, "max_unknown": 100}
    microbe_census.report_results(args, 3051745.7641809303, 980306)
    assert abundance.read_ags_report(rep) == 3051745.7641809303
    (tmp_path / "ref.txt").write_text("Parameters\nmetagenome:\tx\n\nResults\naverage_genome_size:\t2500000.5\ntotal_bases:\t5\ngenome_equivalents:\t0.1\n")
    assert abundance.read_ags_report(str(tmp_path / "ref.txt")) == 2500000.5
    (tmp_path / "none.txt").write_text("Results\ntotal_bases:\t5\n")
    with pytest.raises(abundance.AbundanceError, match="no average_genome_size line"):
        abundance.read_ags_report(str(tmp_path / "none.txt"))
    (tmp_path / "bad.txt").write_text("average_genome_size:\tNA?\n")
    with pytest.raises(abundance.AbundanceError, match="'NA\\?' is not a number"):
        abundance.read_ags_report(str(tmp_path / "bad.txt"))
    with pytest.raises(abundance.AbundanceError, match="not found"):
        abundance.read_ags_report(str(tmp_path / "missing.txt"))


# ---- refusals, before any engine is opened ----------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Reader", boom)
    monkeypatch.setattr(microbe_census, "run_pipeline", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _faa(path, recs, gz=False):
    with (gzip.open(path, "wt") if gz else open(path, "w")) as f:
        for n, s in recs:
            f.write(">%s some description\n%s\n" % (n, s))
    return str(path)


def test_refusals_before_any_gpu_work(tmp_path, no_engine, monkeypatch):
    fq = os.path.join(HERE, "golden", "inputs", "example.fq.gz")
    good = _faa(tmp_path / "good.faa", [("g1", "MKV" * 20), ("g2", "MLA" * 30)])

    def run(**kw):
        args = {"seqfiles": [fq], "genes": good, "outfile": str(tmp_path / "out.tsv"), "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return abundance.run_abundance(args)
    with pytest.raises(abundance.AbundanceError, match="holds 32768 sequences: more than 32767"):
        run(genes=_faa(tmp_path / "many.faa.gz", [("g%d" % i, "MKVL") for i in range(32768)], gz=True))
    with pytest.raises(abundance.AbundanceError, match="Gene long1 is 2048 residues long: longer than 2047"):
        run(genes=_faa(tmp_path / "long.faa", [("g1", "MKV"), ("long1", "A" * 2048)]))
    (tmp_path / "empty.faa").write_text("")
    with pytest.raises(abundance.AbundanceError, match="empty.faa is empty"):
        run(genes=str(tmp_path / "empty.faa"))
    (tmp_path / "blank.faa").write_text("\n\n")
    with pytest.raises(abundance.AbundanceError, match="is empty"):
        run(genes=str(tmp_path / "blank.faa"))
    with pytest.raises(abundance.AbundanceError, match="Gene name g1 occurs more than once"):
        run(genes=_faa(tmp_path / "dup.faa", [("g1", "MKV"), ("g2", "MKV"), ("g1", "MLL")]))
    with pytest.raises(abundance.AbundanceError, match="--ags 3000000.0 and --ags-report r.txt cannot be combined"):
        run(ags_report="r.txt")
    for bad in (0, -2.5e6, float("nan"), float("inf")):
        with pytest.raises(abundance.AbundanceError, match="The AGS .* is not a positive finite number"):
            run(ags=bad)
    (tmp_path / "zero.txt").write_text("average_genome_size:\t0.0\n")
    with pytest.raises(abundance.AbundanceError, match=r"The AGS 0.0 \(report .*zero.txt\) is not a positive"):
        run(ags=None, ags_report=str(tmp_path / "zero.txt"))
    (tmp_path / "map.tsv").write_text("g1\tX\nghost\tX\n")
    with pytest.raises(abundance.AbundanceError, match="line 2: gene ghost is not in the gene FASTA"):
        run(groups=str(tmp_path / "map.tsv"))
    for key, bad, msg in (("min_ident", 101, "--min-ident 101"), ("min_ident", -1, "--min-ident -1"), ("min_ident", 59.5, "--min-ident 59.5"), ("min_aln", -3, "--min-aln -3"),
                          ("min_bits", float("nan"), "--min-bits nan")):
        with pytest.raises(abundance.AbundanceError, match=msg):
            run(**{key: bad})
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(abundance.AbundanceError, match="distributed run \\(WORLD_SIZE 4\\)"):
        run()
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(abundance.AbundanceError, match="distributed run"):
        run(distributed=True)
    # a request with nothing to refuse reaches the reader - the first thing the fixture forbids
    with pytest.raises(AssertionError, match="GPU work was started"):
        run()
    assert not os.path.exists(tmp_path / "out.tsv")


def test_group_map_reading(tmp_path):
    (tmp_path / "m.tsv").write_text("# gene\tgroup\ng1\tX\n\ng3\tY\textra column\n")
    assert abundance.read_groups(str(tmp_path / "m.tsv"), ["g1", "g2", "g3"]) == {"g1": "X", "g3": "Y"}
    (tmp_path / "two.tsv").write_text("g1\tX\ng1\tY\n")
    with pytest.raises(abundance.AbundanceError, match="gene g1 is given two groups, X and Y"):
        abundance.read_groups(str(tmp_path / "two.tsv"), ["g1"])
    (tmp_path / "one.tsv").write_text("g1\n")
    with pytest.raises(abundance.AbundanceError, match="expected gene<TAB>group"):
        abundance.read_groups(str(tmp_path / "one.tsv"), ["g1"])


def _cli():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_argument_parsing():
    cli = _cli()
    a = cli.parse_arguments(["r1.fq.gz,r2.fq.gz", "genes.faa.gz", "out.tsv"])
    assert a["seqfiles"] == ["r1.fq.gz", "r2.fq.gz"] and a["genes"] == "genes.faa.gz" and a["outfile"] == "out.tsv"
    assert (a["nreads"], a["read_length"], a["min_quality"], a["mean_quality"], a["filter_dups"], a["max_unknown"]) == (2000000, None, -5, -5, False, 100)
    assert (a["min_ident"], a["min_aln"], a["min_bits"], a["groups"], a["ags"], a["ags_report"]) == (0, 0, 0.0, None, None, None)
    assert "device" not in a and "model_dir" not in a and "threads" not in a
    a = cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "-n", "5000", "-l", "100", "-q", "10", "-m", "20", "-d", "-u", "5", "-g", "1", "--min-ident", "60", "--min-aln", "30",
                             "--min-bits", "35.5", "--groups", "map.tsv", "--ags", "3.1e6"])
    assert (a["nreads"], a["read_length"], a["min_quality"], a["mean_quality"], a["filter_dups"], a["max_unknown"], a["device"]) == (5000, 100, 10, 20, True, 5, 1)
    assert (a["min_ident"], a["min_aln"], a["min_bits"], a["groups"], a["ags"]) == (60, 30, 35.5, "map.tsv", 3.1e6)
    assert cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--ags-report", "rep.txt"])["ags_report"] == "rep.txt"
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "--min-ident", "59.5"])           # an integer percent
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa", "o.tsv", "-l", "101"])                     # a length the model was not trained for
    with pytest.raises(SystemExit):
        cli.parse_arguments(["x.fq", "g.faa"])


def test_abundance_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    lib = C.CDLL(g.LIB)
    for s in ("mc_set_abundance", "mc_abundance_reset", "mc_abundance_read", "mc_abundance_ms"):
        assert s in _native.EXPORTED_SYMBOLS and hasattr(lib, s)
    for m in ("set_abundance", "abundance_reset", "abundance", "abundance_ms"):
        assert callable(getattr(_native.Engine, m))
