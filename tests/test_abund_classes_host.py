"""Gene abundances under mixed_lengths, the part that needs no GPU: every refusal of the front end with its message - before any engine
or reader is opened -, how the length classes are resolved (a list, the report's length_classes line, the reads themselves, a list that
contradicts the report), the denominator's arithmetic, the header lines, a write_table / read_table round trip and the command line."""
import importlib.util
import os

import numpy as np
import pytest

from microbecensus_amd import _native, abundance, microbe_census

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FQ = os.path.join(HERE, "golden", "inputs", "example.fq.gz")
VALID = [int(x) for x in microbe_census._valid_read_lengths()]


class _Started(AssertionError):
    pass


@pytest.fixture
def no_engine(monkeypatch):
    """an engine, a reader (of one length or of classes) or run_pipeline: the first one that is asked for says which classes it got"""
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
    monkeypatch.setattr(microbe_census, "run_pipeline", lambda a: (_ for _ in ()).throw(_Started("run_pipeline %s" % (a.get("mixed_lengths"),))))
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def _faa(path):
    path.write_text(">g1 x\n%s\n>g2 y\n%s\n" % ("MKV" * 20, "MLA" * 30))
    return str(path)


def _report(path, ags=3051745.5, classes=None):
    path.write_text("Parameters\nmetagenome:\tx\n" + ("length_classes:\t%s\n" % "\t".join(map(str, classes)) if classes else "") + "\nResults\naverage_genome_size:\t%r\n" % ags)
    return str(path)


def test_refusals_before_any_gpu_work(tmp_path, no_engine):
    good = _faa(tmp_path / "good.faa")

    def run(**kw):
        args = {"seqfiles": [FQ], "genes": good, "outfile": str(tmp_path / "out.tsv"), "nreads": 100, "ags": 3.0e6, "mixed_lengths": [100, 150]}
        args.update(kw)
        return abundance.run_abundance(args)
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths 100,150 cannot be combined with -l 100: every read is cut to its own length class"):
        run(read_length=100)
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths cannot be combined with -l 150"):
        run(read_length=150, mixed_lengths=True)
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths 100,150 cannot be combined with --curve 8: rarefying reads of mixed lengths needs the bases of every prefix"):
        run(curve=8)
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths 100,150 with --bootstrap 50 needs --ags or --ags-report: the default AGS is run_pipeline's, which does not bootstrap"):
        run(ags=None, bootstrap=50)
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths 100,101: length classes \[101\] are not lengths the model was trained for: \[50, "):
        run(mixed_lengths=[100, 101])
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths : length classes \[\] are not lengths the model was trained for"):
        run(mixed_lengths=[])
    rep = _report(tmp_path / "bad.txt", classes=[100, 149])
    with pytest.raises(abundance.AbundanceError, match=r"AGS report .*bad.txt: length classes \[149\] are not lengths the model"):
        run(ags=None, ags_report=rep, mixed_lengths=True)
    rep = _report(tmp_path / "r.txt", classes=[100, 150, 200])
    with pytest.raises(abundance.AbundanceError, match=r"--mixed-lengths 100,150 contradicts the length_classes 100,150,200 of the AGS report .*r.txt"):
        run(ags=None, ags_report=rep)
    assert not os.path.exists(tmp_path / "out.tsv")
    # the switch off: none of this is looked at, and -l and --curve are what they were
    with pytest.raises(_Started, match="GPU work was started"):
        run(mixed_lengths=None, read_length=100, curve=8)
    with pytest.raises(_Started, match="GPU work was started"):
        run(mixed_lengths=False, read_length=100)


def test_how_the_classes_are_resolved(tmp_path, no_engine):
    good = _faa(tmp_path / "good.faa")

    def run(**kw):
        args = {"seqfiles": [FQ], "genes": good, "outfile": str(tmp_path / "out.tsv"), "nreads": 100, "ags": 3.0e6}
        args.update(kw)
        return abundance.run_abundance(args)
    with pytest.raises(_Started, match=r"class reader \[100, 150\]"):             # a list: sorted, repeats dropped
        run(mixed_lengths=[150, 100, 150])
    rep = _report(tmp_path / "r.txt", classes=[70, 100])
    with pytest.raises(_Started, match=r"class reader \[70, 100\]"):              # the report's line
        run(ags=None, ags_report=rep, mixed_lengths=True)
    with pytest.raises(_Started, match=r"class reader \[70, 100\]"):              # a list that agrees with it
        run(ags=None, ags_report=rep, mixed_lengths=[100, 70])
    plain = _report(tmp_path / "plain.txt")
    want = microbe_census.auto_detect_length_classes(FQ, VALID)
    with pytest.raises(_Started, match=r"class reader %s" % str(want).replace("[", r"\[").replace("]", r"\]")):     # neither: the reads themselves
        run(ags=None, ags_report=plain, mixed_lengths=True)
    with pytest.raises(_Started, match=r"class reader %s" % str(want).replace("[", r"\[").replace("]", r"\]")):
        run(mixed_lengths=True)
    # the default AGS: run_pipeline is handed the same classes
    with pytest.raises(_Started, match=r"run_pipeline \[100, 150\]"):
        run(ags=None, mixed_lengths=[100, 150])
    with pytest.raises(_Started, match=r"run_pipeline %s" % str(want).replace("[", r"\[").replace("]", r"\]")):
        run(ags=None, mixed_lengths=True)
    assert abundance.read_report_classes(rep) == [70, 100] and abundance.read_report_classes(plain) is None
    (tmp_path / "nan.txt").write_text("length_classes:\t100\tx\naverage_genome_size:\t3.0\n")
    with pytest.raises(abundance.AbundanceError, match="length_classes .* are not integers"):
        abundance.read_report_classes(str(tmp_path / "nan.txt"))
    # run_pipeline's own report is read back
    out = str(tmp_path / "rep.txt")
    microbe_census.report_results({"outfile": out, "seqfiles": ["x.fq"], "sampled_reads": 10, "read_length": "mixed", "mixed_lengths": [100, 150], "length_classes": [100, 150],
                                   "class_reads": [4, 6], "min_quality": -5, "mean_quality": -5, "filter_dups": False, "max_unknown": 100}, 2.5e6, None)
    assert abundance.read_report_classes(out) == [100, 150] and abundance.read_ags_report(out) == 2.5e6


def test_the_denominator_by_hand():
    assert abundance.sampled_bases([4, 6], [100, 150]) == 1300 and abundance.sampled_bases([0, 0], [100, 150]) == 0
    assert abundance.sampled_bases(np.array([2 ** 40, 1]), [100, 150]) == 2 ** 40 * 100 + 150          # integers, not float64
    ge = 1300 / 2.6e6
    assert abundance.rpkg(5, 120, ge) == 5 / (3 * 120 / 1000.0) / ge
    # one class: the fixed-length formula
    assert abundance.sampled_bases([8672], [100]) / 3.0e6 == abundance.genome_equivalents(8672, 100, 3.0e6)


def _table():
    length = np.array([120, 300], np.int64)
    ge = (4 * 100 + 6 * 150) / 2.6e6
    reads = np.array([5, 0], np.int64)
    return {"gene": ["g1", "g2"], "length_aa": length, "reads": reads, "aligned_aa": np.array([150, 0], np.int64), "rpkg": abundance.rpkg(reads, length, ge), "sampled_reads": 10,
            "trimmed_length": "mixed", "ags": 2.6e6, "ags_source": "--ags", "genome_equivalents_sampled": ge, "reads_assigned": 5, "length_classes": [100, 150], "class_reads": [4, 6],
            "class_reads_assigned": [2, 3], "sampled_bases": 1300}


def test_header_lines_and_round_trip(tmp_path):
    args = {"seqfiles": ["a.fq.gz"], "genes": "genes.faa", "min_ident": 0, "min_aln": 0, "min_bits": 0.0}
    t = _table()
    out = str(tmp_path / "out.tsv")
    abundance.write_table(out, args, t)
    lines = open(out).read().split("\n")
    assert lines[:8] == ["# metagenome:\ta.fq.gz", "# genes:\tgenes.faa", "# sampled_reads:\t10", "# trimmed_length:\tmixed", "# length_classes:\t100,150", "# class_reads:\t4,6",
                         "# class_reads_assigned:\t2,3", "# sampled_bases:\t1300"]
    assert lines[8] == "# min_ident:\t0" and lines[15] == "gene\tlength_aa\treads\taligned_aa\trpkg"
    header, rows = abundance.read_table(out)
    assert [int(x) for x in header["length_classes"].split(",")] == t["length_classes"] and [int(x) for x in header["class_reads"].split(",")] == t["class_reads"]
    assert int(header["sampled_bases"]) == 1300 and float(header["genome_equivalents_sampled"]) == t["genome_equivalents_sampled"] == 1300 / float(header["average_genome_size"])
    assert [float(r[4]) for r in rows] == t["rpkg"].tolist() and [r[0] for r in rows] == t["gene"]
    # without the switch's keys the header is what it was
    for k in ("length_classes", "class_reads", "class_reads_assigned", "sampled_bases"):
        del t[k]
    t["trimmed_length"] = 100
    abundance.write_table(out, args, t)
    assert [l.split(":")[0] for l in open(out).read().split("\n")[:5]] == ["# metagenome", "# genes", "# sampled_reads", "# trimmed_length", "# min_ident"]


def test_cli_spells_the_switch_as_run_microbe_census_does():
    spec = importlib.util.spec_from_file_location("gene_abundance_cli", os.path.join(REPO, "scripts", "gene_abundance.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["x.fq", "g.faa", "o.tsv"]
    assert cli.parse_arguments(base)["mixed_lengths"] is None
    assert cli.parse_arguments(base + ["--mixed-lengths"])["mixed_lengths"] is True
    assert cli.parse_arguments(["--mixed-lengths", "100,150"] + base)["mixed_lengths"] == [100, 150]
    with pytest.raises(SystemExit):
        cli.parse_arguments(base + ["--mixed-lengths", "100,x"])


def test_the_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "mcensus.h")).read()
    for name in ("mc_set_abundance_classes", "mc_abundance_classes_read", "mc_abundance_classes_ms"):
        assert name + "(" in text and name in _native.EXPORTED_SYMBOLS
    assert hasattr(_native.Engine, "set_abundance_classes") and hasattr(_native.Engine, "abundance_classes")
