"""run_abundance under mixed_lengths, end to end on a FASTA of 30,000 reads of 40 - 320 bp (test_gpu_classes.py's recipe and its way of
writing the file) with the classes 100 and 150 and the packaged markers as the genes: (a) with a given AGS the counts, depth and tie
columns are the sums of two fixed-length run_abundance runs, each on one class's reads, and rpkg is the formula on the per-class reads;
(b) with the default AGS the estimate is run_pipeline's under the same classes, bit for bit; (c) one class on reads that all reach it
gives the gene rows of -l byte for byte; (d) the bootstrap under a given AGS."""
import os

import numpy as np
import pytest

from microbecensus_amd import _native, abundance, microbe_census as mc

import abundance_table_cases as TC
import classes_restated as cr
import geneboot_restated as GR

pytestmark = pytest.mark.gpu

CLASSES = TC.CLASSES            # [100, 150]
GENES = os.path.join(_native.DATA_DIR, "markers.faa.gz")


_write_fasta = TC.write_fasta


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the mixed FASTA, one FASTA per class (the reads of that class, uncut), and the reads of at least 100 bp"""
    reads, lens = TC.mixed_reads()      # (the recipe: shared with the `mixed` case of the recorded tables)
    cls = cr.class_of(lens, CLASSES)
    d = tmp_path_factory.mktemp("abund_classes_e2e")
    return {"dir": d, "mixed": _write_fasta(d / "mixed.fa", reads), "cls": cls,
            "class": [_write_fasta(d / ("c%d.fa" % L), [s for s, c in zip(reads, cls) if c == k]) for k, L in enumerate(CLASSES)],
            "reach": _write_fasta(d / "reach.fa", [s for s, c in zip(reads, cls) if c < len(CLASSES)])}


def _run(files, path, out, **kw):
    return abundance.run_abundance(dict({"seqfiles": [path], "genes": GENES, "outfile": str(files["dir"] / out), "nreads": 10 ** 9, "device": 0}, **kw))


def _gene_rows(path):
    return [line for line in open(path).read().split("\n") if not line.startswith("#")]


def test_given_ags_equals_the_sums_of_the_fixed_length_runs(files):
    kw = dict(ags=3.0e6, coverage=True, ties=True)
    table, args = _run(files, files["mixed"], "mixed.tsv", mixed_lengths=list(CLASSES), depth_out=str(files["dir"] / "mixed.depth"), **kw)
    per = [_run(files, files["class"][k], "c%d.tsv" % L, read_length=L, depth_out=str(files["dir"] / ("c%d.depth" % L)), **kw)[0] for k, L in enumerate(CLASSES)]
    n = np.bincount(files["cls"], minlength=3)[:2].tolist()
    assert table["class_reads"] == n == [p["sampled_reads"] for p in per] and table["sampled_reads"] == sum(n) and args["class_reads"] == n
    assert table["length_classes"] == CLASSES and table["trimmed_length"] == "mixed" and args["read_length"] == "mixed"
    assert table["class_reads_assigned"] == [p["reads_assigned"] for p in per] and min(table["class_reads_assigned"]) > 0
    for key in ("reads", "aligned_aa", "depth", "unique_reads", "candidate_reads", "share"):
        want = sum(np.asarray(p[key]).astype(np.uint64 if key == "share" else np.int64) for p in per)
        assert np.array_equal(np.asarray(table[key]).astype(want.dtype), want), key
    assert table["reads_ambiguous"] == sum(p["reads_ambiguous"] for p in per) > 0 and table["reads_assigned"] == sum(table["class_reads_assigned"])
    depth = abundance.read_depth(str(files["dir"] / "mixed.depth"), table["gene"], table["length_aa"])
    assert np.array_equal(depth, table["depth"]) and depth.any()
    # the denominator: the bases of every class
    bases = n[0] * 100 + n[1] * 150
    ge = bases / 3.0e6
    assert table["sampled_bases"] == bases and table["genome_equivalents_sampled"] == ge
    want = table["reads"].astype(np.float64) / (3.0 * table["length_aa"].astype(np.float64) / 1000.0) / ge
    assert GR.same_bits(table["rpkg"], want) and table["rpkg"].any()
    header, rows = abundance.read_table(str(files["dir"] / "mixed.tsv"))
    assert header["trimmed_length"] == "mixed" and header["length_classes"] == "100,150" and header["class_reads"] == "%d,%d" % tuple(n)
    assert header["class_reads_assigned"] == "%d,%d" % tuple(table["class_reads_assigned"]) and header["sampled_bases"] == str(bases)
    assert [r[4] for r in rows] == [repr(float(v)) for v in want]


def test_default_ags_is_run_pipelines_under_the_same_classes(files):
    table, args = _run(files, files["mixed"], "own.tsv", mixed_lengths=list(CLASSES))
    est, pargs = mc.run_pipeline({"seqfiles": [files["mixed"]], "nreads": 10 ** 9, "device": 0, "mixed_lengths": list(CLASSES)})
    assert table["ags_source"] == "run_pipeline" and GR.same_bits([table["ags"]], [est])
    assert table["class_reads"] == pargs["class_reads"] and table["length_classes"] == pargs["length_classes"] == CLASSES
    assert table["genome_equivalents_sampled"] == table["sampled_bases"] / est


def test_one_class_on_reads_that_reach_it_is_the_fixed_length_table(files):
    one, _ = _run(files, files["reach"], "one.tsv", mixed_lengths=[100], ags=3.0e6, coverage=True, ties=True)
    _run(files, files["reach"], "fixed.tsv", read_length=100, ags=3.0e6, coverage=True, ties=True)
    a, b = _gene_rows(str(files["dir"] / "one.tsv")), _gene_rows(str(files["dir"] / "fixed.tsv"))
    assert len(a) > 1000 and a == b and one["reads_assigned"] > 0
    ha, hb = abundance.read_table(str(files["dir"] / "one.tsv"))[0], abundance.read_table(str(files["dir"] / "fixed.tsv"))[0]
    assert set(ha) - set(hb) == {"length_classes", "class_reads", "class_reads_assigned", "sampled_bases"} and (ha["trimmed_length"], hb["trimmed_length"]) == ("mixed", "100")
    assert all(ha[k] == hb[k] for k in hb if k != "trimmed_length")


def test_bootstrap_under_a_given_ags(files):
    kw = dict(mixed_lengths=list(CLASSES), ags=3.0e6, bootstrap=50, nreads=40_000)      # (-n sizes the list: the file holds 30,000 reads)
    table, args = _run(files, files["mixed"], "boot.tsv", **kw)
    again, _ = _run(files, files["mixed"], "boot2.tsv", **kw)
    header, rows = abundance.read_table(str(files["dir"] / "boot.tsv"))
    cols = open(str(files["dir"] / "boot.tsv")).read().split("\n")[len(header)].split("\t")
    assert tuple(cols[-3:]) == abundance.BOOT_COLUMNS and header["bootstrap_denominator"] == "fixed_ags" and header["bootstrap"] == "50"
    assert np.array_equal(table["boot_scale"], np.full(50, 1.0 / table["genome_equivalents_sampled"])) and table["boot_used"] == 50
    for key in ("boot_stats",) + abundance.BOOT_COLUMNS:
        assert GR.same_bits(table[key], again[key]), key
    hit = table["reads"] > 0
    assert hit.any() and (table["rpkg_boot_se"][hit] > 0).all() and (table["rpkg_ci95_low"] <= table["rpkg_ci95_high"]).all()
    assert open(str(files["dir"] / "boot.tsv")).read() == open(str(files["dir"] / "boot2.tsv")).read()
