"""The rarefaction curve end to end (csrc/k_curve.h states the rule, tests/curve_restated.py restates it): on the marker engine and the
example reads the curve does not depend on how the reads reach the device - one call, MC_STREAM_BATCH-sized batches, range_begin /
range_end, the dense library's halving path - and equals the restatement on the rows; run_abundance's table['curve'] equals, point by
point, a fresh run_abundance with -n n_k; and the refusals of the ABI."""
import ctypes as C
import os

import numpy as np
import pytest

import abund_inputs as I
import coverage_restated as V
import curve_restated as CR

pytestmark = pytest.mark.gpu

GOLD = I.GOLD


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return I.example_reads()


def _same(cu, want, how):
    for k in ("reads", "aligned", "covered"):
        assert np.array_equal(cu[k], want[k]), (how, k)
    assert np.array_equal(cu["assigned"], want["assigned"]) and cu["beyond"] == want["beyond"], how


def test_curve_does_not_depend_on_batches_or_ranges(engine, reads, monkeypatch):
    from microbecensus_amd import _native, microbe_census
    n = len(reads)
    lengths = [len(s) for s in _native.load_markers()[1]]
    points = microbe_census.curve_points(n, 5)
    got = {}
    engine.set_abundance(True)
    try:
        engine.set_coverage(True)
        engine.set_curve(points)
        rows, _ = engine.search(reads)
        rows = rows.copy()
        got["one call"] = engine.curve()
        ab, cov = engine.abundance(), engine.coverage()
        assert engine.curve_ms() > 0.0
        engine.abundance_reset()
        zero = engine.curve()
        assert not zero["reads"].any() and not zero["covered"].any() and not zero["assigned"].any() and zero["beyond"] == 0
        monkeypatch.setenv("MC_STREAM_BATCH", "2000")
        engine.search(reads)
        monkeypatch.delenv("MC_STREAM_BATCH")
        got["2,000-read batches"] = engine.curve()
        engine.abundance_reset()
        engine.upload(reads)
        for lo, hi in ((5001, n), (0, 5001)):                             # the later range first: minima and sums commute
            engine.range_begin(lo, hi - lo, lo)
            engine.range_end()
        got["range_begin / range_end"] = engine.curve()
        want = CR.curve(V.rows_from_array(rows), lengths, points)
        assert want["beyond"] == 0 and 0 < (want["reads"][0] > 0).sum() < (want["reads"][-1] > 0).sum() and 0 < want["covered"][0].sum() < want["covered"][-1].sum()
        for how, cu in got.items():
            _same(cu, want, how)
        assert np.array_equal(got["one call"]["reads"][-1], ab["reads"]) and np.array_equal(got["one call"]["aligned"][-1], ab["aligned"])      # the last point is the run's own table
        assert np.array_equal(got["one call"]["covered"][-1], cov["covered"]) and int(got["one call"]["assigned"][-1]) == ab["assigned"]
        # a last point short of the sample: the reads behind it are reported and in no point; coverage off: no covered, the same counts
        engine.set_coverage(False)
        engine.set_curve(points[:2])
        engine.search(reads)
        short = engine.curve(covered=False)
        assert short["beyond"] == int(want["assigned"][-1] - want["assigned"][1]) > 0 and np.array_equal(short["reads"], want["reads"][:2]) and "covered" not in short
        engine.set_curve(None)
        engine.abundance_reset()
        engine.search(reads)
        assert np.array_equal(engine.abundance()["reads"], ab["reads"])   # the curve off again: the counts as before
    finally:
        engine.set_abundance(False)


def test_curve_of_a_range_rerun_in_halves_counts_once(monkeypatch):
    """The marker-dense library overflows its pools and is rerun in halves (abund_inputs.dense_runs): every piece comes through the launch
    function once."""
    from microbecensus_amd import microbe_census
    points = microbe_census.curve_points(24_000, 4)

    def switches(eng):
        eng.set_abundance(True, **I.DENSE_CUT)
        eng.set_coverage(True)
        eng.set_curve(points)
    runs = I.dense_runs(monkeypatch, switches, lambda eng: (eng.curve(), eng.abundance(), eng.coverage()))
    lengths = [len(s) for s in runs["seqs"]]
    (st, one), (st5, five, rows5) = runs["one"], runs["five"]
    print("one call:", st["range_splits"], "splits,", st["rows"], "rows")
    assert st["range_splits"] > 0, "the batch did not overflow: the test no longer exercises the halving path"
    assert st5["range_splits"] == 0 and st5["rows"] == st["rows"] == len(rows5)
    want = CR.curve(V.rows_from_array(rows5), lengths, points, **I.DENSE_CUT)
    assert want["beyond"] == 0 and int(want["assigned"][0]) > 2000
    for how, (cu, ab, cov) in (("5,000-read batches", five), ("one call", one)):
        _same(cu, want, how)
        assert np.array_equal(cu["reads"][-1], ab["reads"]) and np.array_equal(cu["covered"][-1], cov["covered"]) and int(cu["assigned"][-1]) == ab["assigned"], how


def test_run_abundance_curve_equals_fresh_runs(tmp_path):
    """run_abundance on the example FASTQ with -n 10000, --ags 3.0e6, --min-breadth, --groups and K = 3: every point equals a fresh
    run_abundance with nreads = n_k; the last point equals the run's own table."""
    from microbecensus_amd import _native, abundance, microbe_census
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % (n, n.split("_")[0]) for n in _native.load_markers()[0][:4000]))

    def run(out, **kw):
        return abundance.run_abundance(dict({"seqfiles": [fq], "genes": genes, "outfile": str(tmp_path / out), "nreads": 10000, "device": 0, "ags": 3.0e6, "min_breadth": 0.1,
                                             "groups": str(tmp_path / "map.tsv")}, **kw))
    table, args = run("curve.tsv", curve=3, curve_genes=str(tmp_path / "matrix.tsv"))
    cu = table["curve"]
    assert cu["points"] == microbe_census.curve_points(table["sampled_reads"], 3) and cu["points"][-1] == table["sampled_reads"] == 8672 and args["curve_ms"] > 0.0
    plain, _ = run("plain.tsv")
    for k, n_k in enumerate(cu["points"]):
        fresh = plain if k == 2 else run("fresh%d.tsv" % k, nreads=n_k)[0]
        assert fresh["sampled_reads"] == n_k
        for key, mine in (("reads", "reads"), ("aligned_aa", "aligned_aa"), ("covered_aa", "covered_aa"), ("detected", "detected"), ("rpkg", "rpkg")):
            assert np.array_equal(cu[mine][k], fresh[key]), (k, key)
        assert cu["groups"][k] == fresh["groups"] and cu["reads_assigned"][k] == fresh["reads_assigned"] and cu["genome_equivalents_sampled"][k] == fresh["genome_equivalents_sampled"]
        assert cu["genes_detected"][k] == int(fresh["detected"].sum()) and cu["genes_with_reads"][k] == int((fresh["reads"] > 0).sum())
        assert cu["groups_with_reads"][k] == sum(1 for g in fresh["groups"] if g[2] > 0)
    assert cu["genes_with_reads"][0] < cu["genes_with_reads"][-1] and cu["reads_assigned"][0] < cu["reads_assigned"][-1]
    for key in ("reads", "aligned_aa", "covered_aa", "detected", "rpkg"):                       # the last point is the run's own table, which is the plain run's
        assert np.array_equal(cu[key][-1], table[key]) and np.array_equal(table[key], plain[key]), key
    # the files: the gene table differs from the plain run's by the one header line; the curve table and the matrix hold the points
    a, b = open(str(tmp_path / "curve.tsv")).read().split("\n"), open(str(tmp_path / "plain.tsv")).read().split("\n")
    assert [l for l in a if l != "# curve:\t3"] == b and a.count("# curve:\t3") == 1
    header, body = abundance.read_table(str(tmp_path / "curve.tsv.curve.tsv"))
    assert header["curve"] == "3" and [int(r[0]) for r in body] == cu["points"] and [int(r[3]) for r in body] == cu["reads_assigned"] and [int(r[5]) for r in body] == cu["genes_detected"]
    lines = open(str(tmp_path / "matrix.tsv")).read().split("\n")
    assert lines[1].split("\t") == ["gene"] + ["reads_%d" % k for k in (1, 2, 3)] + ["covered_aa_%d" % k for k in (1, 2, 3)] and len(lines) == 3 + len(table["gene"])
    assert [int(l.split("\t")[3]) for l in lines[2:-1]] == table["reads"].tolist()


def test_run_abundance_curve_with_the_samples_own_ags(tmp_path):
    """The default AGS source: run_pipeline's own curve at the same points gives every point its AGS, and the last point's AGS, genome
    equivalents and RPKG are the run's own table's."""
    from microbecensus_amd import _native, abundance, microbe_census
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    table, args = abundance.run_abundance({"seqfiles": [fq], "genes": genes, "outfile": str(tmp_path / "own.tsv"), "nreads": 10000, "device": 0, "curve": 3})
    est, pargs = microbe_census.run_pipeline({"seqfiles": [fq], "nreads": 10000, "device": 0, "curve": 3})
    cu = table["curve"]
    assert table["ags_source"] == "run_pipeline" and table["ags"] == est and "covered_aa" not in cu
    assert cu["points"] == [p["reads"] for p in pargs["ags_curve"]] == microbe_census.curve_points(table["sampled_reads"], 3)
    assert cu["ags"] == [p["ags"] for p in pargs["ags_curve"]] and all(a is not None and a > 0 for a in cu["ags"]) and len(set(cu["ags"])) == 3
    assert cu["ags"][-1] == table["ags"] and cu["genome_equivalents_sampled"][-1] == table["genome_equivalents_sampled"]
    assert np.array_equal(cu["rpkg"][-1], table["rpkg"]) and np.array_equal(cu["reads"][-1], table["reads"]) and cu["reads_assigned"][-1] == table["reads_assigned"]
    for k, n_k in enumerate(cu["points"]):
        ge = abundance.genome_equivalents(n_k, table["trimmed_length"], cu["ags"][k])
        assert cu["genome_equivalents_sampled"][k] == ge and np.array_equal(cu["rpkg"][k], abundance.rpkg(cu["reads"][k], table["length_aa"], ge))
    header, body = abundance.read_table(str(tmp_path / "own.tsv.curve.tsv"))
    assert header["ags_source"] == "run_pipeline" and [r[1] for r in body] == [repr(a) for a in cu["ags"]] and [r[2] for r in body] == [repr(g) for g in cu["genome_equivalents_sampled"]]


def test_refusals_through_the_abi(engine, reads):
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    nseq = len(engine.names)
    pts = np.array([10, 20, 30], np.int64)
    buf = np.zeros(3 * nseq, np.int64)
    three, beyond = np.zeros(3, np.int64), C.c_int64(-1)
    assert lib.mc_set_curve(h, 3, pts.ctypes.data) != 0 and "abundance counting is off" in err() and "K = 3" in err()
    assert lib.mc_curve_read(h, buf.ctypes.data, None, None, None, None) != 0 and "the curve is off" in err()
    assert lib.mc_curve_ms(h) == 0.0 and lib.mc_set_curve(h, 0, None) == 0            # off while off: nothing to do
    engine.set_abundance(True)
    try:
        assert lib.mc_set_curve(h, -1, pts.ctypes.data) != 0 and "K -1 is not a number of points from 0 to 64" in err()
        assert lib.mc_set_curve(h, 65, pts.ctypes.data) != 0 and "K 65 is not a number of points from 0 to 64" in err()
        bad = np.array([0, 5, 6], np.int64)
        assert lib.mc_set_curve(h, 3, bad.ctypes.data) != 0 and "point 0 is 0: below 1" in err()
        bad = np.array([5, 4, 6], np.int64)
        assert lib.mc_set_curve(h, 3, bad.ctypes.data) != 0 and "point 1 is 4: below the point before it, 5" in err()
        assert lib.mc_curve_read(h, buf.ctypes.data, None, None, None, None) != 0 and "the curve is off" in err()      # every refusal left it off
        rep = np.array([5, 5, 6], np.int64)
        assert lib.mc_curve_k(h) == 0 and lib.mc_set_curve(h, 3, rep.ctypes.data) == 0 and lib.mc_curve_k(h) == 3      # repeats are allowed
        assert engine.curve(covered=False)["reads"].shape == (3, nseq)             # (set through the raw ABI: the binding asks the library for K)
        assert lib.mc_curve_read(h, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, three.ctypes.data, C.byref(beyond)) != 0 and "covered asked for with coverage off" in err()
        assert lib.mc_curve_read(h, buf.ctypes.data, None, None, three.ctypes.data, C.byref(beyond)) == 0 and not buf.any() and beyond.value == 0
        with pytest.raises(RuntimeError, match="mc_search_varlen: refused while the curve is on .*K = 3"):
            engine.search_varlen([bytes(reads[0]), bytes(reads[1][:90])])
        engine.upload(reads[:500])
        engine.range_begin(0, 500, 0)
        try:
            assert lib.mc_set_curve(h, 3, pts.ctypes.data) != 0 and "still in flight" in err()
            assert lib.mc_set_curve(h, 0, None) != 0 and "still in flight" in err()
        finally:
            engine.range_end()
        assert lib.mc_set_curve(h, 0, None) == 0 and lib.mc_curve_k(h) == 0
        rows_ok, _ = engine.search_varlen([bytes(reads[0]), bytes(reads[1][:90])])  # the curve off: mixed lengths are searched again
    finally:
        engine.set_abundance(False)
    assert lib.mc_curve_read(h, buf.ctypes.data, None, None, None, None) != 0 and "the curve is off" in err()          # the counts going off took the curve with them
