"""Per-gene read counts on the device (mc_set_abundance; csrc/k_abundance.h states the rule) against tests/abundance_restated.py
applied to the REFERENCE BINARY's m8 goldens: the marker database and the generic one, under cut-offs; independence from batches,
ranges and entry points; the halving path of a range that overflows its pools; the refusals; and run_abundance end to end."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import abund_inputs as I
import abundance_restated as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
CASE = "config1_example_fq"

# the three cut-off sets of the marker test: none; identity >= 60 and aln >= 30; a bit-score cut (the golden's printed bit scores
# step by 0.38 - 0.39: 27.1 lies between 26.95 and 27.34; the test asserts that no printed value lies within 1e-3 of a cut-off)
CUTS = [dict(), dict(min_ident=60, min_aln=30), dict(min_bits=27.1)]


def _same(got, want):
    return np.array_equal(got["reads"], want["reads"]) and np.array_equal(got["aligned"], want["aligned"]) and got["assigned"] == want["assigned"]


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return I.example_reads()


@pytest.fixture(scope="module")
def golden_rows():
    """the reference binary's m8 of the case as restatement rows - computed once, shared, never changed"""
    from microbecensus_amd import _native
    names, _ = _native.load_markers()
    return R.rows_from_m8(os.path.join(GOLD, CASE + ".m8.gz"), names), len(names)


@pytest.mark.parametrize("cut", CUTS, ids=["none", "ident60_aln30", "bits27.1"])
def test_marker_database_equals_the_restatement_of_the_reference_m8(engine, reads, golden_rows, cut):
    rows, nseq = golden_rows
    assert R.cutoffs_clear_of_printed_values(rows, cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    want = R.abundance(rows, nseq, **cut)
    if cut:
        assert 20 < want["assigned"] < R.abundance(rows, nseq)["assigned"]          # (a cut-off set that cuts, and leaves something)
    engine.set_abundance(True, **cut)
    try:
        engine.search(reads)
        got = engine.abundance()
    finally:
        engine.set_abundance(False)
    print(cut, "assigned", got["assigned"], "genes hit", int((got["reads"] > 0).sum()), "searched", got["searched"])
    assert got["searched"] == len(reads)
    assert got["assigned"] == want["assigned"] and int(got["reads"].sum()) == got["assigned"]
    assert np.array_equal(got["reads"], want["reads"]) and np.array_equal(got["aligned"], want["aligned"])


def test_generic_database_equals_the_restatement_of_the_reference_m8():
    """18,553 sequences, 20,000 reads, the generic seed path: subject indices up to 18,552."""
    mixed = dict(min_ident=50, min_aln=25, min_bits=40.5, max_loge=-2.5)
    with I.generic_case() as (eng, names, seqs, rd, meta, m8):
        rows = R.rows_from_m8(m8, names)
        assert len(rows) == meta["m8_rows"] and max(r[1] for r in rows) > 18000
        for cut in (dict(), mixed):
            assert R.cutoffs_clear_of_printed_values(rows, cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
            want = R.abundance(rows, len(names), **cut)
            eng.set_abundance(True, **cut)
            eng.search(rd)
            got = eng.abundance()
            print(cut, "assigned", got["assigned"], "genes hit", int((got["reads"] > 0).sum()), "abundance ms", eng.abundance_ms(), "of", eng.stats()["ms_total"])
            assert got["searched"] == len(rd) and _same(got, want)
        assert want["assigned"] not in (0, meta["reads_with_rows"])          # (the mixed set cuts)


def test_counters_do_not_depend_on_batches_ranges_or_entry_point(engine, reads, golden_rows, tmp_path, monkeypatch):
    from microbecensus_amd import _native
    rows, nseq = golden_rows
    cut = CUTS[2]
    want = R.abundance(rows, nseq, **cut)
    n = len(reads)
    got = {}
    engine.set_abundance(True, **cut)
    try:
        engine.search(reads)
        got["one search"] = engine.abundance()
        engine.abundance_reset()
        zero = engine.abundance()
        assert zero["searched"] == 0 and zero["assigned"] == 0 and not zero["reads"].any() and not zero["aligned"].any() and engine.abundance_ms() == 0.0
        for lo, hi in ((0, 1000), (1000, 1003), (1003, n)):                # three calls of uneven sizes, no reset in between
            engine.search(reads[lo:hi], first_read_id=lo)
        got["three searches"] = engine.abundance()
        engine.set_abundance(False)                                        # off and on again: zeros
        engine.set_abundance(True, **cut)
        zero = engine.abundance()
        assert zero["searched"] == 0 and zero["assigned"] == 0 and not zero["reads"].any() and not zero["aligned"].any()
        monkeypatch.setenv("MC_STREAM_BATCH", "2000")
        engine.search(reads)
        monkeypatch.delenv("MC_STREAM_BATCH")
        got["one search in 2,000-read batches"] = engine.abundance()
        engine.abundance_reset()
        engine.upload(reads)
        engine.run_range(0, 3000, 0)
        engine.run_range(3000, n - 3000, 3000)
        got["upload + run_range pieces"] = engine.abundance()
        engine.abundance_reset()
        engine.range_begin(0, 5001, 0)
        engine.range_end()
        engine.range_begin(5001, n - 5001, 5001)
        engine.range_end()
        got["range_begin / range_end"] = engine.abundance()
        assert len(engine.rows()) > 0                                      # (keep_rows is on: the rows still arrive)
        engine.abundance_reset()
        fa = tmp_path / "reads.fa"
        fa.write_bytes(gzip.open(os.path.join(GOLD, CASE + ".reads.fa.gz"), "rb").read())
        rd = _native.Reader([str(fa)], 100, 10_000_000, False, 0, -5, -5, 100, False)
        try:
            rows_f, best_f = engine.search_files(rd, keep_rows=False)
            assert rd.stats()["sampled"] == n
        finally:
            rd.close()
        assert len(rows_f) == 0 and len(engine.rows()) == 0 and engine.stats()["rows"] == len(rows)      # no row reached the host; all were made
        got["search_files, keep_rows=False"] = engine.abundance()
        assert engine.abundance_ms() > 0.0
    finally:
        engine.set_abundance(False)
    for how, g in got.items():
        assert g["searched"] == n and _same(g, want), how
    # the switch off: the rows and best hits of today, by the golden's md5
    g = json.load(open(os.path.join(GOLD, CASE + ".json")))
    rows_off, best_off = engine.search(reads)
    out = str(tmp_path / "off.m8")
    engine.write_m8(out)
    assert len(rows_off) == g["m8_rows"] and hashlib.md5(open(out, "rb").read()).hexdigest() == g["m8_md5"]
    from microbecensus_amd.microbe_census import _BestHits
    assert dict(_BestHits(best_off, _native.load_model()["families"])._build()) == g["best_hits"]
    with pytest.raises(RuntimeError, match="abundance counting is off"):
        engine.abundance()


def test_search_without_rows_returns_nothing_and_counts_what_search_files_counts(engine, reads, tmp_path):
    """Engine.search(reads, keep_rows=False): nothing comes back and no row reaches the host, the counters are those of
    search_files(keep_rows=False) on the same reads, and the next plain search returns its rows again"""
    from microbecensus_amd import _native
    engine.set_abundance(True, **CUTS[2])
    try:
        assert engine.search(reads, keep_rows=False) is None and len(engine.rows()) == 0 and engine.stats()["rows"] > 0
        got = engine.abundance()
        engine.abundance_reset()
        fa = tmp_path / "reads.fa"
        fa.write_bytes(gzip.open(os.path.join(GOLD, CASE + ".reads.fa.gz"), "rb").read())
        rd = _native.Reader([str(fa)], 100, 10_000_000, False, 0, -5, -5, 100, False)
        try:
            engine.search_files(rd, keep_rows=False)
        finally:
            rd.close()
        want = engine.abundance()
        assert got["searched"] == want["searched"] == len(reads) and want["assigned"] > 0 and _same(got, want)
        rows, best = engine.search(reads)
        assert len(rows) == engine.stats()["rows"] > 0 and len(best) > 0 and len(engine.rows()) == len(rows)
    finally:
        engine.set_abundance(False)


def test_a_range_that_overflows_its_pools_counts_once(monkeypatch):
    """The marker-dense library (abund_inputs.dense_runs says why 24,000 reads), and the test asserts that it takes the halving path.  The
    counters must be those of 5,000-read batches (which fit: no split), and the restatement's on that run's own host rows - the one place
    the code's rows are the yardstick; tests/test_gpu_blindspots.py pins them to the oracle."""
    cut = I.DENSE_CUT
    runs = I.dense_runs(monkeypatch, lambda eng: eng.set_abundance(True, **cut), lambda eng: (eng.abundance(), eng.abundance_ms()), stay=True)
    names, rd, (st, (one, ms)), (st5, (five, _), rows5), ((stay, _), stay_rows) = runs["names"], runs["reads"], runs["one"], runs["five"], runs["stay"]
    print("one call:", st["range_splits"], "splits,", st["rows"], "rows; abundance ms", ms, "of", st["ms_total"])
    assert st["range_splits"] > 0, "the batch did not overflow: the test no longer exercises the halving path"
    assert st5["range_splits"] == 0 and st5["rows"] == st["rows"] == len(rows5)
    assert stay_rows == 0
    want = R.abundance(R.rows_from_array(rows5), len(names), **cut)
    assert want["assigned"] > 10_000 and one["searched"] == five["searched"] == stay["searched"] == len(rd)
    assert _same(five, want) and _same(one, want) and _same(stay, want)


def test_refusals_through_the_abi(engine, reads):
    from microbecensus_amd import _native
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    for args, msg in (((1, 101, 0, 0.0, 1.0), "min_ident 101"), ((1, -1, 0, 0.0, 1.0), "min_ident -1"), ((1, 0, -7, 0.0, 1.0), "min_aln -7"),
                      ((1, 0, 0, float("nan"), 1.0), "min_bits is NaN"), ((1, 0, 0, 0.0, float("nan")), "max_loge is NaN")):
        assert lib.mc_set_abundance(h, *args) != 0 and msg in err(), (args, err())
    assert lib.mc_abundance_reset(h) != 0 and "abundance counting is off" in err()
    buf = np.zeros(len(engine.names), np.int64)
    assert lib.mc_abundance_read(h, buf.ctypes.data, buf.ctypes.data, None, None) != 0 and "abundance counting is off" in err()
    # best hits only, in both orders
    engine.set_best_hits_only(True)
    assert lib.mc_set_abundance(h, 1, 0, 0, 0.0, 1.0) != 0 and "best hits only is on" in err()
    engine.set_best_hits_only(False)
    engine.set_abundance(True)
    try:
        assert lib.mc_set_best_hits_only(h, 1) != 0 and "abundance counting is on" in err()
        assert lib.mc_set_best_hits_only(h, 0) == 0
        # a range in flight
        engine.upload(reads[:2000])
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_abundance(h, 1, 0, 0, 0.0, 1.0) != 0 and "in flight" in err()
        assert lib.mc_set_abundance(h, 0, 0, 0, 0.0, 1.0) != 0 and "in flight" in err()
        assert lib.mc_abundance_reset(h) != 0 and "in flight" in err()
        engine.range_end()
        assert engine.abundance()["searched"] == 2000
        # length classes while the counts are on
        rows = np.zeros((4, 100), np.uint8)
        assert lib.mc_search_classes(h, rows.ctypes.data, 4, 100, 0) != 0
        # a refused cut-off leaves the counts as they were, and the handle usable
        assert lib.mc_set_abundance(h, 1, 200, 0, 0.0, 1.0) != 0 and "min_ident 200" in err()
        engine.search(reads[:2000])
        assert engine.abundance()["searched"] == 4000
    finally:
        engine.set_abundance(False)
    model = _native.load_model()
    engine.set_run_classes([100], {100: model["pars"]["100"]}, model["families"])
    try:
        engine.set_abundance(True)
        pad = np.zeros((50, 100), np.uint8)
        pad[:] = reads[:50]
        assert lib.mc_search_classes(h, pad.ctypes.data, 50, 100, 0) != 0 and "abundance counting is on" in err()
        engine.set_abundance(False)
        best, cls, per = engine.search_classes(pad)                        # ... and off again it runs
        assert int(per.sum()) == 50
    finally:
        engine.set_abundance(False)
        engine.set_run(100, model["pars"]["100"], model["families"])
    rows_ok, _ = engine.search(reads[:2000])                               # the handle is what it was
    assert len(rows_ok) > 0


def test_run_abundance_end_to_end(golden_rows, tmp_path):
    """run_abundance with the packaged markers as the genes, on the example FASTQ under config1's sample options (-n 10000; 100 bp).  The
    table under --ags-report is compared byte for byte except for the one header line that names where the AGS came from - the line
    the two runs must differ in."""
    from microbecensus_amd import _native, abundance, microbe_census
    rows, nseq = golden_rows
    want = R.abundance(rows, nseq)
    g = json.load(open(os.path.join(GOLD, CASE + ".json")))
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    out = str(tmp_path / "genes.tsv")
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % (n, n.split("_")[0]) for n in _native.load_markers()[0][:4000]))
    table, args = abundance.run_abundance({"seqfiles": [fq], "genes": genes, "outfile": out, "nreads": 10000, "device": 0, "groups": str(tmp_path / "map.tsv")})
    est, pargs = microbe_census.run_pipeline({"seqfiles": [fq], "nreads": 10000, "device": 0})
    assert est == g["est_ags"] and table["ags"] == est and args["sampled_reads"] == pargs["sampled_reads"] == g["sampled_reads"] and args["read_length"] == 100
    header, body = abundance.read_table(out)
    assert header["average_genome_size"] == repr(est) and float(header["average_genome_size"]) == est and header["ags_source"] == "run_pipeline"
    assert (int(header["sampled_reads"]), int(header["trimmed_length"]), int(header["reads_assigned"])) == (g["sampled_reads"], 100, want["assigned"])
    assert (header["min_ident"], header["min_aln"], header["min_bits"], header["metagenome"], header["genes"]) == ("0", "0", "0.0", fq, genes)
    names, seqs = _native.load_markers()
    assert [r[0] for r in body] == names and [int(r[1]) for r in body] == [len(s) for s in seqs]        # every gene, FASTA order, zeros included
    assert [int(r[2]) for r in body] == want["reads"].tolist() and [int(r[3]) for r in body] == want["aligned"].tolist()
    ge = int(header["sampled_reads"]) * int(header["trimmed_length"]) / float(header["average_genome_size"])
    assert float(header["genome_equivalents_sampled"]) == ge
    assert [float(r[4]) for r in body] == [int(r[2]) / (3 * int(r[1]) / 1000.0) / ge for r in body]
    gh, gbody = abundance.read_table(out + ".groups.tsv")
    assert gh["reads_assigned"] == header["reads_assigned"] and sum(int(r[1]) for r in gbody) == nseq and sum(int(r[2]) for r in gbody) == want["assigned"]
    assert [tuple(r) for r in gbody] == [(a, str(b), str(c), repr(d)) for a, b, c, d in abundance.group_table(names, want["reads"], [float(r[4]) for r in body],
                                                                                                      {n: n.split("_")[0] for n in names[:4000]})]
    # --ags-report: that run's report
    rep = str(tmp_path / "report.txt")
    microbe_census.report_results(dict(pargs, outfile=rep), est, None)
    out2 = str(tmp_path / "genes2.tsv")
    abundance.run_abundance({"seqfiles": [fq], "genes": genes, "outfile": out2, "nreads": 10000, "device": 0, "ags_report": rep})
    a, b = open(out, "rb").read().split(b"\n"), open(out2, "rb").read().split(b"\n")
    assert [l for l in b if l.startswith(b"# ags_source:")] == [("# ags_source:\treport %s" % rep).encode()]
    assert [l for l in a if not l.startswith(b"# ags_source:")] == [l for l in b if not l.startswith(b"# ags_source:")]
