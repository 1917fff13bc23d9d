"""Coverage breadth and depth on the device (mc_set_coverage; csrc/k_coverage.h states the rule) against tests/coverage_restated.py
applied to the REFERENCE BINARY's m8 goldens: the marker database and the generic one, under cut-offs; independence from batches,
ranges, entry points and reads in between; the halving path of a range that overflows its pools; the refusals; and run_abundance with
the three switches end to end.  The counts of the same run are held to tests/abundance_restated.py throughout."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import abund_inputs as I
import abundance_restated as R
import coverage_restated as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASE = "config1_example_fq"
CUTS = [dict(), dict(min_ident=60, min_aln=30)]


def _same(got, depth, want):
    return all(np.array_equal(got[k], want[k]) for k in ("covered", "spanned", "max_depth")) and np.array_equal(depth, want["depth"])


def _same_counts(got, want):
    return np.array_equal(got["reads"], want["reads"]) and np.array_equal(got["aligned"], want["aligned"]) and got["assigned"] == want["assigned"]


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return I.example_reads()


@pytest.fixture(scope="module")
def golden():
    """the reference binary's m8 of the case restated under both cut-off sets - computed once, shared, never changed"""
    from microbecensus_amd import _native
    names, seqs = _native.load_markers()
    lengths = [len(s) for s in seqs]
    rows = V.rows_from_m8(os.path.join(GOLD, CASE + ".m8.gz"), names)
    return {"rows": rows, "lengths": lengths, "cov": [V.coverage(rows, lengths, **c) for c in CUTS], "ab": [R.abundance([r[:6] for r in rows], len(names), **c) for c in CUTS]}


@pytest.mark.parametrize("k", [0, 1], ids=["none", "ident60_aln30"])
def test_marker_database_equals_the_restatement_of_the_reference_m8(engine, reads, golden, k):
    want, want_ab = golden["cov"][k], golden["ab"][k]
    if k:
        assert 20 < want_ab["assigned"] < golden["ab"][0]["assigned"]                   # (a cut-off set that cuts, and leaves something)
    engine.set_abundance(True, **CUTS[k])
    try:
        engine.set_coverage(True)
        engine.search(reads)
        got, depth, ab = engine.coverage(), engine.coverage_depth(), engine.abundance()
        ms = engine.coverage_ms()
    finally:
        engine.set_abundance(False)
    print(CUTS[k], "assigned", ab["assigned"], "covered", int(got["covered"].sum()), "spanned", int(got["spanned"].sum()), "max depth", int(got["max_depth"].max()), "scan ms", ms)
    assert depth.dtype == np.uint32 and len(depth) == sum(golden["lengths"]) and ms > 0.0
    assert ab["searched"] == len(reads) and _same_counts(ab, want_ab)
    assert _same(got, depth, want)
    assert V.invariants(got, ab["reads"], golden["lengths"]) == []
    if not k:
        assert (int(got["covered"].sum()), int(got["spanned"].sum()), int(got["max_depth"].max())) == (5167, 5288, 2)


def test_generic_database_equals_the_restatement_of_the_reference_m8():
    """18,553 sequences, 20,000 reads, the generic seed path: depths up to 10, subject indices up to 18,552."""
    mixed = dict(min_ident=50, min_aln=25, min_bits=40.5, max_loge=-2.5)
    with I.generic_case() as (eng, names, seqs, rd, meta, m8):
        lengths = [len(s) for s in seqs]
        rows = V.rows_from_m8(m8, names)
        assert len(rows) == meta["m8_rows"]
        for cut in (dict(), mixed):
            assert R.cutoffs_clear_of_printed_values(rows, cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
            want, want_ab = V.coverage(rows, lengths, **cut), R.abundance([r[:6] for r in rows], len(names), **cut)
            eng.set_abundance(True, **cut)
            eng.set_coverage(True)
            eng.search(rd)
            got, depth, ab = eng.coverage(), eng.coverage_depth(), eng.abundance()
            print(cut, "assigned", ab["assigned"], "covered", int(got["covered"].sum()), "spanned", int(got["spanned"].sum()), "max depth", int(got["max_depth"].max()),
                  "abundance ms", eng.abundance_ms(), "scan ms", eng.coverage_ms(), "of", eng.stats()["ms_total"])
            assert ab["searched"] == len(rd) and _same_counts(ab, want_ab) and _same(got, depth, want)
            assert V.invariants(got, ab["reads"], lengths) == []
        assert want_ab["assigned"] not in (0, meta["reads_with_rows"])                   # (the mixed set cuts)


def test_coverage_does_not_depend_on_batches_ranges_or_entry_point(engine, reads, golden, tmp_path, monkeypatch):
    from microbecensus_amd import _native
    cut, want, want_ab = CUTS[0], golden["cov"][0], golden["ab"][0]
    n = len(reads)
    got = {}

    def take(how):
        got[how] = (engine.coverage(), engine.coverage_depth(), engine.abundance())

    def zeros():
        c, d, a = engine.coverage(), engine.coverage_depth(), engine.abundance()
        return not any(c[k].any() for k in c) and not d.any() and a["searched"] == 0 and a["assigned"] == 0 and not a["reads"].any()
    engine.set_abundance(True, **cut)
    try:
        engine.set_coverage(True)
        engine.search(reads)
        take("one search")
        engine.abundance_reset()                                           # ... zeroes the depth too
        assert zeros() and engine.abundance_ms() == 0.0
        between = None
        for lo, hi in ((0, 1000), (1000, 1003), (1003, n)):                # three calls of uneven sizes, no reset in between
            engine.search(reads[lo:hi], first_read_id=lo)
            if hi == 1003:
                between = engine.coverage()                                # a read between two of them changes nothing
        take("three searches, a read in between")
        assert 0 < int(between["spanned"].sum()) < int(want["spanned"].sum())
        engine.set_coverage(False)                                         # off and on again: zeros, of the counts too
        with pytest.raises(RuntimeError, match="coverage is off"):
            engine.coverage()
        assert engine.abundance()["searched"] == n                         # (off leaves the counts alone)
        engine.set_coverage(True)
        assert zeros()
        monkeypatch.setenv("MC_STREAM_BATCH", "2000")
        engine.search(reads)
        monkeypatch.delenv("MC_STREAM_BATCH")
        take("one search in 2,000-read batches")
        engine.abundance_reset()
        engine.upload(reads)
        engine.run_range(0, 3000, 0)
        engine.run_range(3000, n - 3000, 3000)
        take("upload + run_range pieces")
        engine.abundance_reset()
        fa = tmp_path / "reads.fa"
        fa.write_bytes(gzip.open(os.path.join(GOLD, CASE + ".reads.fa.gz"), "rb").read())
        rd = _native.Reader([str(fa)], 100, 10_000_000, False, 0, -5, -5, 100, False)
        try:
            rows_f, _ = engine.search_files(rd, keep_rows=False)
            assert rd.stats()["sampled"] == n
        finally:
            rd.close()
        assert len(rows_f) == 0 and len(engine.rows()) == 0 and engine.stats()["rows"] == len(golden["rows"])     # no row reached the host; all were made
        take("search_files, keep_rows=False")
        assert engine.coverage_ms() > 0.0
        engine.set_abundance(True, **cut)                                  # the counts set again: the depth starts again with them
        assert zeros()
    finally:
        engine.set_abundance(False)
    for how, (c, d, a) in got.items():
        assert a["searched"] == n and _same_counts(a, want_ab) and _same(c, d, want), how
    # the switch off: the counts alone, and the rows of today by the golden's md5
    g = json.load(open(os.path.join(GOLD, CASE + ".json")))
    engine.set_abundance(True, **cut)
    try:
        rows_off, _ = engine.search(reads)
        assert _same_counts(engine.abundance(), want_ab)
        with pytest.raises(RuntimeError, match="coverage is off"):
            engine.coverage_depth()
    finally:
        engine.set_abundance(False)
    out = str(tmp_path / "off.m8")
    engine.write_m8(out)
    assert len(rows_off) == g["m8_rows"] and hashlib.md5(open(out, "rb").read()).hexdigest() == g["m8_md5"]


def test_a_range_that_overflows_its_pools_marks_once(monkeypatch):
    """The recipe and size of test_gpu_abundance.py's test_a_range_that_overflows_its_pools_counts_once: 24,000 marker-dense reads on an
    engine of their own take the halving path (asserted).  The coverage of the one call must be that of 5,000-read batches (which fit:
    no split) and the restatement's on that run's own host rows."""
    cut = I.DENSE_CUT

    def switches(eng):
        eng.set_abundance(True, **cut)
        eng.set_coverage(True)
    runs = I.dense_runs(monkeypatch, switches, lambda eng: (eng.coverage(), eng.coverage_depth(), eng.abundance(), eng.abundance_ms(), eng.coverage_ms()))
    names, rd, lengths = runs["names"], runs["reads"], [len(s) for s in runs["seqs"]]
    (st, one), (st5, five, rows5) = runs["one"], runs["five"]
    print("one call:", st["range_splits"], "splits,", st["rows"], "rows; abundance ms", one[3], "scan ms", one[4], "of", st["ms_total"])
    assert st["range_splits"] > 0, "the batch did not overflow: the test no longer exercises the halving path"
    assert st5["range_splits"] == 0 and st5["rows"] == st["rows"] == len(rows5)
    one, five = one[:3], five[:3]
    want = V.coverage(V.rows_from_array(rows5), lengths, **cut)
    reads_want = np.bincount([s for s, _, _ in want["best"]], minlength=len(names))
    assert len(want["best"]) > 10_000 and int(want["max_depth"].max()) > 2
    for how, (c, d, a) in (("5,000-read batches", five), ("one call", one)):
        assert a["searched"] == len(rd) and a["assigned"] == len(want["best"]) and np.array_equal(a["reads"], reads_want), how
        assert _same(c, d, want), how
        assert V.invariants(c, a["reads"], lengths) == [], how


def test_refusals_through_the_abi(engine, reads):
    from microbecensus_amd import _native
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    nseq = len(engine.names)
    buf = np.zeros(nseq, np.int64)
    nres = sum(len(s) for s in _native.load_markers()[1])
    depth = np.zeros(nres + 1, np.uint32)
    assert lib.mc_set_coverage(h, 1) != 0 and "abundance counting is off" in err()
    assert lib.mc_coverage_read(h, buf.ctypes.data, None, None) != 0 and "coverage is off" in err()
    assert lib.mc_coverage_depth(h, depth.ctypes.data, nres) != 0 and "coverage is off" in err()
    assert lib.mc_coverage_ms(h) == 0.0 and lib.mc_set_coverage(h, 0) == 0       # off while off: nothing to do
    engine.set_abundance(True)
    try:
        assert lib.mc_coverage_read(h, buf.ctypes.data, None, None) != 0 and "coverage is off" in err()      # abundance on, coverage off
        engine.upload(reads[:2000])
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_coverage(h, 1) != 0 and "in flight" in err()
        engine.range_end()
        engine.set_coverage(True)
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_coverage(h, 0) != 0 and "in flight" in err()
        engine.range_end()
        assert engine.abundance()["searched"] == 2000                        # (set_coverage(True) zeroed the first range's counts)
        for n in (nres + 1, nres - 1, 0):
            assert lib.mc_coverage_depth(h, depth.ctypes.data, n) != 0 and ("holds %d values" % n) in err() and ("%d residues" % nres) in err(), err()
        # every refusal has left the handle usable: only covered asked for; everything asked for
        assert lib.mc_coverage_read(h, buf.ctypes.data, None, None) == 0
        cov, d = engine.coverage(), engine.coverage_depth()
        assert np.array_equal(buf, cov["covered"]) and int(cov["covered"].sum()) > 0 and int(d.sum()) == int(cov["spanned"].sum())
        engine.set_abundance(False)                                          # ... turns coverage off with it
        assert lib.mc_coverage_read(h, buf.ctypes.data, None, None) != 0 and "coverage is off" in err()
        assert lib.mc_set_coverage(h, 1) != 0 and "abundance counting is off" in err()
    finally:
        engine.set_abundance(False)
    rows_ok, _ = engine.search(reads[:2000])                                 # the handle is what it was
    assert len(rows_ok) > 0


HEADER_KEYS = ["metagenome", "genes", "sampled_reads", "trimmed_length", "min_ident", "min_aln", "min_bits", "average_genome_size", "ags_source",
               "genome_equivalents_sampled", "reads_assigned"]


def _header_keys(path):
    return [l[2:].split(":\t")[0] for l in open(path) if l.startswith("# ")]


def test_run_abundance_with_the_switches_end_to_end(golden, tmp_path):
    """run_abundance with the packaged markers as the genes, on the example FASTQ under config1's sample options (-n 10000; 100 bp), under
    --ags (no estimate: the test is about the table)."""
    from microbecensus_amd import _native, abundance
    want, want_ab, lengths = golden["cov"][0], golden["ab"][0], golden["lengths"]
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    names = _native.load_markers()[0]
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % (n, n.split("_")[0]) for n in names[:4000]))
    base = {"seqfiles": [fq], "genes": genes, "nreads": 10000, "device": 0, "ags": 3.0e6, "groups": str(tmp_path / "map.tsv")}
    outs = [str(tmp_path / ("genes%d.tsv" % k)) for k in range(3)]
    for out in outs[:2]:
        table, _ = abundance.run_abundance(dict(base, outfile=out))
        assert "covered_aa" not in table and "detected" not in table
    plain = open(outs[0], "rb").read()
    assert plain == open(outs[1], "rb").read() and open(outs[0] + ".groups.tsv", "rb").read() == open(outs[1] + ".groups.tsv", "rb").read()
    assert _header_keys(outs[0]) == HEADER_KEYS and _header_keys(outs[0] + ".groups.tsv") == HEADER_KEYS + ["groups"]
    lines = plain.decode().split("\n")
    assert lines[len(HEADER_KEYS)] == "gene\tlength_aa\treads\taligned_aa\trpkg" and all(l.count("\t") == 4 for l in lines[len(HEADER_KEYS):-1])
    assert open(outs[0] + ".groups.tsv").read().split("\n")[len(HEADER_KEYS) + 1] == "group\tgenes\treads\trpkg"
    # the three switches
    bed = str(tmp_path / "depth.tsv")
    table, args = abundance.run_abundance(dict(base, outfile=outs[2], coverage=True, min_breadth=0.1, depth_out=bed))
    with_cov = open(outs[2], "rb").read().decode().split("\n")
    nh = len(HEADER_KEYS)
    assert with_cov[:nh] == lines[:nh] and with_cov[nh:nh + 3] == ["# coverage:\ton", "# min_breadth:\t0.1", "# genes_detected:\t%d" % int(table["detected"].sum())]
    assert with_cov[nh + 3] == "gene\tlength_aa\treads\taligned_aa\trpkg\tcovered_aa\tbreadth\tmean_depth\tmax_depth\tdetected"
    body, body0 = [l.split("\t") for l in with_cov[nh + 4:-1]], [l.split("\t") for l in lines[nh + 1:-1]]
    assert len(body) == len(names) and [r[:5] for r in body] == body0                    # the first five columns: byte for byte
    assert [int(r[2]) for r in body] == want_ab["reads"].tolist()
    assert [int(r[5]) for r in body] == want["covered"].tolist() and [int(r[8]) for r in body] == want["max_depth"].tolist()
    assert [r[6] for r in body] == [repr(c / n) for c, n in zip(want["covered"].tolist(), lengths)]
    assert [r[7] for r in body] == [repr(s / n) for s, n in zip(want["spanned"].tolist(), lengths)]
    det = [int(r > 0 and float(c) * 1 >= 0.1 * float(n)) for r, c, n in zip(want_ab["reads"].tolist(), want["covered"].tolist(), lengths)]
    assert [int(r[9]) for r in body] == det and 0 < sum(det) < int((want_ab["reads"] > 0).sum())
    header, _ = abundance.read_table(outs[2])
    assert int(header["genes_detected"]) == sum(det) == sum(int(r[9]) for r in body)
    gh, gbody = abundance.read_table(outs[2] + ".groups.tsv")
    gh0, gbody0 = abundance.read_table(outs[0] + ".groups.tsv")
    assert [r[:4] for r in gbody] == gbody0 and sum(int(r[4]) for r in gbody) == sum(det) and gh["genes_detected"] == header["genes_detected"]
    # the depth file re-expands to the depth of the run, which is the restatement's
    assert np.array_equal(table["depth"], want["depth"])
    assert np.array_equal(abundance.read_depth(bed, names, lengths), table["depth"])
    listed = [l.split("\t")[0] for l in open(bed) if not l.startswith("#")]
    assert list(dict.fromkeys(listed)) == [n for n, r in zip(names, want_ab["reads"].tolist()) if r > 0]      # FASTA order, only genes with reads
    assert args["coverage_ms"] > 0.0
