"""The depth statistics on the device end to end (mc_depth_stats; csrc/mc_depthstats.h states the rule): Engine.depth_stats on the example reads
and the marker database against tests/depthstats_restated.py applied to Engine.coverage_depth() of the same run - and, for the any-depth, to
the spans of tests/ties_restated.py's tied sets on the run's own host rows; the invariants; independence from batches; run_abundance with
the switch - the new columns against the restatement, every other column, the groups file and the depth file byte for byte; long genes in
gene space; the refusals of the ABI."""
import os

import numpy as np
import pytest

import abund_inputs as AI
import abundance_table_cases as TC
import coverage_restated as V
import depthstats_restated as D
import fold_restated as FR
import ties_restated as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
KEEPS = (80, 100)


def _same(got, want):
    return all(np.array_equal(got[k], want[k]) for k in D.FIGURES) and got["keep"] == want["keep"]


@pytest.fixture(scope="module")
def engine():
    yield from AI.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return AI.example_reads()


@pytest.fixture(scope="module")
def run(engine, reads):
    """one search with coverage and ties on - computed once, shared, never changed: the device's reads at both percents of both depths, and what
    the restatement needs"""
    from microbecensus_amd import _native
    lengths = [len(s) for s in _native.load_markers()[1]]
    engine.set_abundance(True)
    try:
        engine.set_coverage(True)
        engine.set_ties(True)
        rows = engine.search(reads)[0].copy()
        r = {"lengths": lengths, "ab": engine.abundance(), "cov": engine.coverage(), "tcov": engine.ties_coverage(), "ti": engine.ties(), "depth": engine.coverage_depth(),
             "got": {P: engine.depth_stats(P) for P in KEEPS}, "got_any": {P: engine.depth_stats(P, any=True) for P in KEEPS}, "ms": engine.depth_stats_ms(),
             "default": engine.depth_stats()}
    finally:
        engine.set_abundance(False)
    sets = T.tied_sets(V.rows_from_array(rows), len(lengths))
    r["depth_any"] = D.depth_of_spans([m for _, members in sets for m in members], lengths)
    return r


def test_engine_equals_the_restatement_on_its_own_depth(run):
    lengths, has = run["lengths"], run["ab"]["reads"] > 0
    assert run["depth"].size == sum(lengths) and run["ms"] > 0.0 and int(has.sum()) > 200
    for P in KEEPS:
        got, want = run["got"][P], D.depth_stats(run["depth"], lengths, has, P)
        assert all(got[k].dtype == np.int64 and got[k].shape == (len(lengths),) for k in D.FIGURES)
        assert _same(got, want), "P = %d" % P
        assert D.invariants(got, run["cov"]["spanned"], run["cov"]["max_depth"]) == []
        assert not any(got[k][~has].any() for k in D.FIGURES), "a gene without reads has four zeros"
    assert np.array_equal(run["got"][100]["trimmed_sum"], run["cov"]["spanned"]) and int(run["got"][100]["high"].max()) == int(run["cov"]["max_depth"].max()) > 0
    assert _same(run["default"], run["got"][80]), "the default percent is 80"
    print("depth stats: %d genes with reads, median > 0 in %d, tad80 > 0 in %d, %.4f ms for %d reads" % (
        int(has.sum()), int((run["got"][80]["median"] > 0).sum()), int((run["got"][80]["trimmed_sum"] > 0).sum()), run["ms"], 2 * len(KEEPS) + 1))


def test_the_any_depth_equals_the_restatement_on_the_tied_sets(run):
    lengths, cand = run["lengths"], run["ti"]["candidates"] > 0
    assert int(run["depth_any"].sum()) == int(run["tcov"]["spanned_any"].sum()) > int(run["cov"]["spanned"].sum()), "the restated any-depth is the device's, and differs from the depth"
    for P in KEEPS:
        got = run["got_any"][P]
        assert _same(got, D.depth_stats(run["depth_any"], lengths, cand, P)), "P = %d" % P
        assert D.invariants(got, run["tcov"]["spanned_any"], run["tcov"]["max_depth_any"]) == []
        assert (got["trimmed_sum"] >= run["got"][P]["trimmed_sum"]).all() and (got["median"] >= run["got"][P]["median"]).all()
    assert np.array_equal(run["got_any"][100]["trimmed_sum"], run["tcov"]["spanned_any"])
    assert not _same(run["got_any"][100], run["got"][100])


def test_batches_give_the_same_integers(engine, reads, run, monkeypatch):
    engine.set_abundance(True)
    try:
        engine.set_coverage(True)
        monkeypatch.setenv("MC_STREAM_BATCH", "5000")
        engine.search(reads)
        monkeypatch.delenv("MC_STREAM_BATCH")
        first = engine.depth_stats(80)
        engine.search(reads[:1000], first_read_id=len(reads))        # the read changed nothing: ranges go on marking behind it
        more, cov = engine.depth_stats(100), engine.coverage()
        engine.abundance_reset()
        zeros, ms = engine.depth_stats(80), engine.depth_stats_ms()
    finally:
        engine.set_abundance(False)
    assert _same(first, run["got"][80]), "one run in 5,000-read batches"
    assert np.array_equal(more["trimmed_sum"], cov["spanned"]) and int(more["trimmed_sum"].sum()) > int(run["cov"]["spanned"].sum())
    assert not any(zeros[k].any() for k in D.FIGURES) and ms > 0.0, "a reset zeroes the depth, and the time before the read that followed it"


def test_refusals_through_the_abi(engine, reads):
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    buf = np.zeros(len(engine.names), np.int64)
    assert lib.mc_depth_stats(h, 80, 0, buf.ctypes.data, None, None, None) != 0 and "coverage is off" in err() and "keep_percent = 80" in err()
    assert lib.mc_depth_stats_ms(h) == 0.0
    engine.set_abundance(True)
    try:
        with pytest.raises(RuntimeError, match=r"coverage is off \(mc_set_coverage\)"):
            engine.depth_stats(80)
        engine.set_coverage(True)
        for P in (0, 101, -1, 1000):
            with pytest.raises(RuntimeError, match="keep_percent %d is not a percent from 1 to 100" % P):
                engine.depth_stats(P)
        with pytest.raises(RuntimeError, match=r"any = 1 while ties are off \(mc_set_ties\)"):
            engine.depth_stats(80, any=True)
        engine.upload(reads[:2000])
        engine.range_begin(0, 2000, 0)
        assert lib.mc_depth_stats(h, 80, 0, buf.ctypes.data, None, None, None) != 0 and "in flight" in err() and "keep_percent = 80" in err()
        engine.range_end()
        # every refusal has left the handle usable: only the median asked for; nothing asked for; everything
        assert lib.mc_depth_stats(h, 100, 0, buf.ctypes.data, None, None, None) == 0 and lib.mc_depth_stats(h, 1, 0, None, None, None, None) == 0
        st, cov = engine.depth_stats(100), engine.coverage()
        assert np.array_equal(buf, st["median"]) and np.array_equal(st["trimmed_sum"], cov["spanned"]) and int(cov["spanned"].sum()) > 0
        engine.set_ties(True)                                           # (zeroes everything)
        assert not engine.depth_stats(80, any=True)["high"].any()
        engine.set_coverage(False)
        with pytest.raises(RuntimeError, match="coverage is off"):
            engine.depth_stats(80, any=True)
    finally:
        engine.set_abundance(False)
    rows_ok, _ = engine.search(reads[:2000])                            # the handle is what it was
    assert len(rows_ok) > 0


def _strip(path, drop_header, keep_cols):
    """the lines of a table without the header lines `drop_header` and with its first keep_cols columns alone"""
    out = []
    for line in open(path).read().split("\n"):
        if line.startswith("# "):
            if line[2:].split(":\t")[0] not in drop_header:
                out.append(line)
        else:
            out.append("\t".join(line.split("\t")[:keep_cols]) if line else line)
    return "\n".join(out)


def test_run_abundance_with_the_switch_end_to_end(run, tmp_path):
    """run_abundance with the packaged markers as the genes, on the example FASTQ under config1's sample options (-n 10000; 100 bp), under --ags,
    with coverage, ties, groups and the depth file in both runs: the new columns are the restatement's on the run's own depth, and the run
    without the switch writes the same bytes less the new columns and header lines."""
    from microbecensus_amd import _native, abundance
    names, _ = _native.load_markers()
    lengths = run["lengths"]
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % (n, n.split("_")[0]) for n in names[:4000]))
    base = {"seqfiles": [fq], "genes": os.path.join(_native.DATA_DIR, "markers.faa.gz"), "nreads": 10000, "device": 0, "ags": 3.0e6, "groups": str(tmp_path / "map.tsv"),
            "coverage": True, "ties": True}
    off, on = str(tmp_path / "off.tsv"), str(tmp_path / "on.tsv")
    plain, _ = abundance.run_abundance(dict(base, outfile=off, depth_out=off + ".depth"))
    assert "depth_stats" not in plain and "median_depth" not in plain and "tad_keep" not in plain
    table, args = abundance.run_abundance(dict(base, outfile=on, depth_out=on + ".depth", depth_stats=True))
    assert args["depth_stats"] is True and args["tad_keep"] == 80 and args["depth_stats_ms"] > 0.0 and table["tad_keep"] == 80
    # the device's figures are the restatement's on the depth of this run - which is the engine fixture's: the same reads
    want = D.depth_stats(table["depth"], lengths, table["reads"] > 0, 80)
    assert np.array_equal(table["depth"], run["depth"]) and _same(table["depth_stats"], want) and _same(table["depth_stats"], run["got"][80])
    assert _same(table["depth_stats_any"], run["got_any"][80])
    # without the switch: byte for byte
    ncol = len(next(l for l in open(off) if l.startswith("gene\t")).split("\t"))
    assert open(off).read() == _strip(on, ("depth_stats", "tad_keep"), ncol)
    assert open(off + ".groups.tsv", "rb").read() == open(on + ".groups.tsv", "rb").read() and open(off + ".depth", "rb").read() == open(on + ".depth", "rb").read()
    # the gene table parses back
    header, body = abundance.read_table(on)
    cols = open(on).read().split("\n")[len(header)].split("\t")
    assert header["depth_stats"] == "on" and header["tad_keep"] == "80" and len(body) == len(names)
    assert cols[ncol:] == ["median_depth", "tad80", "tad80_per_ge", "median_depth_any", "tad80_any"]
    ge = table["genome_equivalents_sampled"]
    tad, tad_any = D.tad(want["trimmed_sum"], lengths, 80), D.tad(run["got_any"][80]["trimmed_sum"], lengths, 80)
    assert [int(r[ncol]) for r in body] == want["median"].tolist() and [int(r[ncol + 3]) for r in body] == run["got_any"][80]["median"].tolist()
    assert [r[ncol + 1] for r in body] == [repr(float(v)) for v in tad] and [r[ncol + 2] for r in body] == [repr(float(v / ge)) for v in tad]
    assert [r[ncol + 4] for r in body] == [repr(float(v)) for v in tad_any]
    none = ~(table["reads"] > 0) & ~(run["ti"]["candidates"] > 0)
    assert int(none.sum()) > 0 and all(body[g][ncol:] == ["0", "0.0", "0.0", "0", "0.0"] for g in np.flatnonzero(none)[:50])
    assert sum(1 for r in body if r[ncol + 1] != "0.0") == int((want["trimmed_sum"] > 0).sum()) > 0


def test_long_genes_in_gene_space():
    """test_gpu_fold.py's database (every second marker, cut at 768 with the fold's overlap): the figures are the GENES' - mc_abundance_count() of
    them - and the restatement's on the gene-space depth of the same engine."""
    from microbecensus_amd import _native, abundance
    names, seqs = TC.long_gene_markers()
    reads = AI.example_reads()
    sp = abundance.split_genes(names, seqs, seg_len=768, overlap=FR.V)
    eng = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"])
    try:
        eng.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
        eng.set_run(100)
        eng.set_abundance(True)
        eng.set_coverage(True)
        eng.search(reads)
        ngenes, got, depth, ab, cov = eng.abundance_count(), {P: eng.depth_stats(P) for P in KEEPS}, eng.coverage_depth(), eng.abundance(), eng.coverage()
    finally:
        eng.close()
    lengths = [int(n) for n in sp["gene_len"]]
    split_hit = [g for g in np.flatnonzero(ab["reads"]) if (sp["seg_gene"] == g).sum() > 1]
    print("long genes: %d genes, %d split, %d segments, genes with reads %d of which split %d, the longest %d" % (len(names), sp["genes_split"], len(sp["seg_names"]), int((ab["reads"] > 0).sum()), len(split_hit), max(lengths)))
    assert ngenes == len(names) == len(lengths) < len(sp["seg_names"]) and depth.size == sum(lengths) and len(split_hit) > 0
    for P in KEEPS:
        assert got[P]["median"].shape == (ngenes,) and _same(got[P], D.depth_stats(depth, lengths, ab["reads"] > 0, P)), "P = %d" % P
        assert D.invariants(got[P], cov["spanned"], cov["max_depth"]) == []
