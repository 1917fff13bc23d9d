"""The bootstrap of the gene counts end to end (csrc/mc_geneboot.h states the rule, tests/geneboot_restated.py restates it): on the marker
engine and the example reads Engine.gene_bootstrap equals the restatement applied to the best rows of the host rows the same search kept,
does not depend on how the reads reach the device, and sums to Engine.bootstrap's W[b] - one set of weights under both bootstraps; the
refusals of the ABI; run_abundance with a given AGS (the three columns equal the restatement, the existing columns are those of a run
without the switch) and with the sample's own AGS (the replicates used are the AGS report's, the scales come from its replicate values)."""
import ctypes as C
import os

import numpy as np
import pytest

import abund_inputs as I
import abundance_restated as R
import geneboot_restated as GR

pytestmark = pytest.mark.gpu

GOLD = I.GOLD
B_ENGINE, SEED = 64, 11


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return I.example_reads()


@pytest.fixture(scope="module")
def assigned(engine, reads):
    """the example reads searched once with the rows kept: (q, s) of the restatement's best rows, the device's answers of that search,
    and the scales - computed once, shared, never changed"""
    nseq = len(engine.names)
    scale = np.random.default_rng(3).uniform(1e-4, 1e-3, B_ENGINE)
    scale[[5, 40]] = [np.nan, 0.0]
    engine.set_abundance(True)
    try:
        engine.set_gene_bootstrap(len(reads))
        rows, _ = engine.search(reads)
        rows = rows.copy()
        got = engine.gene_bootstrap(B_ENGINE, SEED, scale, counts=True)
        ms, ab = engine.gene_bootstrap_ms(), engine.abundance()
    finally:
        engine.set_abundance(False)
    q, s = GR.assignments(R.rows_from_array(rows), nseq)
    return {"q": q, "s": s, "nseq": nseq, "scale": scale, "got": got, "ms": ms, "ab": ab}


def test_engine_equals_the_restatement_on_the_rows_it_kept(assigned):
    a = assigned
    want = GR.counts(a["q"], a["s"], a["nseq"], B_ENGINE, SEED)
    print("assigned", len(a["q"]), "genes with reads", int((want.sum(axis=1) > 0).sum()), "ms", a["ms"])
    assert len(a["q"]) == a["ab"]["assigned"] > 100 and a["got"]["used"] == B_ENGINE - 2 and a["got"]["dropped"] == 0 and a["ms"] > 0.0
    assert np.array_equal(a["got"]["counts"], want)
    assert GR.same_bits(a["got"]["stats"], GR.stats(want, a["scale"]))
    assert np.array_equal(np.bincount(a["s"], minlength=a["nseq"]), a["ab"]["reads"])
    assert 0.5 < want.sum(axis=0).mean() / len(a["q"]) < 1.5 and len(set(want.sum(axis=0).tolist())) > B_ENGINE // 2       # replicates differ, around the sample


def test_batches_do_not_change_it_and_both_bootstraps_share_their_weights(engine, reads, assigned, monkeypatch):
    from microbecensus_amd import _native
    a = assigned
    engine.set_abundance(True)
    try:
        engine.set_gene_bootstrap(len(reads))
        monkeypatch.setenv("MC_STREAM_BATCH", "5000")
        engine.search(reads)
        monkeypatch.delenv("MC_STREAM_BATCH")
        got = engine.gene_bootstrap(B_ENGINE, SEED, a["scale"], counts=True)
        assert np.array_equal(got["counts"], a["got"]["counts"]) and GR.same_bits(got["stats"], a["got"]["stats"])
        again = engine.gene_bootstrap(B_ENGINE, SEED, a["scale"])                 # the list is only read: a second call gives the same
        assert GR.same_bits(again["stats"], got["stats"]) and "counts" not in again
        engine.abundance_reset()
        empty = engine.gene_bootstrap(3, SEED, np.ones(3), counts=True)           # an empty list: zeros everywhere
        assert not empty["counts"].any() and not empty["stats"].any()
        # capacity one short: an ordinary refusal that names the number
        engine.set_gene_bootstrap(len(a["q"]) - 1)
        engine.search(reads)
        with pytest.raises(RuntimeError, match="mc_gene_bootstrap: 1 assigned reads did not fit the list of %d entries" % (len(a["q"]) - 1)):
            engine.gene_bootstrap(B_ENGINE, SEED, a["scale"])
        assert np.array_equal(engine.abundance()["reads"], a["ab"]["reads"])      # the counts are whole
        engine.set_gene_bootstrap(0)
        engine.abundance_reset()
        engine.search(reads)
        assert np.array_equal(engine.abundance()["reads"], a["ab"]["reads"])      # the switch off again: the counts as before
    finally:
        engine.set_abundance(False)
    # the AGS bootstrap on the same reads, its family parameters bypassed: every assigned read a best hit of family 0
    best = np.zeros(len(a["q"]), _native.BEST_DTYPE)
    best["read"], best["family"], best["aln"], best["target_len"] = a["q"], 0, 1, 1
    si, _ = engine.bootstrap(best, ["hits"], B_ENGINE, SEED)
    assert np.array_equal(a["got"]["counts"].sum(axis=0), si[:, -1]) and np.array_equal(si[:, 0], si[:, -1])


def test_refusals_through_the_abi(engine, reads):
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    nseq = len(engine.names)
    scale, stats, dropped = np.ones(4), np.zeros(6 * nseq), C.c_int64(-1)
    assert lib.mc_set_gene_bootstrap(h, 100) != 0 and "abundance counting is off" in err() and "capacity = 100" in err()
    assert lib.mc_gene_bootstrap(h, 4, 0, scale.ctypes.data, None, stats.ctypes.data, C.byref(dropped)) != 0 and "the gene bootstrap is off" in err()
    assert lib.mc_gene_bootstrap_ms(h) == 0.0 and lib.mc_set_gene_bootstrap(h, 0) == 0      # off while off: nothing to do
    engine.set_abundance(True)
    try:
        assert lib.mc_set_gene_bootstrap(h, -1) != 0 and "capacity -1 is not a number of reads from 0 to 2^31 - 1" in err()
        assert lib.mc_set_gene_bootstrap(h, 1 << 31) != 0 and "capacity 2147483648 is not" in err()
        assert lib.mc_gene_bootstrap(h, 4, 0, scale.ctypes.data, None, stats.ctypes.data, C.byref(dropped)) != 0 and "the gene bootstrap is off" in err()   # every refusal left it off
        engine.set_gene_bootstrap(1000)
        for bad in (0, -3, 4097):
            assert lib.mc_gene_bootstrap(h, bad, 0, scale.ctypes.data, None, stats.ctypes.data, C.byref(dropped)) != 0 and "B %d is not a number of replicates from 1 to 4096" % bad in err()
        assert lib.mc_gene_bootstrap(h, 4, 0, None, None, stats.ctypes.data, C.byref(dropped)) != 0 and "NULL scale or stats" in err()
        with pytest.raises(ValueError, match="scale holds 4 values, B is 5"):
            engine.gene_bootstrap(5, 0, scale)
        with pytest.raises(RuntimeError, match="mc_search_varlen: refused while the gene bootstrap is on .*capacity = 1000"):
            engine.search_varlen([bytes(reads[0]), bytes(reads[1][:90])])
        engine.upload(reads[:500])
        engine.range_begin(0, 500, 0)
        try:
            assert lib.mc_set_gene_bootstrap(h, 10) != 0 and "still in flight" in err()
            assert lib.mc_gene_bootstrap(h, 4, 0, scale.ctypes.data, None, stats.ctypes.data, C.byref(dropped)) != 0 and "still in flight" in err()
        finally:
            engine.range_end()
        assert lib.mc_gene_bootstrap(h, 4, 0, scale.ctypes.data, None, stats.ctypes.data, C.byref(dropped)) == 0 and dropped.value == 0
        assert lib.mc_set_gene_bootstrap(h, 0) == 0
        engine.search_varlen([bytes(reads[0]), bytes(reads[1][:90])])             # off: mixed lengths are searched again
    finally:
        engine.set_abundance(False)
    assert lib.mc_gene_bootstrap(h, 4, 0, scale.ctypes.data, None, stats.ctypes.data, C.byref(dropped)) != 0 and "the gene bootstrap is off" in err()   # the counts going off took it with them


def _without_boot(path):
    """the lines of a gene table with the switch's header lines and its three columns taken away"""
    out = []
    for line in open(path).read().split("\n"):
        if line.startswith("# bootstrap"):
            continue
        out.append(line if line.startswith("#") or not line else line.rsplit("\t", 3)[0])
    return out


def test_run_abundance_with_a_given_ags(assigned, tmp_path):
    """--ags VALUE, B = 100 on the golden example file, with coverage, ties and groups on: the three columns equal the restatement; the
    existing columns, the groups table and the depth are those of a run without the switch.  (rpkg need not lie inside its interval.)"""
    from microbecensus_amd import _native, abundance
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % (n, n.split("_")[0]) for n in _native.load_markers()[0][:4000]))

    def run(out, **kw):
        return abundance.run_abundance(dict({"seqfiles": [fq], "genes": genes, "outfile": str(tmp_path / out), "nreads": 10000, "device": 0, "ags": 3.0e6, "coverage": True,
                                             "ties": True, "groups": str(tmp_path / "map.tsv")}, **kw))
    table, args = run("boot.tsv", bootstrap=100, bootstrap_seed=5)
    plain, _ = run("plain.tsv")
    a = assigned
    assert table["sampled_reads"] == 8672 and np.array_equal(table["reads"], a["ab"]["reads"]) and args["gene_bootstrap_ms"] > 0.0
    scale = np.full(100, 1.0 / table["genome_equivalents_sampled"])
    want = GR.stats(GR.counts(a["q"], a["s"], a["nseq"], 100, 5), scale)
    assert GR.same_bits(table["boot_stats"], want) and table["boot_used"] == 100 and np.array_equal(table["boot_scale"], scale)
    se, lo, hi = abundance.boot_columns(want, 100, table["length_aa"])
    for name, col in (("rpkg_boot_se", se), ("rpkg_ci95_low", lo), ("rpkg_ci95_high", hi)):
        assert GR.same_bits(table[name], col), name
    hit = table["reads"] > 0
    kb = 3.0 * table["length_aa"] / 1000.0
    c = GR.counts(a["q"], a["s"], a["nseq"], 100, 5)
    g = int(np.argmax(table["reads"]))
    v = c[g].astype(np.float64) * scale / kb[g]
    assert [lo[g], hi[g]] == np.percentile(v, [2.5, 97.5]).tolist() and se[g] == pytest.approx(np.std(v, ddof=1), rel=1e-9)
    assert (se[hit] > 0).all() and not se[~hit].any() and not hi[~hit].any() and (lo <= hi).all()
    # the files
    assert _without_boot(str(tmp_path / "boot.tsv")) == open(str(tmp_path / "plain.tsv")).read().split("\n")
    assert open(str(tmp_path / "boot.tsv.groups.tsv")).read() == open(str(tmp_path / "plain.tsv.groups.tsv")).read()
    header, rows = abundance.read_table(str(tmp_path / "boot.tsv"))
    assert (header["bootstrap"], header["bootstrap_seed"], header["bootstrap_replicates"], header["bootstrap_denominator"]) == ("100", "5", "100/100", "fixed_ags")
    assert [r[-3:] for r in rows] == [[repr(float(x)) for x in t] for t in zip(se, lo, hi)]
    for key in ("reads", "aligned_aa", "rpkg", "covered_aa", "unique_reads", "shared_reads"):
        assert np.array_equal(table[key], plain[key]), key
    assert "rpkg_boot_se" not in plain and "bootstrap" not in abundance.read_table(str(tmp_path / "plain.tsv"))[0]


def test_run_abundance_with_the_samples_own_ags(assigned, tmp_path):
    """The default AGS source: replicate b of the counts is divided by replicate b of the genome equivalents - run_pipeline's bootstrap
    under the same seed gives every replicate its AGS and its read count."""
    from microbecensus_amd import _native, abundance, microbe_census
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    B, S = 64, 7
    table, args = abundance.run_abundance({"seqfiles": [fq], "genes": genes, "outfile": str(tmp_path / "own.tsv"), "nreads": 10000, "device": 0, "bootstrap": B, "bootstrap_seed": S})
    est, pargs = microbe_census.run_pipeline({"seqfiles": [fq], "nreads": 10000, "device": 0, "bootstrap": B, "bootstrap_seed": S})
    assert table["ags_source"] == "run_pipeline" and table["ags"] == est
    used, asked = pargs["ags_boot_replicates"]
    header, _ = abundance.read_table(str(tmp_path / "own.tsv"))
    assert header["bootstrap_replicates"] == "%d/%d" % (used, asked) and asked == B and table["boot_used"] == used > B // 2 and header["bootstrap_denominator"] == "replicate_ags"
    assert len(pargs["ags_boot_reads"]) == B and args["ags_boot_values"] == pargs["ags_boot_values"] and args["ags_boot_reads"] == pargs["ags_boot_reads"]
    scale = abundance.boot_scale(pargs["ags_boot_values"], pargs["ags_boot_reads"], 100)
    assert GR.same_bits(table["boot_scale"], scale) and int(GR.used(scale).sum()) == used
    n_b = np.array(pargs["ags_boot_reads"])
    assert abs(n_b.mean() / table["sampled_reads"] - 1.0) < 0.02 and len(set(n_b.tolist())) > B // 2                 # every replicate its own read count, around the sample's
    a = assigned
    want = GR.stats(GR.counts(a["q"], a["s"], a["nseq"], B, S), scale)
    assert GR.same_bits(table["boot_stats"], want)
    se, lo, hi = abundance.boot_columns(want, used, table["length_aa"])
    assert GR.same_bits(table["rpkg_boot_se"], se) and GR.same_bits(table["rpkg_ci95_low"], lo) and GR.same_bits(table["rpkg_ci95_high"], hi)
