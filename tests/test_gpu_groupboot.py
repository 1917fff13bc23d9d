"""The bootstrap of the groups table end to end (csrc/mc_groupboot.h states the rule, tests/groupboot_restated.py restates it): on the marker
engine and the example reads Engine.group_bootstrap equals the restatement applied to the replicate counts Engine.gene_bootstrap(counts=True)
returns, behind that call and on its own, in one call and in 5,000-read batches, and its counts sum to Engine.bootstrap's W[b]; the refusals
of the ABI; run_abundance with a given AGS and a map that groups genes by family and leaves some unnamed (the three group columns equal the
restatement, the gene table is that of the run without the switch byte for byte, every existing byte of the groups table is unchanged, an
unnamed gene's group row carries its gene row's interval) and with the sample's own AGS (the groups header names the gene table's
replicates)."""
import ctypes as C
import os

import numpy as np
import pytest

import abund_inputs as I
import abundance_restated as R
import geneboot_restated as GR
import groupboot_restated as GRR

pytestmark = pytest.mark.gpu

GOLD = I.GOLD
B_ENGINE, SEED = 64, 11


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return I.example_reads()


def _family_map(names, named=4000):
    """{gene: family} of the first `named` genes: the others stay unnamed, groups of their own"""
    return {n: n.split("_")[0] for n in names[:named]}


@pytest.fixture(scope="module")
def searched(engine, reads):
    """the example reads searched once with the rows kept: the restatement's assigned reads, the device's gene replicate counts, and the
    group read behind that gene read - computed once, shared, never changed"""
    from microbecensus_amd import _native, abundance
    names, seqs = _native.load_markers()
    nseq = len(engine.names)
    assert list(engine.names) == list(names)
    scale = np.random.default_rng(3).uniform(1e-4, 1e-3, B_ENGINE)
    scale[[5, 40]] = [np.nan, 0.0]
    ids, gnames = abundance.group_ids(names, _family_map(names))
    kb = 3.0 * np.array([len(s) for s in seqs], np.float64) / 1000.0
    engine.set_abundance(True)
    try:
        engine.set_gene_bootstrap(len(reads))
        rows, _ = engine.search(reads)
        rows = rows.copy()
        gene = engine.gene_bootstrap(B_ENGINE, SEED, scale, counts=True)
        behind = engine.group_bootstrap(B_ENGINE, SEED, scale, ids, len(gnames), kb, counts=True)
        ms = engine.group_bootstrap_ms()
    finally:
        engine.set_abundance(False)
    q, s = GR.assignments(R.rows_from_array(rows), nseq)
    y, Cm = GRR.values(gene["counts"], scale, ids, len(gnames), kb)
    return {"q": q, "s": s, "nseq": nseq, "scale": scale, "ids": ids, "ngroups": len(gnames), "kb": kb, "gene": gene, "behind": behind, "ms": ms, "y": y, "C": Cm,
            "stats": GRR.stats(y, scale)}


def test_engine_equals_the_restatement_on_the_gene_replicate_counts(searched):
    a = searched
    live = int((a["C"].sum(axis=1) > 0).sum())
    print("groups", a["ngroups"], "with reads", live, "ms", a["ms"])
    assert 1 < a["ngroups"] < a["nseq"] and live > 20 and a["behind"]["used"] == B_ENGINE - 2 and a["behind"]["dropped"] == 0 and a["ms"] > 0.0
    assert np.array_equal(a["behind"]["counts"], a["C"])
    assert GR.same_bits(a["behind"]["stats"], a["stats"])
    assert (np.bincount(a["ids"][a["ids"] < 40]) > 1).any() and (a["stats"][:, 1] > 0).sum() == live       # groups of several genes; every live group varies


def test_on_its_own_in_batches_and_both_bootstraps_share_their_weights(engine, reads, searched, monkeypatch):
    from microbecensus_amd import _native
    a = searched
    engine.set_abundance(True)
    try:
        engine.set_gene_bootstrap(len(reads))
        monkeypatch.setenv("MC_STREAM_BATCH", "5000")
        engine.search(reads)
        monkeypatch.delenv("MC_STREAM_BATCH")
        own = engine.group_bootstrap(B_ENGINE, SEED, a["scale"], a["ids"], a["ngroups"], a["kb"], counts=True)     # no gene read before it: it makes the replicate counts
        assert np.array_equal(own["counts"], a["C"]) and GR.same_bits(own["stats"], a["stats"])
        again = engine.group_bootstrap(B_ENGINE, SEED, a["scale"], a["ids"], a["ngroups"], a["kb"])                # and takes its own over
        assert GR.same_bits(again["stats"], a["stats"]) and "counts" not in again
        other = engine.group_bootstrap(B_ENGINE, SEED + 1, a["scale"], a["ids"], a["ngroups"], a["kb"])            # another seed: other replicates, made anew
        assert not GR.same_bits(other["stats"], a["stats"])
        back = engine.group_bootstrap(B_ENGINE, SEED, a["scale"], a["ids"], a["ngroups"], a["kb"])
        assert GR.same_bits(back["stats"], a["stats"])
        one = engine.group_bootstrap(B_ENGINE, SEED, a["scale"], np.zeros(a["nseq"], np.int32), 1, a["kb"], counts=True)   # one group of every gene
        assert np.array_equal(one["counts"][0], a["gene"]["counts"].sum(axis=0))
        assert GR.same_bits(one["stats"], GRR.stats(GRR.values(a["gene"]["counts"], a["scale"], np.zeros(a["nseq"], np.int32), 1, a["kb"])[0], a["scale"]))
        engine.abundance_reset()
        empty = engine.group_bootstrap(3, SEED, np.ones(3), a["ids"], a["ngroups"], a["kb"], counts=True)          # an empty list: zeros everywhere
        assert not empty["counts"].any() and not empty["stats"].any()
    finally:
        engine.set_abundance(False)
    # the AGS bootstrap on the same reads, its family parameters bypassed: every assigned read a best hit of family 0
    best = np.zeros(len(a["q"]), _native.BEST_DTYPE)
    best["read"], best["family"], best["aln"], best["target_len"] = a["q"], 0, 1, 1
    si, _ = engine.bootstrap(best, ["hits"], B_ENGINE, SEED)
    assert np.array_equal(a["behind"]["counts"].sum(axis=0), si[:, -1])


def test_refusals_through_the_abi(engine, reads, searched):
    lib, h, a = engine.lib, engine.h, searched

    def err():
        return lib.mc_last_error().decode()
    nseq = a["nseq"]
    scale, stats, dropped = np.ones(4), np.zeros(6 * nseq), C.c_int64(-1)
    gof, kb = np.zeros(nseq, np.int32), np.ones(nseq)

    def call(B=4, sc=scale, g=gof, ng=1, k=kb, st=stats):
        ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        return lib.mc_group_bootstrap(h, B, 0, ptr(sc), ptr(g), ng, ptr(k), None, ptr(st), C.byref(dropped))
    assert call() != 0 and "mc_group_bootstrap: the gene bootstrap is off" in err() and lib.mc_group_bootstrap_ms(h) == 0.0
    engine.set_abundance(True)
    try:
        assert call() != 0 and "the gene bootstrap is off" in err()
        engine.set_gene_bootstrap(1000)
        for bad in (0, -3, 4097):
            assert call(B=bad) != 0 and "B %d is not a number of replicates from 1 to 4096" % bad in err()
        for name in ("sc", "g", "k", "st"):
            assert call(**{name: None}) != 0 and "NULL scale, group_of, gene_kb or stats" in err(), name
        for bad in (0, -1, nseq + 1):
            assert call(ng=bad) != 0 and "ngroups %d is not a number of groups from 1 to %d" % (bad, nseq) in err()
        for bad in (-1, 2):
            g = gof.copy(); g[7] = bad
            assert call(g=g, ng=2) != 0 and "group_of[7] = %d is not a group from 0 to 1" % bad in err()
        for bad, shown in ((0.0, "0.0"), (-3.0, "-3.0"), (np.nan, "nan"), (np.inf, "inf")):
            k = kb.copy(); k[9] = bad
            assert call(k=k) != 0 and "gene_kb[9] = " in err() and "is not a finite number > 0" in err() and shown.rstrip("0").rstrip(".") in err(), shown
        with pytest.raises(ValueError, match="scale holds 4 values, B is 5"):
            engine.group_bootstrap(5, 0, scale, gof, 1, kb)
        with pytest.raises(ValueError, match="group_of holds 3 values"):
            engine.group_bootstrap(4, 0, scale, gof[:3], 1, kb)
        engine.upload(reads[:500])
        engine.range_begin(0, 500, 0)
        try:
            assert call() != 0 and "mc_group_bootstrap: a range begun with mc_range_begin() is still in flight" in err()
        finally:
            engine.range_end()
        assert call() == 0 and dropped.value == 0 and lib.mc_group_bootstrap_ms(h) > 0.0
        engine.set_gene_bootstrap(len(a["q"]) - 1)                                    # capacity one short: an ordinary refusal that names the number
        engine.search(reads)
        assert call() != 0 and "mc_group_bootstrap: 1 assigned reads did not fit the list of %d entries" % (len(a["q"]) - 1) in err() and dropped.value == 1
    finally:
        engine.set_abundance(False)
    assert call() != 0 and "the gene bootstrap is off" in err() and lib.mc_group_bootstrap_ms(h) == 0.0


def _without_boot(path):
    """the lines of a table with the bootstrap's header lines and its three columns taken away"""
    out = []
    for line in open(path).read().split("\n"):
        if line.startswith("# bootstrap"):
            continue
        out.append(line if line.startswith("#") or not line else line.rsplit("\t", 3)[0])
    return out


def test_run_abundance_with_a_given_ags(searched, tmp_path):
    """--ags VALUE, B = 100 on the golden example file with coverage, ties and a map by family that leaves the genes behind the first 4,000
    unnamed: the three group columns equal the restatement; the gene table is that of the run without the switch byte for byte; every
    existing byte of the groups table is unchanged; an unnamed gene's group row carries its gene row's interval bit for bit and its
    standard error within a relative 1e-12."""
    from microbecensus_amd import _native, abundance
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    names = _native.load_markers()[0]
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % kv for kv in _family_map(names).items()))

    def run(out, **kw):
        return abundance.run_abundance(dict({"seqfiles": [fq], "genes": genes, "outfile": str(tmp_path / out), "nreads": 10000, "device": 0, "ags": 3.0e6, "coverage": True,
                                             "ties": True, "groups": str(tmp_path / "map.tsv"), "bootstrap": 100, "bootstrap_seed": 5}, **kw))
    table, args = run("grp.tsv", bootstrap_groups=True)
    plain, pargs = run("plain.tsv")
    a = searched
    assert table["sampled_reads"] == 8672 and args["group_bootstrap_ms"] > 0.0 and "group_bootstrap_ms" not in pargs and "groups_boot" not in plain
    scale = np.full(100, 1.0 / table["genome_equivalents_sampled"])
    cm = GR.counts(a["q"], a["s"], a["nseq"], 100, 5)
    assert np.array_equal(cm.sum(axis=1) > 0, table["reads"] > 0)
    y, _ = GRR.values(cm, scale, a["ids"], a["ngroups"], a["kb"])
    want = GRR.stats(y, scale)
    assert GR.same_bits(table["groups_boot_stats"], want) and len(table["groups_boot"]) == len(table["groups"]) == a["ngroups"]
    se, lo, hi = abundance.group_boot_columns(want, 100)
    got = np.array(table["groups_boot"], np.float64)
    assert GR.same_bits(got[:, 0], se) and GR.same_bits(got[:, 1], lo) and GR.same_bits(got[:, 2], hi)
    G = int(np.argmax([g[2] for g in table["groups"]]))
    assert [lo[G], hi[G]] == np.percentile(y[G], [2.5, 97.5]).tolist() and se[G] == pytest.approx(np.std(y[G], ddof=1), rel=1e-12)
    # the files
    assert open(str(tmp_path / "grp.tsv")).read() == open(str(tmp_path / "plain.tsv")).read()
    assert _without_boot(str(tmp_path / "grp.tsv.groups.tsv")) == open(str(tmp_path / "plain.tsv.groups.tsv")).read().split("\n")
    gh, grows = abundance.read_table(str(tmp_path / "grp.tsv.groups.tsv"))
    th, trows = abundance.read_table(str(tmp_path / "grp.tsv"))
    assert gh["bootstrap_groups"] == "on" and all(gh[k] == th[k] for k in ("bootstrap", "bootstrap_seed", "bootstrap_replicates", "bootstrap_denominator")) and gh["bootstrap_replicates"] == "100/100"
    assert "bootstrap_groups" not in th and "bootstrap" not in abundance.read_table(str(tmp_path / "plain.tsv.groups.tsv"))[0]
    assert [r[-3:] for r in grows] == [[repr(float(x)) for x in t] for t in zip(se, lo, hi)]
    # unnamed genes: groups of one
    by_gene = {r[0]: r for r in trows}
    where = {n: k for k, n in enumerate(names)}
    singles = 0
    for k, (grp, ngenes, nreads, _v) in enumerate(g[:4] for g in table["groups"]):
        if grp in by_gene and ngenes == 1:
            s = where[grp]
            assert grows[k][-2:] == by_gene[grp][-2:] and GR.same_bits(got[k, 1:], [table["rpkg_ci95_low"][s], table["rpkg_ci95_high"][s]]), grp
            assert got[k, 0] == pytest.approx(table["rpkg_boot_se"][s], rel=1e-12, abs=0.0), grp
            singles += nreads > 0
    assert singles > 20
    # a group's standard error never exceeds the sum of its members'
    msum = np.bincount(a["ids"], weights=table["rpkg_boot_se"], minlength=a["ngroups"])
    assert (got[:, 0] <= msum * (1.0 + 1e-9)).all()


def test_the_samples_own_ags_gives_the_groups_the_gene_tables_replicates(tmp_path):
    """The default AGS source: the scales are run_pipeline's replicates, some of them unused; the groups header names the same replicates as the
    gene table's, and the group columns are made of that many."""
    from microbecensus_amd import _native, abundance
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    names = _native.load_markers()[0]
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % kv for kv in _family_map(names).items()))
    table, args = abundance.run_abundance({"seqfiles": [fq], "genes": genes, "outfile": str(tmp_path / "own.tsv"), "nreads": 10000, "device": 0, "bootstrap": 64, "bootstrap_seed": 7,
                                           "groups": str(tmp_path / "map.tsv"), "bootstrap_groups": True})
    gh, grows = abundance.read_table(str(tmp_path / "own.tsv.groups.tsv"))
    th, _ = abundance.read_table(str(tmp_path / "own.tsv"))
    assert gh["bootstrap_replicates"] == th["bootstrap_replicates"] == "%d/64" % table["boot_used"] and gh["bootstrap_denominator"] == "replicate_ags" and gh["bootstrap_groups"] == "on"
    se, lo, hi = abundance.group_boot_columns(table["groups_boot_stats"], table["boot_used"])
    assert [r[-3:] for r in grows] == [[repr(float(x)) for x in t] for t in zip(se, lo, hi)] and (lo <= hi).all() and (se[[g[2] > 0 for g in table["groups"]]] > 0).all()
