"""The bootstrap of the tie shares end to end (csrc/mc_tieboot.h states the rule, tests/tieboot_restated.py restates it): the example reads
against the packaged markers, as test_gpu_geneboot.py runs them, with --ties --bootstrap 64 --bootstrap-ties - the three new columns equal
boot_columns of the restatement applied to the rows of a keep_rows search of the same reads; the two device matrices keep the statement's
invariant; without the switch every file is what it was; a gene none of whose reads tie carries its rpkg interval; a list too small is
refused with the factor that fits; and the same under --mixed-lengths with --ags and under a gene fold at test_gpu_fold.py's (768, V)."""
import os

import numpy as np
import pytest

import abund_inputs as I
import abundance_table_cases as TC
import classes_restated as cr
import coverage_restated as V
import fold_restated as FR
import geneboot_restated as GR
import tieboot_restated as TR

pytestmark = pytest.mark.gpu

GOLD = I.GOLD
B, SEED, AGS = 64, 11, 3.0e6
CODON = dict(zip("ACDEFGHIKLMNPQRSTVWY", ("GCT", "TGT", "GAT", "GAA", "TTT", "GGT", "CAT", "ATT", "AAA", "CTG", "ATG", "AAT", "CCG", "CAG", "CGT", "AGC", "ACC", "GTG", "TGG", "TAT")))


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def kept(engine):
    """the example reads searched once with the rows kept and every switch on: the restatement's entries of those rows, and the device's two
    matrices of that search - computed once, shared, never changed"""
    reads = I.example_reads()
    nseq = len(engine.names)
    scale = np.random.default_rng(3).uniform(1e-4, 1e-3, B)
    scale[[5, 40]] = [np.nan, 0.0]
    engine.set_abundance(True)
    try:
        engine.set_ties(True)
        engine.set_gene_bootstrap(len(reads))
        engine.set_tie_bootstrap(4 * len(reads))
        rows, _ = engine.search(reads)
        rows = rows.copy()
        gb = engine.gene_bootstrap(B, SEED, scale, counts=True)
        tb = engine.tie_bootstrap(B, SEED, scale, shares=True)
        ti, ms = engine.ties(), engine.tie_bootstrap_kernels_ms()
    finally:
        engine.set_abundance(False)
    q, s, sh, ks = TR.entries(V.rows_from_array(rows), nseq)
    return {"q": q, "s": s, "share": sh, "k": ks, "nseq": nseq, "scale": scale, "gb": gb, "tb": tb, "ti": ti, "ms": ms}


def test_engine_equals_the_restatement_and_keeps_the_invariant(kept):
    a = kept
    want = TR.shares(a["q"], a["s"], a["share"], a["nseq"], B, SEED)
    print("reads that add", len(a["k"]), "entries", len(a["q"]), "ambiguous", a["ti"]["ambiguous"], "widest", max(a["k"]), "ms", a["ms"])
    assert a["ti"]["ambiguous"] == sum(1 for k in a["k"] if k > 1) > 0 and len(a["q"]) == int(a["ti"]["candidates"].sum()) > len(a["k"]) > 100
    assert a["tb"]["dropped"] == 0 and a["tb"]["used"] == B - 2 and a["ms"]["collect"] > 0.0 and a["ms"]["read"] > 0.0
    assert np.array_equal(a["tb"]["shares"], want)
    assert GR.same_bits(a["tb"]["stats"], TR.stats(want, a["scale"]))
    for b in range(B):                                             # sum_s cs[b][s] = 2^32 x sum_s c[b][s], from the two device matrices
        assert sum(int(v) for v in a["tb"]["shares"][:, b]) == TR.ONE * int(a["gb"]["counts"][:, b].sum()), b


def _strip(path):
    """the lines of a gene table with the switch's two header lines and its three columns taken away"""
    out = []
    for line in open(path).read().split("\n"):
        if line.startswith("# bootstrap_ties:") or line.startswith("# tie_list:"):
            continue
        out.append(line if line.startswith("#") or not line else line.rsplit("\t", 3)[0])
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from microbecensus_amd import _native, abundance
    d = tmp_path_factory.mktemp("tieboot_e2e")
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    (d / "map.tsv").write_text("".join("%s\t%s\n" % kv for kv in TC.group_map(_native.load_markers()[0]).items()))

    def run(out, **kw):
        return abundance.run_abundance(dict({"seqfiles": [fq], "genes": genes, "outfile": str(d / out), "nreads": 10000, "device": 0, "ags": AGS, "coverage": True, "ties": True,
                                             "groups": str(d / "map.tsv"), "depth_out": str(d / (out + ".depth")), "bootstrap": B, "bootstrap_seed": SEED}, **kw))
    on, args = run("on.tsv", bootstrap_ties=True)
    off, _ = run("off.tsv")
    return {"dir": d, "on": on, "off": off, "args": args}


def test_run_abundance_columns_equal_the_restatement(kept, runs):
    from microbecensus_amd import abundance
    a, t = kept, runs["on"]
    assert t["reads_ambiguous"] > 0 and t["sampled_reads"] == 8672 and runs["args"]["tie_bootstrap_ms"] > 0.0
    scale = np.full(B, 1.0 / t["genome_equivalents_sampled"])
    assert np.array_equal(t["boot_scale"], scale)                                  # the gene bootstrap's own scales
    want = TR.stats(TR.shares(a["q"], a["s"], a["share"], a["nseq"], B, SEED), scale)
    assert GR.same_bits(t["tie_boot_stats"], want) and t["tie_boot_used"] == B
    for name, col in zip(abundance.TIE_BOOT_COLUMNS, abundance.boot_columns(want, B, t["length_aa"])):
        assert GR.same_bits(t[name], col), name
    header, rows = abundance.read_table(str(runs["dir"] / "on.tsv"))
    assert header["bootstrap_ties"] == "on" and header["tie_list"] == "%d/%d" % (len(a["q"]), 4 * 10000)
    assert [r[-3:] for r in rows] == [[repr(float(x)) for x in v] for v in zip(*(t[c] for c in abundance.TIE_BOOT_COLUMNS))]
    cand = t["candidate_reads"] > 0
    assert (t["rpkg_shared_boot_se"][cand] > 0).all() and not t["rpkg_shared_boot_se"][~cand].any() and (t["rpkg_shared_ci95_low"] <= t["rpkg_shared_ci95_high"]).all()
    # a gene none of whose reads tie carries its rpkg interval, bit for bit
    alone = (t["candidate_reads"] == t["unique_reads"]) & cand
    tied = (t["candidate_reads"] > t["unique_reads"])
    assert alone.sum() > 10 and tied.sum() > 10 and np.array_equal(t["reads"][alone], t["unique_reads"][alone])
    for shared, plain in zip(abundance.TIE_BOOT_COLUMNS, abundance.BOOT_COLUMNS):
        assert GR.same_bits(t[shared][alone], t[plain][alone]), shared
    assert not GR.same_bits(t["rpkg_shared_boot_se"][tied], t["rpkg_boot_se"][tied])


def test_without_the_switch_every_file_is_what_it_was(runs):
    d = runs["dir"]
    assert _strip(str(d / "on.tsv")) == open(str(d / "off.tsv")).read().split("\n")
    for suffix in (".groups.tsv", ".depth"):
        assert open(str(d / ("on.tsv" + suffix))).read() == open(str(d / ("off.tsv" + suffix))).read(), suffix
    assert "rpkg_shared_boot_se" not in runs["off"] and "tie_bootstrap_ms" not in runs["off"]
    for key in ("reads", "rpkg", "share", "rpkg_shared", "rpkg_boot_se", "boot_stats"):
        assert GR.same_bits(np.asarray(runs["on"][key], np.float64), np.asarray(runs["off"][key], np.float64)), key


def test_a_list_too_small_is_refused_with_the_factor_that_fits(tmp_path):
    """The example reads cannot overflow a factor of 1: 8,672 sampled reads size the gene list, and the README's 251 assigned reads with 57 ties
    across at most 6 genes are at most 251 + 57 x 5 = 536 entries.  So: a synthetic FASTA of duplicated genes - 40 markers, each three times
    under three names - and reads cut from their back-translation: nearly every read ties across three genes, about three entries a read."""
    from microbecensus_amd import _native, abundance
    names, seqs = _native.load_markers()
    pick = [g for g in range(0, len(seqs), 97) if 150 <= len(seqs[g]) <= 400 and set(seqs[g]) <= set(CODON)][:40]
    with open(tmp_path / "genes.faa", "w") as f:
        for copy in "abc":
            for g in pick:
                f.write(">%s_%s\n%s\n" % (names[g], copy, seqs[g]))
    reads = []
    for g in pick:
        dna = "".join(CODON[c] for c in seqs[g])
        reads += [dna[i:i + 100].encode() for i in range(0, len(dna) - 100, 7)]
    fa = TC.write_fasta(tmp_path / "reads.fa", reads)

    def run(out, **kw):
        return abundance.run_abundance(dict({"seqfiles": [fa], "genes": str(tmp_path / "genes.faa"), "outfile": str(tmp_path / out), "nreads": None, "device": 0, "ags": AGS,
                                             "ties": True, "bootstrap": 8, "bootstrap_ties": True}, **kw))
    t, _ = run("fits.tsv")                                          # the default factor, 4, holds them; nreads None, no cap: the sampler's count sizes both lists (-n would)
    total, n = int(t["candidate_reads"].sum()), t["sampled_reads"]
    assert n == len(reads) and n < total <= 4 * n and t["reads_ambiguous"] > n // 2
    fits = -(-total // n)
    print("reads", n, "entries", total, "fits", fits)
    with pytest.raises(abundance.AbundanceError, match=r"--bootstrap-ties: %d tie entries did not fit the list of %d \(--tie-list-factor 1 x %d reads\): --tie-list-factor %d fits all %d" % (
            total - n, n, n, fits, total)):
        run("short.tsv", tie_list_factor=1)
    assert not os.path.exists(str(tmp_path / "short.tsv"))
    again, _ = run("exact.tsv", tie_list_factor=fits)
    assert GR.same_bits(again["tie_boot_stats"], t["tie_boot_stats"])


def test_mixed_lengths_under_a_given_ags(tmp_path):
    """30,000 reads of 40 - 320 bp in the classes 100 and 150 (test_gpu_abund_classes_e2e.py's file): the restatement on the rows of one
    fixed-length keep_rows search per class, every read's id its rank among the sampled reads (those that reach a class)"""
    from microbecensus_amd import _native, abundance
    reads, lens = TC.mixed_reads()
    classes = TC.CLASSES
    cls = cr.class_of(lens, classes)
    keep = np.flatnonzero(cls < len(classes))
    rank = np.full(len(reads), -1, np.int64)
    rank[keep] = np.arange(len(keep))
    t, args = abundance.run_abundance({"seqfiles": [TC.write_fasta(tmp_path / "mixed.fa", reads)], "genes": os.path.join(_native.DATA_DIR, "markers.faa.gz"), "outfile": str(tmp_path / "m.tsv"),
                                       "nreads": 40_000, "device": 0, "ags": AGS, "ties": True, "bootstrap": B, "bootstrap_seed": SEED, "bootstrap_ties": True, "mixed_lengths": list(classes)})
    mat = cr.make_rows(reads, classes[-1])
    q, s, sh = [], [], []
    e = _native.Engine(device=0)
    try:
        nseq = len(e.names)
        for k, L in enumerate(classes):
            idx = np.flatnonzero(cls == k)
            e.set_run(L)
            e.set_abundance(True)
            try:
                host, _ = e.search(mat[idx, :L])
                qk, sk, shk, _ = TR.entries(V.rows_from_array(host), nseq, ids=lambda pos, idx=idx: rank[idx[pos]])
            finally:
                e.set_abundance(False)
            q.append(qk); s.append(sk); sh.append(shk)
    finally:
        e.close()
    q, s, sh = np.concatenate(q), np.concatenate(s), np.concatenate(sh)
    assert t["sampled_reads"] == len(keep) and len(q) == int(t["candidate_reads"].sum()) > t["reads_assigned"] > 0 and q.min() >= 0
    scale = np.full(B, 1.0 / t["genome_equivalents_sampled"])
    want = TR.stats(TR.shares(q, s, sh, nseq, B, SEED), scale)
    assert GR.same_bits(t["tie_boot_stats"], want)
    for name, col in zip(abundance.TIE_BOOT_COLUMNS, abundance.boot_columns(want, B, t["length_aa"])):
        assert GR.same_bits(t[name], col), name


def test_long_genes_at_the_test_sized_segments():
    """test_gpu_fold.py's database and cut: every second marker, segments of 768 that overlap by V; the engine on the segments with the fold
    set.  k_tieboot_collect runs behind the fold, in gene space: the restatement on the host rows of the same search, folded in numpy."""
    from microbecensus_amd import _native, abundance
    names, seqs = TC.long_gene_markers()
    reads = I.example_reads()
    sp = abundance.split_genes(names, seqs, seg_len=768, overlap=FR.V)
    scale = np.full(B, 0.03125)
    eng = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"])
    try:
        eng.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
        eng.set_run(100)
        eng.set_abundance(True)
        eng.set_ties(True)
        eng.set_gene_bootstrap(len(reads))
        eng.set_tie_bootstrap(4 * len(reads))
        rows = eng.search(reads)[0].copy()
        tb, gb, ti = eng.tie_bootstrap(B, SEED, scale, shares=True), eng.gene_bootstrap(B, SEED, scale, counts=True), eng.ties()
    finally:
        eng.close()
    assert sp["genes_split"] >= 20 and len(tb["shares"]) == len(names)
    folded = FR.fold(rows, FR.records(sp["gene_len"], 768, FR.V)[0])
    q, s, sh, ks = TR.entries(V.rows_from_array(folded), len(names))
    want = TR.shares(q, s, sh, len(names), B, SEED)
    split = np.flatnonzero(sp["gene_len"] > 768)
    assert len(q) == int(ti["candidates"].sum()) > len(ks) > 0 and want[split].any()                # entries of genes that were cut
    assert np.array_equal(tb["shares"], want) and GR.same_bits(tb["stats"], TR.stats(want, scale))
    assert all(sum(int(v) for v in tb["shares"][:, b]) == TR.ONE * int(gb["counts"][:, b].sum()) for b in range(B))
