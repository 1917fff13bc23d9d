"""The bootstrap of the coverage columns end to end (csrc/mc_covboot.h states the rule, tests/covboot_restated.py restates it): the example
reads against the packaged markers, as test_gpu_geneboot.py and test_gpu_tieboot.py run them, with --min-breadth 0.5 --bootstrap 200
--bootstrap-coverage - the new columns equal the restatement applied to the rows of a keep_rows search of the same reads, integers exactly
and doubles bit for bit; the device's matrices keep the statement's invariants against the same run's covered_aa and gene bootstrap; the
figures do not depend on the batches; a seed gives its bits twice and another seed others; without the switch every file is what it was; and
the same under a gene fold at test_gpu_fold.py's (768, V), under --mixed-lengths with --ags, and through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import abund_inputs as I
import abundance_table_cases as TC
import classes_restated as cr
import covboot_restated as CR
import coverage_restated as V
import fold_restated as FR
import geneboot_restated as GR

pytestmark = pytest.mark.gpu

GOLD = I.GOLD
REPO = os.path.dirname(I.HERE)
B, SEED, AGS, F = 200, 11, 3.0e6, 0.5
F_LOW = 0.05                            # a breadth that single reads of 33 residues reach on genes of some hundred: the example reads detect nothing at 0.5
NEW = 5                                 # the columns the switch adds with min_breadth


@pytest.fixture(scope="module")
def engine():
    yield from I.marker_engine()


@pytest.fixture(scope="module")
def kept(engine):
    """the example reads searched once with the rows kept and the switches on: the restatement's entries of those rows, and the device's
    matrices of that search - computed once, shared, never changed"""
    from microbecensus_amd import _native, abundance
    reads = I.example_reads()
    lengths = np.array([len(s) for s in _native.load_markers()[1]], np.int64)
    need = abundance.coverage_need(lengths, F)
    engine.set_abundance(True)
    try:
        engine.set_coverage(True)
        engine.set_gene_bootstrap(len(reads))
        engine.set_coverage_bootstrap(len(reads))
        rows, _ = engine.search(reads)
        rows = rows.copy()
        gb = engine.gene_bootstrap(B, SEED, np.ones(B), counts=True)
        cb = engine.coverage_bootstrap(B, SEED, need, covered=True)
        again = engine.coverage_bootstrap(B, SEED, need, covered=True)
        other = engine.coverage_bootstrap(B, SEED + 1, need, covered=True)
        plain = engine.coverage_bootstrap(B, SEED)
        low = engine.coverage_bootstrap(B, SEED, abundance.coverage_need(lengths, F_LOW))
        cov, ab, ms = engine.coverage(), engine.abundance(), engine.coverage_bootstrap_kernels_ms()
        refusals = []
        for call in (lambda: engine.coverage_bootstrap(0, SEED), lambda: engine.coverage_bootstrap(4097, SEED), lambda: engine.coverage_bootstrap(B, SEED, np.r_[need[:7], 0, need[8:]]),
                     lambda: engine.set_coverage_bootstrap(-1), lambda: engine.set_coverage_bootstrap(2 ** 31)):
            with pytest.raises(RuntimeError) as e:
                call()
            refusals.append(str(e.value))
        engine.set_coverage(False)                                  # coverage off takes the switch with it
        with pytest.raises(RuntimeError) as e:
            engine.coverage_bootstrap(B, SEED)
        refusals.append(str(e.value))
        with pytest.raises(RuntimeError) as e:
            engine.set_coverage_bootstrap(100)
        refusals.append(str(e.value))
    finally:
        engine.set_abundance(False)
    with pytest.raises(RuntimeError) as e:
        engine.set_coverage_bootstrap(100)
    refusals.append(str(e.value))
    q, g, s, e_ = CR.entries(V.rows_from_array(rows), lengths)
    want = CR.cover(q, g, s, e_, lengths, B, SEED)
    return {"q": q, "g": g, "s": s, "e": e_, "lengths": lengths, "need": need, "want": want, "gb": gb, "cb": cb, "again": again, "other": other, "plain": plain, "low": low, "cov": cov, "ab": ab, "ms": ms,
            "refusals": refusals}


def test_engine_equals_the_restatement_and_keeps_the_invariants(kept):
    a = kept
    cb = a["cb"]
    print("assigned", len(a["q"]), "genes with reads", int((a["ab"]["reads"] > 0).sum()), "empty spans", int((a["s"] > a["e"]).sum()), "ms", a["ms"])
    assert len(a["q"]) == a["ab"]["assigned"] > 100 and cb["dropped"] == 0 and a["ms"]["collect"] > 0.0 and a["ms"]["read"] > 0.0
    assert np.array_equal(cb["covered"], a["want"]), "covered residues"
    assert GR.same_bits(cb["stats"], CR.stats(a["want"])), "the six doubles"
    assert np.array_equal(cb["detected"], CR.detected(a["want"], a["need"])), "detected"
    # the invariants, from the device's own figures of the same run: covered_aa of the scan, the gene bootstrap's counts under the same seed
    covered, counts, cov = a["cov"]["covered"], a["gb"]["counts"], cb["covered"]
    assert (cov <= covered[:, None]).all() and (cov.max(axis=1) > 0).sum() > 50
    assert (counts[cov > 0] > 0).all()
    valid = np.ones(len(covered), bool)
    valid[a["g"][a["s"] > a["e"]]] = False
    assert np.array_equal((cov > 0)[valid], (counts > 0)[valid])
    one = np.flatnonzero(a["ab"]["reads"] == 1)
    width = {int(gg): int(e) - int(s) + 1 for gg, s, e in zip(a["g"], a["s"], a["e"])}
    assert len(one) > 10 and all(set(cov[gg].tolist()) <= {0, width[int(gg)]} for gg in one)
    # the sample's own call against the replicates': a gene the sample does not detect has no support, under F and under a breadth that
    # single reads reach
    from microbecensus_amd import abundance
    for f, got in ((F, cb["detected"]), (F_LOW, a["low"]["detected"])):
        need = abundance.coverage_need(a["lengths"], f)
        det = (covered >= need) & (a["ab"]["reads"] > 0)
        assert np.array_equal(det.astype(np.int64), abundance.detect(a["ab"]["reads"], covered, a["lengths"], f))
        assert np.array_equal(got, CR.detected(a["want"], need)) and not got[~det].any() and (got <= B).all()
        print("F %g: %d genes detected, support counts %s" % (f, int(det.sum()), sorted(set(got[det].tolist()))[:12]))
    assert det.sum() > 20 and len(set(a["low"]["detected"][det].tolist())) > 3


def test_same_seed_same_bits_another_seed_other_replicates(kept):
    a = kept
    assert np.array_equal(a["again"]["covered"], a["cb"]["covered"]) and GR.same_bits(a["again"]["stats"], a["cb"]["stats"]) and np.array_equal(a["again"]["detected"], a["cb"]["detected"])
    assert not np.array_equal(a["other"]["covered"], a["cb"]["covered"]) and np.array_equal(a["other"]["covered"], CR.cover(a["q"], a["g"], a["s"], a["e"], a["lengths"], B, SEED + 1))
    assert GR.same_bits(a["plain"]["stats"], a["cb"]["stats"]) and "detected" not in a["plain"] and "covered" not in a["plain"]


def test_refusals_name_the_value(kept):
    r = kept["refusals"]
    assert "mc_coverage_bootstrap: B 0 is not a number of replicates from 1 to 4096" in r[0] and "B 4097" in r[1]
    assert "mc_coverage_bootstrap: need[7] = 0" in r[2]
    assert "mc_set_coverage_bootstrap: capacity -1 is not a number of entries from 0 to 2^31 - 1" in r[3] and "capacity 2147483648" in r[4]
    assert "mc_coverage_bootstrap: the coverage bootstrap is off" in r[5]
    assert "mc_set_coverage_bootstrap: coverage is off (mc_set_coverage)" in r[6] and "capacity = 100" in r[6]
    assert "mc_set_coverage_bootstrap: the counts are off (mc_set_abundance)" in r[7]


def _strip(path, new):
    """the lines of a gene table with the switch's header line and its columns taken away"""
    out = []
    for line in open(path).read().split("\n"):
        if line.startswith("# bootstrap_coverage:"):
            continue
        out.append(line if line.startswith("#") or not line else line.rsplit("\t", new)[0])
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from microbecensus_amd import _native, abundance
    d = tmp_path_factory.mktemp("covboot_e2e")
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    (d / "map.tsv").write_text("".join("%s\t%s\n" % kv for kv in TC.group_map(_native.load_markers()[0]).items()))

    def run(out, **kw):
        return abundance.run_abundance(dict({"seqfiles": [fq], "genes": genes, "outfile": str(d / out), "nreads": 10000, "device": 0, "ags": AGS, "min_breadth": F, "ties": True,
                                             "groups": str(d / "map.tsv"), "depth_out": str(d / (out + ".depth")), "bootstrap": B, "bootstrap_seed": SEED, "bootstrap_ties": True}, **kw))
    on, args = run("on.tsv", bootstrap_coverage=True)
    off, _ = run("off.tsv", bootstrap_coverage=False)
    never, _ = run("never.tsv")                                     # (a request that never heard of the switch)
    os.environ["MC_STREAM_BATCH"] = "3000"
    try:
        batches, _ = run("batches.tsv", bootstrap_coverage=True)
    finally:
        del os.environ["MC_STREAM_BATCH"]
    return {"dir": d, "on": on, "off": off, "never": never, "batches": batches, "args": args}


def test_run_abundance_columns_equal_the_restatement(kept, runs):
    from microbecensus_amd import abundance
    a, t = kept, runs["on"]
    assert t["sampled_reads"] == 8672 and runs["args"]["coverage_bootstrap_ms"] > 0.0 and t["reads_assigned"] == len(a["q"])
    want = CR.stats(a["want"])
    assert GR.same_bits(t["cov_boot_stats"], want) and np.array_equal(t["cov_boot_detected"], CR.detected(a["want"], a["need"]))
    cols = abundance.cov_boot_columns(want, B, t["length_aa"])
    for name, col in zip(abundance.COV_BOOT_COLUMNS, cols):
        assert GR.same_bits(t[name], col), name
    # the columns are what numpy makes of the replicate breadths themselves
    breadth_b = a["want"].astype(np.float64) / t["length_aa"][:, None]
    have = np.flatnonzero(t["reads"] > 0)
    assert np.allclose(t["breadth_boot_mean"][have], breadth_b[have].mean(axis=1), rtol=1e-12, atol=0) and np.allclose(t["breadth_boot_se"][have], breadth_b[have].std(axis=1, ddof=1), rtol=1e-9, atol=1e-15)
    lo, hi = np.percentile(breadth_b[have], [2.5, 97.5], axis=1)
    assert np.allclose(t["breadth_ci95_low"][have], lo, rtol=1e-12, atol=0) and np.allclose(t["breadth_ci95_high"][have], hi, rtol=1e-12, atol=0)
    assert (t["breadth_ci95_high"] <= t["breadth"]).all() and (t["breadth_ci95_low"] <= t["breadth_boot_mean"]).all() and (t["breadth_boot_mean"] <= t["breadth_ci95_high"]).all()
    assert np.array_equal(t["detected_support"], t["cov_boot_detected"] / float(B)) and not t["detected_support"][t["detected"] == 0].any()
    header, rows = abundance.read_table(str(runs["dir"] / "on.tsv"))
    assert header["bootstrap_coverage"] == "on" and header["min_breadth"] == "0.5"
    assert [r[-NEW:] for r in rows] == [[repr(float(x)) for x in v] for v in zip(*(t[c] for c in abundance.COV_BOOT_COLUMNS + ("detected_support",)))]
    print("detected %d genes; their support %s" % (int(t["detected"].sum()), t["detected_support"][t["detected"] == 1].tolist()[:10]))


def test_the_figures_do_not_depend_on_the_batches(runs):
    for key in ("cov_boot_stats", "cov_boot_detected", "breadth_boot_se", "detected_support", "covered_aa", "reads"):
        assert GR.same_bits(np.asarray(runs["batches"][key], np.float64), np.asarray(runs["on"][key], np.float64)), key
    d = runs["dir"]
    assert open(str(d / "batches.tsv")).read().split("\n")[1:] == open(str(d / "on.tsv")).read().split("\n")[1:]


def test_without_the_switch_every_file_is_what_it_was(runs):
    d = runs["dir"]
    assert _strip(str(d / "on.tsv"), NEW) == open(str(d / "off.tsv")).read().split("\n")
    for suffix in ("", ".groups.tsv", ".depth"):
        assert open(str(d / ("off.tsv" + suffix))).read() == open(str(d / ("never.tsv" + suffix))).read(), suffix
        if suffix:
            assert open(str(d / ("on.tsv" + suffix))).read() == open(str(d / ("off.tsv" + suffix))).read(), suffix
    assert "breadth_boot_se" not in runs["off"] and "coverage_bootstrap_ms" not in runs["off"] and "cov_boot_stats" not in runs["never"]
    for key in ("reads", "rpkg", "covered_aa", "breadth", "detected", "rpkg_boot_se", "boot_stats", "tie_boot_stats", "rpkg_shared_boot_se"):
        assert GR.same_bits(np.asarray(runs["on"][key], np.float64), np.asarray(runs["off"][key], np.float64)), key


def test_the_command_line_writes_the_header_line_and_the_columns(tmp_path):
    from microbecensus_amd import _native, abundance
    out = str(tmp_path / "cli.tsv")
    cmd = [sys.executable, os.path.join(REPO, "scripts", "gene_abundance.py"), os.path.join(GOLD, "inputs", "example.fq.gz"), os.path.join(_native.DATA_DIR, "markers.faa.gz"), out,
           "-n", "10000", "--ags", "3.0e6", "--min-breadth", str(F_LOW), "--bootstrap", "20", "--bootstrap-coverage"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    header, rows = abundance.read_table(out)
    cols = open(out).read().split("\n")[len(header)].split("\t")
    assert header["bootstrap_coverage"] == "on" and header["bootstrap"] == "20" and cols[-NEW:] == list(abundance.COV_BOOT_COLUMNS) + ["detected_support"] and cols[-NEW - 1] == "rpkg_ci95_high"
    sup = np.array([float(r[-1]) for r in rows])
    assert len(rows) == len(_native.load_markers()[0]) and ((sup >= 0) & (sup <= 1)).all() and (sup > 0).any() and np.allclose(sup * 20, np.round(sup * 20))
    p = subprocess.run(cmd[:-1] + ["--bootstrap-coverage", "--curve", "4"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode != 0 and "--bootstrap" in p.stdout


def test_long_genes_at_the_test_sized_segments():
    """test_gpu_fold.py's database and cut: every second marker, segments of 768 that overlap by V; the engine on the segments with the fold
    set.  k_covboot_collect runs behind the fold, in gene space: the figures are the restatement's on the host rows of the same search, folded
    in numpy - and those of the unsplit search, for every gene whose reads have the same best rows in both (which gene of a tied set a read
    goes to depends on the row order among tied genes, test_gpu_fold.py; those reads are printed and held to 1 % of the assigned)."""
    from microbecensus_amd import _native, abundance
    names, seqs = TC.long_gene_markers()
    reads = I.example_reads()
    lengths = np.array([len(s) for s in seqs], np.int64)
    need = abundance.coverage_need(lengths, F)
    sp = abundance.split_genes(names, seqs, seg_len=768, overlap=FR.V)

    def run(eng, fold):
        try:
            if fold:
                eng.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
            eng.set_run(100)
            eng.set_abundance(True)
            eng.set_coverage(True)
            eng.set_coverage_bootstrap(len(reads))
            rows = eng.search(reads)[0].copy()
            return rows, eng.coverage_bootstrap(64, SEED, need, covered=True), eng.coverage()
        finally:
            eng.close()
    urows, un, _ = run(_native.Engine(device=0, names=names, seqs=seqs, marker_family=[0] * len(names), nfam=1), False)
    srows, cb, cov = run(_native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"]), True)
    assert sp["genes_split"] >= 20 and len(cb["covered"]) == len(names) and np.array_equal(sp["gene_len"], lengths)
    folded = FR.fold(srows, FR.records(sp["gene_len"], 768, FR.V)[0])
    q, g, s, e = CR.entries(V.rows_from_array(folded), lengths)
    want = CR.cover(q, g, s, e, lengths, 64, SEED)
    split = np.flatnonzero(lengths > 768)
    assert want[split].any() and (e[np.isin(g, split)] >= 768).any()                              # spans that reach beyond a gene's first segment
    assert np.array_equal(cb["covered"], want) and GR.same_bits(cb["stats"], CR.stats(want)) and np.array_equal(cb["detected"], CR.detected(want, need))
    assert (cb["covered"] <= cov["covered"][:, None]).all()
    uq, ug, us, ue = CR.entries(V.rows_from_array(urows), lengths)
    mine, theirs = set(zip(q.tolist(), g.tolist(), s.tolist(), e.tolist())), set(zip(uq.tolist(), ug.tolist(), us.tolist(), ue.tolist()))
    moved = mine ^ theirs
    same = np.ones(len(names), bool)
    same[[x[1] for x in moved]] = False
    print("entries %d / %d, %d differ between split and unsplit, in %d genes" % (len(mine), len(theirs), len(moved), int((~same).sum())))
    assert len({x[0] for x in moved}) <= 0.01 * len(uq) and same[split].sum() > 10
    assert np.array_equal(cb["covered"][same], un["covered"][same]) and GR.same_bits(cb["stats"][same], un["stats"][same]) and np.array_equal(cb["detected"][same], un["detected"][same])


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
    Bm = 64
    t, args = abundance.run_abundance({"seqfiles": [TC.write_fasta(tmp_path / "mixed.fa", reads)], "genes": os.path.join(_native.DATA_DIR, "markers.faa.gz"), "outfile": str(tmp_path / "m.tsv"),
                                       "nreads": 40_000, "device": 0, "ags": AGS, "min_breadth": F, "bootstrap": Bm, "bootstrap_seed": SEED, "bootstrap_coverage": True, "mixed_lengths": list(classes)})
    mat = cr.make_rows(reads, classes[-1])
    lengths = t["length_aa"]
    q, g, s, e = [], [], [], []
    eng = _native.Engine(device=0)
    try:
        for k, L in enumerate(classes):
            idx = np.flatnonzero(cls == k)
            eng.set_run(L)
            eng.set_abundance(True)
            try:
                host, _ = eng.search(mat[idx, :L])
                part = CR.entries(V.rows_from_array(host), lengths, ids=lambda pos, idx=idx: rank[idx[pos]])
            finally:
                eng.set_abundance(False)
            for acc, col in zip((q, g, s, e), part):
                acc.append(col)
    finally:
        eng.close()
    q, g, s, e = (np.concatenate(x) for x in (q, g, s, e))
    assert t["sampled_reads"] == len(keep) and len(q) == t["reads_assigned"] > 0 and q.min() >= 0 and len(set(q.tolist())) == len(q)
    want = CR.cover(q, g, s, e, lengths, Bm, SEED)
    assert GR.same_bits(t["cov_boot_stats"], CR.stats(want)) and np.array_equal(t["cov_boot_detected"], CR.detected(want, abundance.coverage_need(lengths, F)))
    for name, col in zip(abundance.COV_BOOT_COLUMNS, abundance.cov_boot_columns(CR.stats(want), Bm, lengths)):
        assert GR.same_bits(t[name], col), name
