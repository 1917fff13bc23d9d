"""The identity of the assigned reads on the device (mc_set_identity; csrc/mc_identity.h states the rule) against tests/identity_restated.py
applied to the REFERENCE BINARY's m8 golden under cut-offs: the histogram, the three sums and the figures; independence from batches,
ranges and reads without rows in between; the invariants; run_abundance with the three switches and groups end to end, and the same run
without them byte for byte; long genes and mixed lengths against the restatement on rows kept from the same engine; the refusals of the
ABI.  The counts of the same runs are held to tests/abundance_restated.py throughout."""
import os

import numpy as np
import pytest

import abund_inputs as AI
import abundance_restated as R
import abundance_table_cases as TC
import classes_restated as cr
import fold_restated as FR
import identity_restated as I

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASE = "config1_example_fq"
CUTS = [dict(), dict(min_ident=60, min_aln=30)]                    # test_gpu_coverage.py's two
LEVELS = [0, 50, 66, 90, 100]
SUMS = ("matched", "mismatched", "gap_opens")
BINS = ("ident_min", "ident_median", "ident_max")


def _same(got, hist, want):
    return np.array_equal(hist, want["hist"]) and all(np.array_equal(got[k], want[k]) for k in SUMS + BINS) and np.array_equal(got["ge"], want["ge"])


def _same_counts(got, want):
    return np.array_equal(got["reads"], want["reads"]) and np.array_equal(got["aligned"], want["aligned"]) and got["assigned"] == want["assigned"]


@pytest.fixture(scope="module")
def engine():
    yield from AI.marker_engine()


@pytest.fixture(scope="module")
def reads():
    return AI.example_reads()


@pytest.fixture(scope="module")
def golden():
    """the reference binary's m8 of the case restated under both cut-off sets - computed once, shared, never changed"""
    from microbecensus_amd import _native
    names, seqs = _native.load_markers()
    rows = I.rows_from_m8(os.path.join(GOLD, CASE + ".m8.gz"), names)
    return {"names": names, "lengths": [len(s) for s in seqs], "idn": [I.identity(rows, len(names), LEVELS, **c) for c in CUTS],
            "ab": [R.abundance([r[:6] for r in rows], len(names), **c) for c in CUTS]}


@pytest.mark.parametrize("k", [0, 1], ids=["none", "ident60_aln30"])
def test_marker_database_equals_the_restatement_of_the_reference_m8(engine, reads, golden, k):
    want, want_ab = golden["idn"][k], golden["ab"][k]
    engine.set_abundance(True, **CUTS[k])
    try:
        engine.set_identity(True)
        engine.search(reads)
        got, hist, ab = engine.identity(LEVELS), engine.identity_hist(), engine.abundance()
        none = engine.identity()
        ms, scan_ms = engine.identity_ms(), engine.identity_scan_ms()
    finally:
        engine.set_abundance(False)
    print(CUTS[k], "assigned", ab["assigned"], "bins in use", int((hist.sum(axis=0) > 0).sum()), "matched", int(got["matched"].sum()), "k_identity ms", ms, "scan ms", scan_ms)
    assert hist.dtype == np.uint32 and hist.shape == (len(golden["names"]), 101) and ms > 0.0 and scan_ms > 0.0
    assert ab["searched"] == len(reads) and _same_counts(ab, want_ab)
    assert _same(got, hist, want)
    assert none["ge"].shape == (len(golden["names"]), 0) and all(np.array_equal(none[key], got[key]) for key in SUMS + BINS), "a read without levels"
    assert I.invariants(dict(got, hist=hist), ab["reads"], ab["aligned"], LEVELS) == []
    assert int(hist.sum()) == (251, 23)[k] and int((hist.sum(axis=1) > 0).sum()) == (239, 22)[k]


def test_identity_does_not_depend_on_batches_ranges_or_reads_in_between(engine, reads, golden, monkeypatch):
    want, want_ab, n = golden["idn"][0], golden["ab"][0], len(reads)
    got = {}

    def take(how):
        got[how] = (engine.identity(LEVELS), engine.identity_hist(), engine.abundance())

    def zeros():
        i, h, a = engine.identity(LEVELS), engine.identity_hist(), engine.abundance()
        return not h.any() and not any(i[key].any() for key in SUMS) and all((i[key] == -1).all() for key in BINS) and not i["ge"].any() and a["searched"] == 0 and not a["reads"].any()
    engine.set_abundance(True)
    try:
        engine.set_identity(True)
        assert zeros()
        engine.search(reads)
        take("one search")
        engine.abundance_reset()                                           # ... zeroes the identity too, and its times
        assert zeros() and engine.identity_ms() == 0.0
        between = None
        for lo, hi in ((0, 1000), (1000, 1003), (1003, n)):                # three calls of uneven sizes, no reset in between
            engine.search(reads[lo:hi], first_read_id=lo)
            if hi == 1003:
                between = engine.identity_hist()                           # a read between two of them changes nothing
        take("three searches, a read in between")
        assert 0 < int(between.sum()) < int(want["hist"].sum())
        engine.set_identity(False)                                         # off and on again: zeros, of the counts too
        with pytest.raises(RuntimeError, match="the identity is off"):
            engine.identity()
        assert engine.abundance()["searched"] == n                         # (off leaves the counts alone)
        engine.set_identity(True)
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
        engine.set_coverage(True)                                          # another switch going on zeroes these tables too
        assert zeros()
        engine.set_ties(True)
        engine.search(reads)
        take("beside coverage and ties")
        engine.set_abundance(True)                                         # the counts set again: the identity starts again with them
        assert zeros()
    finally:
        engine.set_abundance(False)
    assert len(got) == 5
    for how, (i, h, a) in got.items():
        assert a["searched"] == n and _same_counts(a, want_ab) and _same(i, h, want), how


def test_refusals_through_the_abi(engine, reads):
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    nseq = len(engine.names)
    buf, hist = np.zeros(nseq, np.int64), np.zeros((nseq, 101), np.uint32)
    lv = np.int32([50, 90])
    assert lib.mc_set_identity(h, 1) != 0 and "abundance counting is off" in err()
    assert lib.mc_identity_read(h, None, 0, buf.ctypes.data, None, None, None, None, None, None) != 0 and "the identity is off" in err()
    assert lib.mc_identity_hist(h, hist.ctypes.data) != 0 and "the identity is off" in err()
    assert lib.mc_identity_ms(h) == 0.0 and lib.mc_set_identity(h, 0) == 0       # off while off: nothing to do
    engine.set_abundance(True)
    try:
        assert lib.mc_identity_read(h, None, 0, buf.ctypes.data, None, None, None, None, None, None) != 0 and "the identity is off" in err()
        engine.upload(reads[:2000])
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_identity(h, 1) != 0 and "in flight" in err()
        engine.range_end()
        engine.set_identity(True)
        engine.range_begin(0, 2000, 0)
        assert lib.mc_set_identity(h, 0) != 0 and "in flight" in err()
        engine.range_end()
        assert engine.abundance()["searched"] == 2000                        # (set_identity(True) zeroed the first range's counts)
        for levels, text in (([-1], "level 0 is -1: not a percent from 0 to 100"), ([50, 101], "level 1 is 101: not a percent"), ([50, 50], "level 1 is 50: not above the level before it, 50"),
                             ([90, 50], "level 1 is 50: not above the level before it, 90"), (list(range(9)), "nlevels 9 is not a number of levels from 0 to 8")):
            with pytest.raises(RuntimeError, match=text):
                engine.identity(levels)
        assert lib.mc_identity_read(h, None, -1, None, None, None, None, None, None, None) != 0 and "nlevels -1" in err()
        assert lib.mc_identity_read(h, None, 2, None, None, None, None, None, None, None) != 0 and "2 levels and a NULL array" in err()
        assert lib.mc_identity_hist(h, None) != 0 and "NULL array" in err()
        # every refusal has left the handle usable: only matched asked for; levels without ge; everything asked for
        assert lib.mc_identity_read(h, None, 0, buf.ctypes.data, None, None, None, None, None, None) == 0
        assert lib.mc_identity_read(h, lv.ctypes.data, 2, None, None, None, None, None, None, None) == 0
        idn = engine.identity([50, 90])
        assert np.array_equal(buf, idn["matched"]) and int(buf.sum()) > 0 and int(idn["ge"][:, 0].sum()) >= int(idn["ge"][:, 1].sum()) > 0
        engine.set_abundance(False)                                          # ... turns the identity off with it
        assert lib.mc_identity_hist(h, hist.ctypes.data) != 0 and "the identity is off" in err()
        assert lib.mc_set_identity(h, 1) != 0 and "abundance counting is off" in err()
    finally:
        engine.set_abundance(False)
    rows_ok, _ = engine.search(reads[:2000])                                 # the handle is what it was
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


def test_run_abundance_with_the_switches_end_to_end(golden, tmp_path):
    """run_abundance with the packaged markers as the genes, on the example FASTQ under config1's sample options (-n 10000; 100 bp), under
    --ags, with groups: the files parse back to the restatement's figures, and the run without the switches writes the same bytes less the
    new columns and header lines."""
    from microbecensus_amd import _native, abundance
    names, lengths = golden["names"], golden["lengths"]
    levels = [50, 90]
    want = dict(golden["idn"][0], ge=golden["idn"][0]["ge"][:, [LEVELS.index(t) for t in levels]])
    want_ab = golden["ab"][0]
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    genes = os.path.join(_native.DATA_DIR, "markers.faa.gz")
    (tmp_path / "map.tsv").write_text("".join("%s\t%s\n" % (n, n.split("_")[0]) for n in names[:4000]))
    group_of = TC.group_map(names)
    base = {"seqfiles": [fq], "genes": genes, "nreads": 10000, "device": 0, "ags": 3.0e6, "groups": str(tmp_path / "map.tsv")}
    off, on, hist_file = str(tmp_path / "off.tsv"), str(tmp_path / "on.tsv"), str(tmp_path / "ident.tsv")
    plain, _ = abundance.run_abundance(dict(base, outfile=off))
    assert "identity" not in plain and "matched_aa" not in plain and "groups_ident" not in plain
    table, args = abundance.run_abundance(dict(base, outfile=on, ident_levels=levels, ident_out=hist_file))
    assert args["identity"] is True and args["identity_ms"] > 0.0
    # the device's figures are the restatement's, and the counts abundance_restated's
    idn = table["identity"]
    assert _same(idn, idn["hist"], want) and np.array_equal(table["reads"], want_ab["reads"]) and np.array_equal(table["aligned_aa"], want_ab["aligned"])
    # without the switches: byte for byte
    assert open(off).read() == _strip(on, ("identity", "ident_levels"), 5)
    assert open(off + ".groups.tsv").read() == _strip(on + ".groups.tsv", ("identity", "ident_levels"), 4)
    # the gene table parses back
    header, body = abundance.read_table(on)
    cols = open(on).read().split("\n")[len(header)].split("\t")
    assert header["identity"] == "on" and header["ident_levels"] == "50,90"
    assert cols[5:] == list(abundance.IDENT_COLUMNS) + ["reads_ident_ge50", "rpkg_ident_ge50", "reads_ident_ge90", "rpkg_ident_ge90"] and len(body) == len(names)
    has = want_ab["reads"] > 0
    for c, key in ((5, "matched"), (6, "mismatched"), (7, "gap_opens")):
        assert [int(r[c]) for r in body] == want[key].tolist(), key
    assert [r[8] for r in body] == [repr(100.0 * m / a) if h else "NA" for m, a, h in zip(want["matched"].tolist(), want_ab["aligned"].tolist(), has.tolist())]
    for c, key in ((9, "ident_median"), (10, "ident_min"), (11, "ident_max")):
        assert [r[c] for r in body] == ["NA" if v < 0 else "%d" % v for v in want[key].tolist()], key
    ge = table["genome_equivalents_sampled"]
    for j in range(2):
        assert [int(r[12 + 2 * j]) for r in body] == want["ge"][:, j].tolist()
        assert [r[13 + 2 * j] for r in body] == [repr(float(v)) for v in abundance.rpkg(want["ge"][:, j], lengths, ge)]
    assert sum(1 for r in body if r[8] == "NA") == int((~has).sum()) > 0 and 0 < int(want["ge"][:, 1].sum()) < int(want["ge"][:, 0].sum()) < 251
    # the groups table: sums over the members
    gh, gbody = abundance.read_table(on + ".groups.tsv")
    gcols = open(on + ".groups.tsv").read().split("\n")[len(gh)].split("\t")
    assert gcols[4:] == ["matched_aa", "ident_mean", "reads_ident_ge50", "rpkg_ident_ge50", "reads_ident_ge90", "rpkg_ident_ge90"] and gh["identity"] == "on"
    acc = {}
    for nm, m, a, g0, g1 in zip(names, want["matched"].tolist(), want_ab["aligned"].tolist(), want["ge"][:, 0].tolist(), want["ge"][:, 1].tolist()):
        t = acc.setdefault(group_of.get(nm, nm), [0, 0, 0, 0])
        t[0] += m; t[1] += a; t[2] += g0; t[3] += g1
    assert [r[0] for r in gbody] == list(acc)
    assert [(int(r[4]), r[5], int(r[6]), int(r[8])) for r in gbody] == [(t[0], repr(100.0 * t[0] / t[1]) if t[1] else "NA", t[2], t[3]) for t in acc.values()]
    assert sum(int(r[6]) for r in gbody) == int(want["ge"][:, 0].sum())
    # the histogram file re-expands to the device's histogram
    back = abundance.read_ident(hist_file, names)
    assert np.array_equal(back, want["hist"])
    listed = [l.split("\t")[0] for l in open(hist_file) if not l.startswith("#")]
    assert list(dict.fromkeys(listed)) == [n for n, h in zip(names, has.tolist()) if h] and len(listed) == int((want["hist"] > 0).sum())


def test_long_genes_in_gene_space():
    """test_gpu_fold.py's database (every second marker, cut at 768 with the fold's overlap): the identity of the split run is the restatement's on
    its own host rows folded in numpy - the tables are the genes', a segment's read lands on its gene."""
    from microbecensus_amd import _native, abundance
    names, seqs = TC.long_gene_markers()
    reads = AI.example_reads()
    sp = abundance.split_genes(names, seqs, seg_len=768, overlap=FR.V)
    eng = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"])
    try:
        eng.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
        eng.set_run(100)
        eng.set_abundance(True)
        eng.set_identity(True)
        rows = eng.search(reads)[0].copy()
        got, hist, ab = eng.identity(LEVELS), eng.identity_hist(), eng.abundance()
    finally:
        eng.close()
    folded = FR.fold(rows, FR.records(sp["gene_len"], 768, FR.V)[0])
    want = I.identity(I.rows_from_array(folded), len(names), LEVELS)
    want_ab = R.abundance(R.rows_from_array(folded), len(names))
    split_hit = [g for g in np.flatnonzero(ab["reads"]) if (sp["seg_gene"] == g).sum() > 1]
    print("long genes: %d genes, %d split, %d segments, assigned %d, genes with reads %d of which split %d" % (len(names), sp["genes_split"], len(sp["seg_names"]), ab["assigned"], int((ab["reads"] > 0).sum()), len(split_hit)))
    assert hist.shape == (len(names), 101) and len(split_hit) > 0 and ab["assigned"] > 100
    assert _same_counts(ab, want_ab) and _same(got, hist, want)
    assert I.invariants(dict(got, hist=hist), ab["reads"], ab["aligned"], LEVELS) == []


def test_mixed_lengths_ride_on_every_piece(tmp_path):
    """run_abundance --mixed-lengths 100,150 --ags on 30,000 reads of 40 - 320 bp (test_gpu_abund_classes_e2e.py's file): the histogram and the sums
    are the sums over the classes of the restatement on the host rows of a fixed-length search of that class's reads on an engine of the same
    database, the figures those of the summed histogram."""
    from microbecensus_amd import _native, abundance
    seqs, lens = TC.mixed_reads()
    classes = TC.CLASSES
    path = TC.write_fasta(tmp_path / "mixed.fa", seqs)
    levels = [50, 90]
    table, args = abundance.run_abundance({"seqfiles": [path], "genes": os.path.join(_native.DATA_DIR, "markers.faa.gz"), "outfile": str(tmp_path / "mixed.tsv"), "nreads": 10 ** 9, "device": 0,
                                           "mixed_lengths": list(classes), "ags": 3.0e6, "ident_levels": levels, "ident_out": str(tmp_path / "ident.tsv")})
    padded = cr.make_rows(seqs, classes[-1])
    cls = cr.class_of(np.minimum(lens, classes[-1]), classes)
    eng = _native.Engine(device=0)
    nseq = len(eng.names)
    hist, sums, reads = np.zeros((nseq, 101), np.int64), {k: np.zeros(nseq, np.int64) for k in SUMS}, np.zeros(nseq, np.int64)
    try:
        for k, L in enumerate(classes):
            eng.set_run(L)
            host, _ = eng.search(padded[cls == k, :L])
            one = I.identity(I.rows_from_array(host), nseq)
            hist += one["hist"]
            reads += R.abundance(R.rows_from_array(host), nseq)["reads"]
            for key in SUMS:
                sums[key] += one[key]
    finally:
        eng.close()
    idn = table["identity"]
    print("mixed lengths: class reads %s, assigned %s, bins in use %d" % (table["class_reads"], table["class_reads_assigned"], int((hist.sum(axis=0) > 0).sum())))
    assert min(table["class_reads_assigned"]) > 0 and np.array_equal(table["reads"], reads) and args["identity_ms"] > 0.0
    assert np.array_equal(idn["hist"], hist) and all(np.array_equal(idn[key], sums[key]) for key in SUMS)
    figs = [I.figures_of_hist(h, levels) for h in hist]
    assert [tuple(int(idn[key][g]) for key in BINS) + (idn["ge"][g].tolist(),) for g in range(nseq)] == [f[:3] + (f[3],) for f in figs]
    assert I.invariants(idn, table["reads"], table["aligned_aa"], levels) == []
    assert np.array_equal(abundance.read_ident(str(tmp_path / "ident.tsv"), table["gene"]), hist)
