"""Length classes on the GPU (mc_set_run_classes, mc_search_classes, mc_search_files on a class reader, run_pipeline's
mixed_lengths): every class of a mixed run against the single-length run of that class's reads, the pipeline against its per-class
runs, the refusals, and the device prologue against its numpy restatement.  All calls go through the C ABI."""
import os

import numpy as np
import pytest

from microbecensus_amd import _native, microbe_census as mc, synth

import classes_restated as cr

pytestmark = pytest.mark.gpu
MODEL = _native.load_model()
FAMS = MODEL["families"]
VALID = [int(x) for x in mc._valid_read_lengths()]
CLASSES = [L for L in VALID if L <= 300]                # 16 classes: 50 .. 300


@pytest.fixture(scope="module")
def engine():
    e = _native.Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed():
    """30,000 reads of marker-bearing genomes, each cut to a seeded length in 40 .. 320: (list of bytes, lengths)"""
    _, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=1_500_000, seed=31, marker_gene_fraction=0.3)
    full = synth.sample_reads(genome, 30_000, 320, seed=32)
    lens = np.random.default_rng(33).integers(40, 321, size=len(full))
    return [bytes(full[i, :lens[i]]) for i in range(len(full))], lens


def _set_classes(engine, classes):
    engine.set_run_classes(classes, {L: MODEL["pars"][str(L)] for L in classes}, FAMS)


def _same(a, b):
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in ("read", "family", "aln", "target_len", "bits"))


@pytest.mark.parametrize("best_only", [False, True], ids=["rows", "best-only"])
def test_every_class_equals_its_single_length_run(engine, mixed, best_only, monkeypatch):
    seqs, lens = mixed
    rows = cr.make_rows(seqs, CLASSES[-1])
    want_cls = cr.class_of(np.minimum(lens, CLASSES[-1]), CLASSES)
    _set_classes(engine, CLASSES)
    engine.set_best_hits_only(best_only)
    try:
        best, cls, class_reads = engine.search_classes(rows, first_read_id=7)
        assert len(engine.rows()) == 0                                           # a class run hands out no rows
        assert engine.stats()["reads"] == len(rows)
        monkeypatch.setenv("MC_STREAM_BATCH", "7000")                            # batches and ranges that split every class
        best_small, cls_small, reads_small = engine.search_classes(rows, first_read_id=7)
        monkeypatch.delenv("MC_STREAM_BATCH")
        assert _same(best, best_small) and (cls == cls_small).all() and (class_reads == reads_small).all()
        assert (class_reads == np.bincount(want_cls, minlength=len(CLASSES) + 1)).all() and class_reads[-1] > 0
        assert (np.diff(best["read"]) > 0).all()
        assert (cls == want_cls[best["read"] - 7]).all()
        with_hits = 0
        for k, L in enumerate(CLASSES):
            idx = np.flatnonzero(want_cls == k)
            got = best[cls == k].copy()
            got["read"] = np.searchsorted(idx, got["read"] - 7)                  # renumbered by rank inside the class
            engine.set_run(L, MODEL["pars"][str(L)], FAMS)
            engine.set_best_hits_only(best_only)
            _, want = engine.search(rows[idx, :L])
            assert _same(got, want), "class %d (%d bp)" % (k, L)
            with_hits += len(want) > 0
            _set_classes(engine, CLASSES)
            engine.set_best_hits_only(best_only)
        assert with_hits >= 5
    finally:
        engine.set_best_hits_only(False)


def test_one_class_is_mc_search_byte_for_byte(engine, mixed):
    seqs, lens = mixed
    L = 150
    cut = np.stack([np.frombuffer(s[:L], np.uint8) for s, n in zip(seqs, lens) if L <= n < 175][:4000])
    engine.set_run(L, MODEL["pars"][str(L)], FAMS)
    _, want = engine.search(cut, first_read_id=100)
    rows = np.zeros((len(cut), 175), np.uint8)
    rows[:, :L] = cut
    _set_classes(engine, [100, 150, 175])
    best, cls, class_reads = engine.search_classes(rows, first_read_id=100)
    assert len(want) > 0 and best.tobytes() == want.tobytes()
    assert (cls == 1).all() and class_reads.tolist() == [0, len(cut), 0, 0]
    # a later mc_set_run restores the single-length run
    engine.set_run(L, MODEL["pars"][str(L)], FAMS)
    _, again = engine.search(cut, first_read_id=100)
    assert again.tobytes() == want.tobytes()
    with pytest.raises(RuntimeError, match="mc_set_run_classes"):
        engine.search_classes(rows)


def test_refusals(engine):
    for cl, word in (([], "0 length classes"), (list(range(18, 51)), "33 length classes"), ([17, 100], "17"), ([100, 511], "511"), ([150, 100], "100"), ([100, 100], "100")):
        with pytest.raises(RuntimeError, match=word):
            engine.set_run_classes(cl)
    _set_classes(engine, [100, 150])
    with pytest.raises(RuntimeError, match="stride 140"):
        engine.search_classes(np.full((4, 140), 65, np.uint8))
    # a range in flight
    engine.upload(np.full((8, 150), 65, np.uint8))
    engine.range_begin(0, 8)
    try:
        with pytest.raises(RuntimeError, match="in flight"):
            engine.search_classes(np.full((4, 150), 65, np.uint8))
        with pytest.raises(RuntimeError, match="in flight"):
            engine.set_run_classes([100, 150])
    finally:
        engine.range_end()
    # a reader of other classes, and a single-length reader on a class handle
    for rd in (_native.Reader.with_classes([__file__], [100, 140, 150], 10, False, 0, -5, -5, 100, False), _native.Reader([__file__], 150, 10, False, 0, -5, -5, 100, False)):
        try:
            with pytest.raises(RuntimeError, match="length classes"):
                engine.search_files(rd)
        finally:
            rd.close()
    engine.set_run(150)
    rd = _native.Reader.with_classes([__file__], [100, 150], 10, False, 0, -5, -5, 100, False)
    try:
        with pytest.raises(RuntimeError, match="mc_set_run_classes"):
            engine.search_files(rd)
    finally:
        rd.close()


@pytest.mark.parametrize("n", [1, 4096, 4097, 20011, (1 << 21) - 1])
def test_prologue_against_numpy(engine, n):
    # (the largest batch at a small stride; 20011 rows at the longest legal stride: 64 lanes per row)
    classes = [18, 20, 24, 31, 40] if n > 100000 else [50, 200, 400, 505, 510] if n == 20011 else [50, 60, 100, 150, 300]
    stride = classes[-1]
    rng = np.random.default_rng(n)
    lens = rng.integers(0, stride + 1, size=n)
    rows = rng.integers(65, 91, size=(n, stride), dtype=np.uint8)
    rows[np.arange(stride)[None, :] >= lens[:, None]] = 0
    engine.set_run_classes(classes)
    perm, start, word0, srt, ms = engine.classes_prologue(rows)
    wperm, wstart, wword0, wsrt = cr.prologue(rows, classes)
    assert (start == wstart).all() and (word0 == wword0).all()
    assert (perm == wperm).all()
    assert len(srt) == len(wsrt) and (srt == wsrt).all()


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, s.decode()))
    return str(path)


def test_pipeline_equals_its_per_class_runs(mixed, tmp_path):
    seqs, lens = mixed
    path = _write_fasta(tmp_path / "mixed.fa", seqs)
    est, args = mc.run_pipeline({"seqfiles": [path], "outfile": str(tmp_path / "o.txt"), "mixed_lengths": True, "nreads": 10 ** 9})
    classes = args["length_classes"]
    assert len(classes) >= 5 and args["read_length"] == "mixed"
    cls = cr.class_of(lens, classes)
    assert args["class_reads"] == np.bincount(cls, minlength=len(classes) + 1)[:len(classes)].tolist()
    assert args["sampled_reads"] == int((cls < len(classes)).sum())
    sums = []
    for k, L in enumerate(classes):
        part = _write_fasta(tmp_path / ("c%d.fa" % L), [s for s, c in zip(seqs, cls) if c == k])
        a = {"seqfiles": [part], "read_length": L, "nreads": 10 ** 9}
        mc.check_input(a)
        mc.impute_missing_args(a)
        paths = mc.get_relative_paths(a)
        try:
            mc._sample_search_classify(a, paths)
            cache = mc._run_cache[paths["tempfile"]]
            sums.append(mc.aggregate_hits(a, paths, mc._BestHits(cache["best"], cache["families"])))
        finally:
            mc.clean_up(paths)
        assert a["sampled_reads"] == args["class_reads"][k]
    assert sums == args["class_sums"]
    assert est == mc.pooled_ags(mc._model(), classes, args["class_reads"], sums)
    # the Python statement of the sampler gives the same estimate
    est_py, args_py = mc.run_pipeline({"seqfiles": [path], "outfile": str(tmp_path / "p.txt"), "mixed_lengths": classes, "nreads": 10 ** 9, "python_reader": True})
    assert est_py == est and args_py["class_reads"] == args["class_reads"]
    mc.report_results(args, est, None)
    text = open(args["outfile"]).read()
    assert "trimmed_length:\tmixed\n" in text and "length_classes:\t%s\n" % "\t".join(map(str, classes)) in text
    assert "class_reads:\t%s\n" % "\t".join(map(str, args["class_reads"])) in text


def test_reads_of_one_legal_length_give_todays_ags(mixed, tmp_path):
    seqs, lens = mixed
    path = _write_fasta(tmp_path / "one.fa", [s[:150] for s, n in zip(seqs, lens) if n >= 150])
    want, a = mc.run_pipeline({"seqfiles": [path], "outfile": str(tmp_path / "a.txt"), "nreads": 10 ** 9})
    got, b = mc.run_pipeline({"seqfiles": [path], "outfile": str(tmp_path / "b.txt"), "nreads": 10 ** 9, "mixed_lengths": True})
    assert a["read_length"] == 150 and b["length_classes"] == [150] and b["class_reads"] == [a["sampled_reads"]]
    assert got == want


def test_validate_length_mix_pools_its_passes(tmp_path):
    """validate(length_mix=...): the 100+150 row is the pooled estimate of one pass per class, each with its own library id"""
    import gzip
    import community_restated as cmr
    from microbecensus_amd import training, validation
    genomes = cmr.fixture_members()[:6]
    gdir = tmp_path / "genomes"
    gdir.mkdir()
    for name, bases, off in genomes:
        with gzip.open(str(gdir / (name + ".fna.gz")), "wb", compresslevel=1) as f:
            for k in range(len(off) - 1):
                f.write(b">c%d\n" % k + bases[off[k]: off[k + 1]].tobytes() + b"\n")
    mix = validation.parse_length_mix("100:0.4,150:0.6")
    n = 50001
    recs = validation.validate(str(gdir), str(tmp_path / "out"), [150], n, random=1, members=4, seed=5, length_mix=mix)
    assert [r["read_length"] for r in recs] == [150, "100+150"]
    r = recs[1]
    assert r["class_reads"] == [20000, 30001] and r["reads"] == 50001 and sum(r["member_reads"]) == 50001
    names, abund = validation.random_community([g[0] for g in genomes], 0, 4, 1.0, 5)
    copies = validation.copies_of(names, abund)
    by = {g[0]: (g[1], g[2]) for g in genomes}
    comm = _native.Community([by[g] for g in names], copies, 0)
    eng = _native.Engine(device=0)
    try:
        sums = []
        for (L, _), n_k in zip(mix, r["class_reads"]):
            eng.set_run(L, MODEL["pars"][str(L)], FAMS)
            best = eng.community_library(comm, n_k, 5, training.library_id("random000|100+150", L))
            sums.append(mc.aggregate_hits({"read_length": L, "verbose": False}, {}, mc._BestHits(best, FAMS)))
    finally:
        comm.close()
        eng.close()
    assert r["est_ags"] == mc.pooled_ags(mc._model(), [100, 150], r["class_reads"], sums)
    assert r["error"] == (r["est_ags"] - r["true_ags"]) / r["true_ags"] and r["true_ags"] == recs[0]["true_ags"]
    rows = training.read_map(str(tmp_path / "out" / "validation.map"), header=True)
    assert rows[1][:4] == ["random000", "100+150", "4", "50001"] and float(rows[1][5]) == r["est_ags"]
    tsv = training.read_map(str(tmp_path / "out" / "communities" / "random000.tsv"), header=True)
    assert [int(x[4]) for x in tsv] == r["member_reads"]


def _same_rows(a, b):
    """m8 rows equal field by field (the record has padding bytes, which nobody writes)"""
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in a.dtype.names)


def test_class_piece_boundaries_and_handle_back(engine, mixed, monkeypatch):
    """1,000, 1,001 and 1 rows of three classes beside 3 rows too short, interleaved, at the smallest batch: the rows arrive in batches of
    1,000, 1,000 and 5, each cut into one piece per class present (a class never exceeds its batch, so no class is cut in two here;
    test_every_class_equals_its_single_length_run does that).  Best hits and classes are those of the per-class single-length runs,
    and a second class run straight after is byte-identical.
    The handle comes back: a fixed-length search at the top class's length and a run over resident reads, taken after
    mc_set_run_classes, are repeated after the class runs with NO mc_set_run or mc_set_run_classes between, the last of them a run
    whose last piece is of 100 bp - so length, frame pitch, tables, parameters (d_P) and the resident reads were all another
    class's when it ended, and only the restore makes them the top class's again."""
    seqs, lens = mixed
    classes, counts = [50, 100, 150], [1000, 1001, 1, 3]
    all_cls = cr.class_of(np.minimum(lens, classes[-1]), classes)
    pick = np.concatenate([np.flatnonzero(all_cls == k)[:c] for k, c in enumerate(counts)])
    np.random.default_rng(5).shuffle(pick)                                       # the classes interleaved: every batch of rows holds several
    rows = cr.make_rows([seqs[i] for i in pick], classes[-1])
    want_cls = all_cls[pick]
    r150 = np.stack([np.frombuffer(s[:150], np.uint8) for s, n in zip(seqs, lens) if n >= 150][:2000])
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")
    _set_classes(engine, classes)
    rows0, best0 = engine.search(r150)                                           # the handle's single-length state: the top class's
    engine.upload(r150[:700])
    engine.run(first_read_id=5)
    res0 = engine.results()
    assert len(rows0) > 0 and len(best0) > 0 and len(res0[1]) > 0
    best, cls, class_reads = engine.search_classes(rows, first_read_id=7)
    assert engine.stats()["reads"] == len(rows) == 2005 and len(engine.rows()) == 0
    best2, cls2, class_reads2 = engine.search_classes(rows, first_read_id=7)
    assert len(best) > 0 and best2.tobytes() == best.tobytes() and cls2.tobytes() == cls.tobytes()
    assert class_reads.tolist() == counts == class_reads2.tolist()
    assert (np.diff(best["read"]) > 0).all() and (cls == want_cls[best["read"] - 7]).all()
    _, cls3, class_reads3 = engine.search_classes(rows[want_cls < 2][:1500])     # batches of 1,000 and 500: the last piece is of class 0 or 1
    assert class_reads3[2:].tolist() == [0, 0] and len(cls3) > 0
    engine.run(first_read_id=5)                                                  # the resident reads are still the uploaded ones
    res1 = engine.results()
    assert _same_rows(res1[0], res0[0]) and res1[1].tobytes() == res0[1].tobytes()
    rows1, best1 = engine.search(r150)
    assert _same_rows(rows1, rows0) and best1.tobytes() == best0.tobytes()
    with_hits = 0
    for k, L in enumerate(classes):
        idx = np.flatnonzero(want_cls == k)
        got = best[cls == k].copy()
        got["read"] = np.searchsorted(idx, got["read"] - 7)                      # renumbered by rank inside the class
        engine.set_run(L, MODEL["pars"][str(L)], FAMS)
        _, want = engine.search(rows[idx, :L])
        assert _same(got, want), "class %d (%d bp)" % (k, L)
        with_hits += len(want) > 0
    assert with_hits >= 1 and len(best[cls == 1]) > 0
