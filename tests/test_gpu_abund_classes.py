"""The abundance counts on class runs (mc_set_abundance_classes; csrc/k_abund_classes.h and include/mcensus.h state the rule): a class
run of 30,000 reads of 40 - 320 bp in four classes against THE MERGED FIXED-LENGTH PATH - per class set_run(L_k), the counts, coverage
and ties, and a search of that class's reads cut to L_k - whose counters, summed over the classes, the class run equals integer for
integer; the per-class table against numpy; the gene bootstrap under global read ids against tests/geneboot_restated.py applied to the
host rows of the per-class runs; one class against set_run + search byte for byte; the refusals of the ABI.  The engine runs on the
packaged markers as the genes; all calls go through the C ABI."""
import ctypes as C

import numpy as np
import pytest

from microbecensus_amd import _native, synth

import abundance_restated as R
import classes_restated as cr
import geneboot_restated as GR

pytestmark = pytest.mark.gpu

CLASSES = [50, 100, 150, 300]
FIRST, B, SEED, CAP = 7, 64, 11, 30_000


@pytest.fixture(scope="module")
def engine():
    e = _native.Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed():
    """test_gpu_classes.py's `mixed` recipe: 30,000 reads of marker-bearing genomes, each cut to a seeded length in 40 .. 320"""
    _, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=1_500_000, seed=31, marker_gene_fraction=0.3)
    full = synth.sample_reads(genome, 30_000, 320, seed=32)
    lens = np.random.default_rng(33).integers(40, 321, size=len(full))
    return [bytes(full[i, :lens[i]]) for i in range(len(full))], lens


def _switches(e, boot=None):
    e.set_abundance(True)
    e.set_coverage(True)
    e.set_ties(True)
    if boot:
        e.set_gene_bootstrap(boot)


def _take(e):
    ab, ti = e.abundance(), e.ties()
    return {"reads": ab["reads"], "aligned": ab["aligned"], "assigned": ab["assigned"], "searched": ab["searched"], "depth": e.coverage_depth().astype(np.int64),
            "candidates": ti["candidates"], "unique": ti["unique"], "share": ti["share"], "ambiguous": ti["ambiguous"]}


SUMMED = ("reads", "aligned", "assigned", "searched", "depth", "candidates", "unique", "share", "ambiguous")


@pytest.fixture(scope="module")
def oracle(engine, mixed):
    """the merged fixed-length path, computed once, shared, never changed: per class the counters of set_run(L_k) + search on that class's
    reads cut to L_k, and the (global id, gene) of every read the restatement assigns from the host rows of that search"""
    seqs, lens = mixed
    rows = cr.make_rows(seqs, CLASSES[-1])
    want_cls = cr.class_of(np.minimum(lens, CLASSES[-1]), CLASSES)
    nseq = len(engine.names)
    per, q, s = [], [], []
    for k, L in enumerate(CLASSES):
        idx = np.flatnonzero(want_cls == k)
        engine.set_run(L)
        _switches(engine)
        try:
            host, _ = engine.search(rows[idx, :L])
            per.append(_take(engine))
            rank, gene = GR.assignments(R.rows_from_array(host), nseq)
        finally:
            engine.set_abundance(False)
        q.append(FIRST + idx[rank])
        s.append(gene)
    return {"rows": rows, "want_cls": want_cls, "per": per, "q": np.concatenate(q), "s": np.concatenate(s), "nseq": nseq}


def test_class_run_equals_the_merged_fixed_length_runs(engine, oracle, monkeypatch):
    o = oracle
    scale = np.random.default_rng(3).uniform(1e-4, 1e-3, B)
    scale[[5, 40]] = [np.nan, 0.0]
    engine.set_run_classes(CLASSES)
    _switches(engine, CAP)
    try:
        engine.set_abundance_classes(True)
        best, cls, class_reads = engine.search_classes(o["rows"], first_read_id=FIRST)
        assert len(engine.rows()) == 0 and engine.stats()["reads"] == len(o["rows"])
        got, tab, gb = _take(engine), engine.abundance_classes(), engine.gene_bootstrap(B, SEED, scale, counts=True)
        engine.abundance_reset()
        monkeypatch.setenv("MC_STREAM_BATCH", "7000")                                # batches and ranges that split every class
        best_s, cls_s, reads_s = engine.search_classes(o["rows"], first_read_id=FIRST)
        monkeypatch.delenv("MC_STREAM_BATCH")
        got_s, tab_s, gb_s = _take(engine), engine.abundance_classes(), engine.gene_bootstrap(B, SEED, scale, counts=True)
        ms = engine.abundance_classes_ms()
    finally:
        engine.set_abundance(False)
    # plain and split: identical
    assert best.tobytes() == best_s.tobytes() and cls.tobytes() == cls_s.tobytes() and (class_reads == reads_s).all()
    for key in SUMMED:
        assert np.array_equal(got[key], got_s[key]), key
    assert all(np.array_equal(tab[key], tab_s[key]) for key in ("rows", "assigned"))
    assert np.array_equal(gb["counts"], gb_s["counts"]) and GR.same_bits(gb["stats"], gb_s["stats"]) and ms > 0.0
    # counts, aligned residues, the depth and the tie counters (shares in 2^-32 units): the sums over the classes, integer for integer
    K = len(CLASSES)
    for key in SUMMED:
        want = sum(np.asarray(p[key]).astype(np.uint64 if key == "share" else np.int64) for p in o["per"])
        if key == "searched":
            want = want + int((o["want_cls"] == K).sum())                            # the rows below the lowest class are searched too
        assert np.array_equal(np.asarray(got[key]).astype(want.dtype if hasattr(want, "dtype") else np.int64), want), key
    assert got["searched"] == len(o["rows"])
    # the best hits of the class run are what a class run without the counts returns
    engine.set_run_classes(CLASSES)
    plain, plain_cls, plain_reads = engine.search_classes(o["rows"], first_read_id=FIRST)
    assert best.tobytes() == plain.tobytes() and cls.tobytes() == plain_cls.tobytes() and (class_reads == plain_reads).all()
    # the per-class table
    assert np.array_equal(tab["rows"], np.bincount(o["want_cls"], minlength=K + 1)) and np.array_equal(tab["rows"], class_reads)
    assert tab["assigned"].tolist() == [int(p["assigned"]) for p in o["per"]] + [0]
    # the gene bootstrap under global ids
    want = GR.counts(o["q"], o["s"], o["nseq"], B, SEED)
    assert len(o["q"]) == got["assigned"] and gb["dropped"] == 0 and gb["used"] == B - 2
    assert np.array_equal(gb["counts"], want)
    assert GR.same_bits(gb["stats"], GR.stats(want, scale))
    # guards against an empty pass
    print("assigned per class", tab["assigned"].tolist(), "rows", tab["rows"].tolist(), "ambiguous", got["ambiguous"], "class kernel ms", ms)
    assert int((tab["assigned"][:K] > 0).sum()) >= 3 and got["ambiguous"] > 0 and tab["rows"][K] > 0 and len(o["q"]) > 0
    assert len(np.unique(o["q"])) == len(o["q"]) and o["q"].min() >= FIRST


def test_one_class_gives_the_tables_of_set_run_byte_for_byte(engine, mixed):
    seqs, lens = mixed
    L = 150
    cut = np.stack([np.frombuffer(s[:L], np.uint8) for s, n in zip(seqs, lens) if L <= n < 175][:4000])
    engine.set_run(L)
    _switches(engine)
    try:
        engine.search(cut, first_read_id=100)
        want = _take(engine)
    finally:
        engine.set_abundance(False)
    engine.set_run_classes([L])
    _switches(engine)
    try:
        engine.set_abundance_classes(True)
        engine.search_classes(cut, first_read_id=100)                                # (rows of the top class's length: every read fills its row)
        got, tab = _take(engine), engine.abundance_classes()
    finally:
        engine.set_abundance(False)
    assert want["assigned"] > 0
    for key in SUMMED:
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    assert tab["rows"].tolist() == [len(cut), 0] and tab["assigned"].tolist() == [want["assigned"], 0]


def test_refusals_through_the_abi(engine, mixed):
    lib, h = engine.lib, engine.h

    def err():
        return lib.mc_last_error().decode()
    seqs, lens = mixed
    rows = cr.make_rows(seqs[:3000], 150)
    r150 = np.stack([np.frombuffer(s[:150], np.uint8) for s, n in zip(seqs, lens) if n >= 150][:2000])
    out = (C.c_int64 * 3)()
    engine.set_run_classes([100, 150])
    assert lib.mc_set_abundance_classes(h, 1) != 0 and "abundance counting is off" in err() and "on = 1" in err()
    assert lib.mc_abundance_classes_read(h, out, out, 3) != 0 and "mc_set_abundance_classes" in err()
    assert lib.mc_set_abundance_classes(h, 0) == 0                                   # off while off: nothing to do
    engine.set_abundance(True)
    try:
        before = engine.search(r150)                                                 # the fixed-length counts under plain set_abundance
        counts0 = engine.abundance()
        with pytest.raises(RuntimeError, match="a class run is refused while abundance counting is on"):
            engine.search_classes(rows)
        engine.set_curve([10, 20])
        assert lib.mc_set_abundance_classes(h, 1) != 0 and "the curve is on" in err() and "K = 2" in err()
        engine.set_curve(None)
        engine.upload(r150[:500])
        engine.range_begin(0, 500, 0)
        try:
            assert lib.mc_set_abundance_classes(h, 1) != 0 and "still in flight" in err() and "on = 1" in err()
        finally:
            engine.range_end()
        engine.set_abundance_classes(True)
        with pytest.raises(RuntimeError, match=r"mc_set_curve: refused while the counts may ride on class runs .*K = 2"):
            engine.set_curve([10, 20])
        assert lib.mc_abundance_classes_read(h, out, out, 2) != 0 and "2 values" in err() and "2 classes" in err()
        engine.set_gene_bootstrap(100)
        with pytest.raises(RuntimeError, match="mc_search_varlen: refused while the gene bootstrap is on"):
            engine.search_varlen([bytes(r150[0]), bytes(r150[1][:90])])
        engine.set_gene_bootstrap(0)
        engine.search_classes(rows)
        assert engine.abundance()["searched"] == len(rows) and engine.abundance_classes()["rows"].sum() == len(rows)
        engine.abundance_reset()                                                     # every zeroing zeroes the table too
        assert not engine.abundance_classes()["rows"].any() and not engine.abundance_classes()["assigned"].any()
        engine.set_abundance_classes(False)                                          # the switch off: the refusal is back, with its text
        with pytest.raises(RuntimeError, match="a class run is refused while abundance counting is on"):
            engine.search_classes(rows)
        engine.set_abundance_classes(True)
    finally:
        engine.set_abundance(False)                                                  # the counts going off take the switch with them
    assert lib.mc_abundance_classes_read(h, out, out, 3) != 0 and "mc_set_abundance_classes" in err()
    best, _, class_reads = engine.search_classes(rows)                               # a class run runs again
    assert len(best) > 0 and class_reads.sum() == len(rows)
    engine.set_abundance(True)
    try:
        with pytest.raises(RuntimeError, match="a class run is refused while abundance counting is on"):
            engine.search_classes(rows)
        after = engine.search(r150)
        counts1 = engine.abundance()
    finally:
        engine.set_abundance(False)
    assert counts0["assigned"] > 0 and all(np.array_equal(counts0[k], counts1[k]) for k in ("reads", "aligned", "searched", "assigned"))
    assert before[1].tobytes() == after[1].tobytes()
