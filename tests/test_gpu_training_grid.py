"""The training grid (csrc/k_grid.h k_grid_classify, grid_pars / grid_counts, train_range) against the reference's classify_reads
(training/training.py:311-334) on what training feeds it: whole simulated libraries against the reference's own .hits tables
(tests/golden/training_library_<case>.json.gz), and, where no golden exists, against tests/grid_restated.py (the plain restatement
the CPU test pins to those tables) over the oracle's m8 of the same reads: read lengths across L mod 3, non-default grids, a small
--gene-fams marker set with ties, and the pool-overflow halving inside train_range.  Every test asserts that its input exercises
what it claims to."""
import gzip
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

import grid_restated as gr
import simlib_restated as sr
from microbecensus_amd import _native, synth, training

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
import make_training_library_golden as mk  # noqa: E402

GRID = (training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)


@pytest.fixture(scope="module")
def packaged():
    """(gene2fam, gene2len, families) of the packaged marker set."""
    names, seqs = _native.load_markers()
    model = _native.load_model()
    fams = model["families"]
    return {n: fams[f] for n, f in zip(names, model["marker_family"])}, {n: len(s) for n, s in zip(names, seqs)}, fams


def oracle_m8(reads, tmp_path, tag, rapdb=mk.RAPDB):
    """The oracle's m8 text of the reads (headers = read indices), at most 16 processes."""
    return mk.oracle_m8(reads, str(tmp_path), tag, rapdb).decode()


def restated(text, grid, gene2fam, gene2len, fams, L):
    """tests/grid_restated.classify as (hits, aln, cov) arrays of the engine's shape."""
    aln_covs, max_pids, min_scores = grid
    shape = (len(aln_covs), len(max_pids), len(min_scores), len(fams))
    hits = np.zeros(shape, np.int64); aln = np.zeros(shape, np.int64); cov = np.zeros(shape, np.float64)
    for (ic, ip, js, fam), (h, a, c) in gr.classify(text, aln_covs, max_pids, min_scores, gene2len, gene2fam, fams, str(L)).items():
        f = fams.index(fam)
        hits[ic, ip, js, f], aln[ic, ip, js, f], cov[ic, ip, js, f] = h, a, c
    return hits, aln, cov


def assert_grid_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "hits", np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(got[1], want[1]), (what, "aln", np.argwhere(got[1] != want[1])[:5])
    bad = np.abs(got[2] - want[2]) > 1e-12 * np.abs(want[2])
    assert not bad.any(), (what, "cov", np.argwhere(bad)[:5])


def m8_counts(text, gene2fam, gene2len):
    """Rows, rows with gapopen > 0, reverse-strand rows, reads with a consequential best-score tie."""
    lines = text.splitlines()
    gapped = sum(1 for line in lines if int(line.split()[5]) > 0)
    reverse = sum(1 for line in lines if float(line.split()[6]) > float(line.split()[7]))
    return len(lines), gapped, reverse, gr.consequential_ties(text, gene2fam, gene2len)


def golden_arrays(gold, fams):
    shape = (len(gold["aln_covs"]), len(gold["max_pids"]), len(gold["min_scores"]), len(fams))
    hits = np.zeros(shape, np.int64); aln = np.zeros(shape, np.int64); cov = np.zeros(shape, np.float64)
    for fam, aln_cov, max_pid, min_score, h, a, c in gold["rows"]:
        k = (gold["aln_covs"].index(aln_cov), gold["max_pids"].index(max_pid), gold["min_scores"].index(min_score), fams.index(fam))
        hits[k], aln[k], cov[k] = h, a, c
    assert int((hits > 0).sum()) == gold["n_rows_with_hits"]
    return hits, aln, cov


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_library_pass_equals_reference_golden(case, packaged, monkeypatch, tmp_path):
    """A whole library (Genome + set_library + train_library, in >= 3 ranges) against the .hits table the reference's own
    classify_reads made of the oracle's m8 of the same reads; the pinned path's m8 against the oracle's, so a failure points at
    the search or at the grid."""
    gene2fam, gene2len, fams = packaged
    gold = json.load(gzip.open(os.path.join(GOLD, "training_library_%s.json.gz" % case), "rt"))
    lib = gold["library"]
    L, n, seed, lid, kind = lib["read_len"], lib["nreads"], lib["seed"], lib["library_id"], lib["kind"]
    name, bases, off = mk.load_genome(lib["genome_index"])
    assert name == lib["genome"] and lid == training.library_id(name, L)
    batch = max(1000, 2 * ((n // 3) // 2))                      # (even: a range never parts the mates of a pair)
    monkeypatch.setenv("MC_STREAM_BATCH", str(batch))
    assert math.ceil(n / batch) >= 3
    want = golden_arrays(gold, fams)
    assert want[0].sum() > 5000
    text = gzip.open(os.path.join(GOLD, "training_library_%s.m8.gz" % case), "rt").read()
    rows, gapped, reverse, ties = m8_counts(text, gene2fam, gene2len)
    print(case, lib, "ranges", math.ceil(n / batch), "rows", rows, "gapped", gapped, "reverse", reverse, "consequential ties", ties)
    assert reverse > 0 and ties > 0 and (gapped > 0 or not kind.get("error_model"))
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        g.set_library(**kind)
        eng.set_run(L)
        got = eng.train_library(g, n, seed, lid, *GRID)
        assert eng.stats()["reads"] == n
        again = eng.train_library(g, n, seed, lid, *GRID)
        print("two identical passes: cov bitwise equal:", bool(np.array_equal(got[2], again[2])))
        # the pinned path: the device's reads, searched, as m8 text
        reads = eng.simulate(g, n, seed, lid)
        eng.search(reads)
        m8 = tmp_path / "pinned.m8"
        eng.write_m8(str(m8))
        assert hashlib.md5(m8.read_bytes()).hexdigest() == gold["m8_md5"], "the search's m8 differs from the oracle's"
        pinned = eng.grid_classify(*GRID)
    finally:
        eng.close()
        g.close()
    assert_grid_equal(pinned, want, "grid_classify")
    assert_grid_equal(got, want, "train_library")
    assert_grid_equal(again, want, "train_library, again")


def test_read_lengths_across_l_mod_3(packaged, tmp_path):
    """train_library at read lengths of every L mod 3 (mc_row_coverage's read_len / 3.0) on Illumina reads, against the restatement
    over the oracle's m8 of the same reads."""
    gene2fam, gene2len, fams = packaged
    name, bases, off = mk.load_genome(3)
    kind = dict(error_model="illumina")
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    mods, total_gapped, total_hits = set(), 0, 0
    try:
        g.set_library(**kind)
        for L in (33, 64, 100, 150, 199, 301, 500):
            n, seed, lid = (1500 if L > 300 else 3000), 20 + L, training.library_id(name, L)
            text = oracle_m8(sr.simulate(bases, off, L, 0, n, seed, lid, **kind), tmp_path, "L%d" % L)
            rows, gapped, reverse, ties = m8_counts(text, gene2fam, gene2len)
            eng.set_run(L)
            got = eng.train_library(g, n, seed, lid, *GRID)
            want = restated(text, GRID, gene2fam, gene2len, fams, L)
            print("L", L, "rows", rows, "gapped", gapped, "reverse", reverse, "ties", ties, "hits at the loosest cell", int(want[0][0, -1, 0].sum()))
            assert_grid_equal(got, want, "L=%d" % L)
            if L >= 64:
                assert want[0].sum() > 0 and reverse > 0, L
            mods.add(L % 3)
            total_gapped += gapped
            total_hits += int(want[0].sum())
    finally:
        eng.close()
        g.close()
    assert mods == {0, 1, 2} and total_gapped > 0 and total_hits > 0


NONDEFAULT_GRIDS = [
    # unsorted, duplicated and fractional cut-offs; unsorted coverages and identities, max_pid 0 and 100
    ([0.5, 0.0, 0.25], [100, 0, 90], [30.5, 23, 49.99, 23]),
    # the limits: 8 aln_covs (1.0 among them) x 8 max_pids x 64 min_scores, cut-offs in a scrambled order
    ([0.0, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 1.0], [0, 40, 60, 75, 85, 95, 99, 100], [20.0 + 0.5 * ((37 * k) % 64) for k in range(64)]),
]


def test_nondefault_grids(packaged, monkeypatch, tmp_path):
    """grid_classify and train_library on one library with grids training never uses, against the restatement on the oracle's
    m8 of the same reads (the pinned path's m8 equals it)."""
    gene2fam, gene2len, fams = packaged
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")
    name, bases, off = mk.load_genome(4)
    L, n, seed, lid, kind = 150, 3000, 31, training.library_id(name, 150), dict(error_model="illumina")
    text = oracle_m8(sr.simulate(bases, off, L, 0, n, seed, lid, **kind), tmp_path, "nd")
    rows, gapped, reverse, ties = m8_counts(text, gene2fam, gene2len)
    print("rows", rows, "gapped", gapped, "reverse", reverse, "ties", ties)
    assert gapped > 0 and reverse > 0 and ties > 0
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        g.set_library(**kind)
        eng.set_run(L)
        eng.search(eng.simulate(g, n, seed, lid))
        m8 = tmp_path / "pinned.m8"
        eng.write_m8(str(m8))
        assert m8.read_text() == text
        for grid in NONDEFAULT_GRIDS:
            want = restated(text, grid, gene2fam, gene2len, fams, L)
            covs, pids, scores = grid
            # the edges carry something: max_pid 0 passes nothing, 100 passes rows; aln_cov 1.0 and the duplicated cut-offs count
            assert want[0][:, pids.index(0)].sum() == 0 and want[0][:, pids.index(100)].sum() > 0
            if 1.0 in covs:
                assert want[0][covs.index(1.0)].sum() > 0
            if scores.count(23) == 2:
                i, j = [k for k, s in enumerate(scores) if s == 23]
                assert np.array_equal(want[0][:, :, i], want[0][:, :, j]) and want[0][:, :, i].sum() > want[0][:, :, scores.index(30.5)].sum() > 0
            assert_grid_equal(eng.grid_classify(*grid), want, ("grid_classify", len(scores)))
        for grid in NONDEFAULT_GRIDS:
            got = eng.train_library(g, n, seed, lid, *grid)
            assert_grid_equal(got, restated(text, grid, gene2fam, gene2len, fams, L), ("train_library", len(grid[2])))
    finally:
        eng.close()
        g.close()


def test_small_family_set_with_ties(tmp_path):
    """A --gene-fams marker set of 3 families (training.build_marker_set) with a protein repeated under a second family (dropped:
    the first occurrence of a sequence is kept) and truncated copies of one protein in the other families (another target length):
    reads of that protein tie between families, and first-on-tie must decide the family as classify_reads decides it."""
    names, seqs = _native.load_markers()
    model = _native.load_model()
    fams = model["families"][:3]
    by_fam = [[(nm, sq) for nm, sq, mf in zip(names, seqs, model["marker_family"]) if mf == fi][:60] for fi in range(3)]
    base_name, base_seq = next((nm, sq) for nm, sq in by_fam[0] if len(sq) > 250)
    by_fam[1].append(("dup_" + base_name, base_seq))                 # the same sequence again, in family 1
    by_fam[1].append(("tail_" + base_name, base_seq[:-20]))            # truncated at the end, in family 1
    by_fam[2].append(("head_" + base_name, base_seq[15:]))             # truncated at the start, in family 2
    fam_dir = tmp_path / "fams"
    fam_dir.mkdir()
    for fam, recs in zip(fams, by_fam):
        with gzip.open(fam_dir / (fam + ".faa.gz"), "wt") as f:
            f.write("".join(">%s\n%s\n" % r for r in recs))
    cn, cs, cf, cfam = training.build_marker_set(training.list_families(str(fam_dir)))
    assert cfam == fams and "dup_" + base_name not in cn and "tail_" + base_name in cn and "head_" + base_name in cn
    gene2fam = {nm: cfam[f] for nm, f in zip(cn, cf)}
    gene2len = {nm: len(sq) for nm, sq in zip(cn, cs)}
    rapdb = str(tmp_path / "custom_db")
    _native.rapdb_write(cn, cs, rapdb)
    # a genome of the set's proteins, with copies of the truncated protein among them
    bases = np.concatenate([synth.build_genomes(cs, total_bp=150_000, seed=61, marker_gene_fraction=1.0),
                            synth.build_genomes([base_seq], total_bp=30_000, seed=62, marker_gene_fraction=1.0, divergence=0.1)])
    off = np.array([0, len(bases)], np.int64)
    L, n, seed, lid = 150, 4000, 63, training.library_id("custom", 150)
    text = oracle_m8(sr.simulate(bases, off, L, 0, n, seed, lid), tmp_path, "fam", rapdb=rapdb)
    rows, gapped, reverse, ties = m8_counts(text, gene2fam, gene2len)
    cross = sum(1 for t in _top_families(text, gene2fam) if len(t) > 1)
    print("rows", rows, "gapped", gapped, "reverse", reverse, "consequential ties", ties, "ties across families", cross)
    assert ties > 0 and cross > 0 and reverse > 0
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0, names=cn, seqs=cs, marker_family=cf, nfam=len(cfam))
    try:
        eng.set_run(L)
        got = eng.train_library(g, n, seed, lid, *GRID)
        eng.search(eng.simulate(g, n, seed, lid))
        m8 = tmp_path / "pinned.m8"
        eng.write_m8(str(m8))
        assert m8.read_text() == text
    finally:
        eng.close()
        g.close()
    want = restated(text, GRID, gene2fam, gene2len, cfam, L)
    assert want[0].sum() > 0
    assert_grid_equal(got, want, "custom marker set")


def _top_families(text, gene2fam):
    top = {}
    for q, t, _, _, _, _, _, _, score in gr.parse_m8(text):
        cur = top.get(q)
        if cur is None or cur[0] < score:
            top[q] = [score, {gene2fam[t]}]
        elif cur[0] == score:
            cur[1].add(gene2fam[t])
    return [v[1] for v in top.values()]


def test_pool_overflow_halving_in_train_range(packaged, monkeypatch, tmp_path):
    """A marker-dense library overflows the pools of its one range, and train_range runs it in halves: the grid must be that of
    the same library in small ranges that fit, and a prefix must be the restatement's over the oracle's m8."""
    gene2fam, gene2len, fams = packaged
    names, seqs = _native.load_markers()
    bases = synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0)
    off = np.array([0, len(bases)], np.int64)
    L, n, seed, lid = 150, 60_000, 71, training.library_id("dense", 150)
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(L)
        whole = eng.train_library(g, n, seed, lid, *GRID)
        st = eng.stats()
        print("one range:", st)
        assert st["range_splits"] > 0, "the range did not overflow: the test no longer exercises the halving in train_range"
        monkeypatch.setenv("MC_STREAM_BATCH", "5000")
        small = eng.train_library(g, n, seed, lid, *GRID)
        st = eng.stats()
        print("ranges of 5,000:", st)
        assert st["range_splits"] == 0
        m = 1000
        prefix = eng.train_library(g, m, seed, lid, *GRID)
    finally:
        eng.close()
        g.close()
    assert whole[0].sum() > 0
    assert_grid_equal(whole, small, "halved against small ranges")
    text = oracle_m8(sr.simulate(bases, off, L, 0, m, seed, lid), tmp_path, "dense")
    rows, gapped, reverse, ties = m8_counts(text, gene2fam, gene2len)
    print("prefix rows", rows, "gapped", gapped, "reverse", reverse, "ties", ties)
    assert ties > 0
    want = restated(text, GRID, gene2fam, gene2len, fams, L)
    assert want[0].sum() > 0
    assert_grid_equal(prefix, want, "prefix against the restatement")


def test_grid_refusals():
    name, bases, off = mk.load_genome(0)
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(100)
        eng.search(eng.simulate(g, 2000, 1, 1))
        covs, pids, scores = GRID
        for call in (lambda *grid: eng.grid_classify(*grid), lambda *grid: eng.train_library(g, 2000, 1, 1, *grid)):
            for bad in ([50, 97.5], [float("nan")], [float("inf")]):
                with pytest.raises(ValueError, match="max_pids must be integers"):
                    call(covs, bad, scores)
            for bad in (float("nan"), float("inf"), -float("inf")):
                with pytest.raises(RuntimeError, match=r"min_scores\[1\] is not finite"):
                    call(covs, pids, [23.0, bad, 30.0])
                with pytest.raises(RuntimeError, match=r"aln_covs\[2\] is not finite"):
                    call([0.0, 0.5, bad], pids, scores)
            for shape in ((9, 8, 64), (8, 9, 64), (8, 8, 65)):
                with pytest.raises(RuntimeError, match="grid larger than 8 x 8 x 64"):
                    call([0.1 * k for k in range(shape[0])], list(range(50, 50 + shape[1])), [23.0 + k for k in range(shape[2])])
            h, a, c = call([0.1 * k for k in range(8)], [60 + 5 * k for k in range(8)], [23.0 + 0.5 * k for k in range(64)])
            assert h.shape == (8, 8, 64, eng.nfam) and h.sum() > 0
            h, _, _ = call(covs, [50.0, 100.0], scores)                # integral floats are integers
            assert h.shape[1] == 2
    finally:
        eng.close()
        g.close()
