"""Training libraries of seq_sim.py's read lengths on the device (mc_genome_set_read_lengths MC_READLEN_REFERENCE): the two-pass
simulator against its restatement, whole library passes against the reference's classify_reads on the oracle's m8 of the same reads
(tests/golden/training_varlen_*.json.gz, tests/golden/make_varlen_training_golden.py), the real base count, the refusals, and
train_microbe_census.py --reference-lengths end to end."""
import gzip
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from microbecensus_amd import _native, training

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
import make_training_library_golden as mk  # noqa: E402
import simlib_varlen_restated as svr  # noqa: E402

GRID = (training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)


def golden_arrays(gold, fams):
    shape = (len(gold["aln_covs"]), len(gold["max_pids"]), len(gold["min_scores"]), len(fams))
    hits = np.zeros(shape, np.int64); aln = np.zeros(shape, np.int64); cov = np.zeros(shape, np.float64)
    for fam, aln_cov, max_pid, min_score, h, a, c in gold["rows"]:
        k = (gold["aln_covs"].index(aln_cov), gold["max_pids"].index(max_pid), gold["min_scores"].index(min_score), fams.index(fam))
        hits[k], aln[k], cov[k] = h, a, c
    assert int((hits > 0).sum()) == gold["n_rows_with_hits"]
    return hits, aln, cov


def assert_grid_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "hits", np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(got[1], want[1]), (what, "aln", np.argwhere(got[1] != want[1])[:5])
    bad = np.abs(got[2] - want[2]) > 1e-12 * np.abs(want[2])
    assert not bad.any(), (what, "cov", np.argwhere(bad)[:5])


@pytest.mark.parametrize("case", ["a", "b"])
def test_reference_length_library_equals_golden(case, monkeypatch):
    """The device's reads are the restatement's (md5 of the golden); a whole library pass in >= 3 ranges gives the reference's
    .hits table (hits and aln exact, cov to 1e-12) and the library's real base count."""
    gold = json.load(gzip.open(os.path.join(GOLD, "training_varlen_%s.json.gz" % case), "rt"))
    lib = gold["library"]
    L, n, seed, lid, kind = lib["read_len"], lib["nreads"], lib["seed"], lib["library_id"], lib["kind"]
    name, bases, off = mk.load_genome(lib["genome_index"])
    assert name == lib["genome"] and lid == training.library_id(name, L)
    batch = 4000
    monkeypatch.setenv("MC_STREAM_BATCH", str(batch))
    assert math.ceil(n / batch) >= 3
    fams = _native.load_model()["families"]
    want = golden_arrays(gold, fams)
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        g.set_library(**kind)
        g.set_read_lengths(True)
        vb, vo = g.simulate_varlen(L, n, seed, lid)
        assert hashlib.md5(vb.tobytes()).hexdigest() == gold["reads_md5"] and int(vo[-1]) == gold["library_bases"]
        assert np.diff(vo).min() == gold["min_len"] and np.diff(vo).max() == gold["max_len"]
        eng.set_run(L)
        got = eng.train_library(g, n, seed, lid, *GRID)
        assert eng.train_library_bases() == gold["library_bases"] != n * L
        assert eng.stats()["reads"] == n
    finally:
        eng.close()
        g.close()
    assert want[0].sum() > 1000
    assert_grid_equal(got, want, case)


def test_reference_lengths_without_errors_is_the_default_mode(monkeypatch):
    """Under error model none both modes make the same reads: the same bins, and n x L bases."""
    monkeypatch.setenv("MC_STREAM_BATCH", "5000")
    name, bases, off = mk.load_genome(3)
    L, n, seed, lid = 150, 12000, 5, training.library_id(name, 150)
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(L)
        fixed = eng.train_library(g, n, seed, lid, *GRID)
        assert eng.train_library_bases() == n * L
        g.set_read_lengths(True)
        ref = eng.train_library(g, n, seed, lid, *GRID)
        assert eng.train_library_bases() == n * L
        vb, vo = g.simulate_varlen(L, n, seed, lid)
        assert (np.diff(vo) == L).all() and vb.tobytes() == g.simulate(L, n, seed, lid).tobytes()
    finally:
        eng.close()
        g.close()
    assert fixed[0].sum() > 0
    assert_grid_equal(ref, fixed, "none")


def test_reference_length_refusals():
    name, bases, off = mk.load_genome(4)
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        with pytest.raises(RuntimeError, match="unknown read-length mode 2"):
            g.set_read_length_mode(2)
        g.set_library("uniform", 0.5)
        g.set_read_lengths(True)
        with pytest.raises(RuntimeError, match="bases long .*longer than 510"):
            g.simulate_varlen(500, 200, 1, 2)
        eng.set_run(500)
        with pytest.raises(RuntimeError, match="longer than 510"):
            eng.train_library(g, 200, 1, 2, *GRID)
    finally:
        eng.close()
        g.close()


def test_train_cli_reference_lengths(tmp_path):
    """train_microbe_census.py --error-model illumina --reference-lengths on two fixture genomes: model.json records the flag, the
    written reads have seq_sim.py's lengths (the restatement's reads), and the rates are the grid's counts over the real bp."""
    genomes_dir, model_dir, reads_dir = tmp_path / "genomes", tmp_path / "model", tmp_path / "reads"
    genomes_dir.mkdir()
    loaded = []
    for k in (6, 7):
        name, bases, off = mk.load_genome(k)
        with gzip.open(str(genomes_dir / (name + ".fna.gz")), "wb", compresslevel=1) as f:
            for c in range(len(off) - 1):
                f.write(b">%s_%d\n%s\n" % (name.encode(), c, bases[off[c]:off[c + 1]].tobytes()))
        loaded.append((name, bases, off))
    env = dict(os.environ)
    env.pop("MC_STREAM_BATCH", None)
    subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_microbe_census.py"), str(genomes_dir), str(model_dir), "-l", "150", "-c", "2",
                    "-x", "2", "--error-model", "illumina", "--reference-lengths", "--write-reads", str(reads_dir)], check=True, env=env, timeout=900)
    model = json.load(open(model_dir / "model.json"))
    assert model["library"] == {"error_model": "illumina", "error_rate": None, "paired_end": False, "insert": None, "reference_lengths": True}
    eng = _native.Engine(device=0)
    try:
        eng.set_run(150)
        for name, bases, off in loaded:
            n = training.library_reads(2, int(off[-1]), 150)
            lid = training.library_id(name, 150)
            fa = open(reads_dir / "150" / (name + "-reads.fa"), "rb").read().splitlines()
            seqs = fa[1::2]
            assert len(seqs) == n and len({len(s) for s in seqs}) > 1
            head = svr.simulate_varlen(bases, off, 150, 0, 200, 0, lid, error_model="illumina")
            assert b"".join(seqs[:200]) == head[0].tobytes()
            g = _native.Genome(bases, off, 0)
            try:
                g.set_library("illumina")
                g.set_read_lengths(True)
                eng.train_library(g, n, 0, lid, *GRID)
                assert eng.train_library_bases() == sum(len(s) for s in seqs)
            finally:
                g.close()
    finally:
        eng.close()


def test_training_rates_use_the_real_bp(tmp_path):
    """training.train(reference_lengths=True): the rates are the grid's counts over each library's real bp (uniform errors at 5 %:
    the totals differ from n x L)."""
    genomes_dir = tmp_path / "genomes"
    genomes_dir.mkdir()
    loaded = []
    for k in (6, 7):
        name, bases, off = mk.load_genome(k)
        with gzip.open(str(genomes_dir / (name + ".fna.gz")), "wb", compresslevel=1) as f:
            for c in range(len(off) - 1):
                f.write(b">%s_%d\n%s\n" % (name.encode(), c, bases[off[c]:off[c + 1]].tobytes()))
        loaded.append((name, bases, off))
    kind = dict(error_model="uniform", error_rate=0.05)
    eng = _native.Engine(device=0)
    counts, bp, nominal = [], [], []
    try:
        eng.set_run(150)
        for name, bases, off in loaded:
            n = training.library_reads(2, int(off[-1]), 150)
            g = _native.Genome(bases, off, 0)
            try:
                g.set_library(**kind)
                g.set_read_lengths(True)
                counts.append(eng.train_library(g, n, 0, training.library_id(name, 150), *GRID))
                bp.append(eng.train_library_bases())
                nominal.append(n * 150)
            finally:
                g.close()
    finally:
        eng.close()
    assert bp != nominal
    rates = training.rates_by_candidate([c[0] for c in counts], [c[1] for c in counts], [c[2] for c in counts], bp)
    got = training.train(str(genomes_dir), str(tmp_path / "model"), [150], 2, xfolds=2, reference_lengths=True, log=lambda *a: None, **kind)
    assert got["library"]["reference_lengths"] is True
    # (the coverage sums are accumulated in no fixed order: 1e-12, the grid's contract)
    assert np.allclose(got["_rates"][150], rates, rtol=1e-12, atol=0)
    rates_nominal = training.rates_by_candidate([c[0] for c in counts], [c[1] for c in counts], [c[2] for c in counts], nominal)
    assert not np.allclose(got["_rates"][150], rates_nominal, rtol=1e-9, atol=0)


def test_handle_comes_back_after_reference_length_training(monkeypatch):
    """A fixed-length search, one reference-length library of three ranges, the same search again WITHOUT another set_run: identical
    rows and best hits - the run's length, frame pitch and tables are the handle's again, and the resident reads hold no range."""
    from microbecensus_amd import synth
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")
    name, bases, off = mk.load_genome(3)
    _, mseqs = _native.load_markers()
    reads = synth.sample_reads(synth.build_genomes(mseqs, total_bp=400_000, seed=7, marker_gene_fraction=0.2), 2000, 150, seed=3)
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(150)
        rows0, best0 = eng.search(reads)
        g.set_library("uniform", 0.05)
        g.set_read_lengths(True)
        eng.train_library(g, 3000, 5, training.library_id(name, 150), *GRID)
        assert eng.stats()["reads"] == 3000 and eng.train_library_bases() != 3000 * 150      # reads of several lengths: the tables were switched
        with pytest.raises(RuntimeError, match="range outside the resident read set"):
            eng.run_range(0, 1)                                                # (training leaves no resident reads behind)
        rows1, best1 = eng.search(reads)
        eng.upload(reads)
        eng.run()
        rows2, best2 = eng.results()
    finally:
        eng.close()
        g.close()
    assert len(rows0) > 0 and len(best0) > 0
    for rows, best in ((rows1, best1), (rows2, best2)):
        assert len(rows) == len(rows0) and all((rows[f] == rows0[f]).all() for f in rows.dtype.names)
        assert best.tobytes() == best0.tobytes()
