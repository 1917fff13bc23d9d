"""GPU tests of the simulator's library kinds (mc_genome_set_library, csrc/k_simulate.h k_sim_walk): device bytes against the
numpy restatement, the exact invariants, the fused library pass against the pinned path, the ABI's refusals, and training end to
end with Illumina errors and with mate pairs."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import simlib_restated as sr
from microbecensus_amd import _native, training

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


def load_genomes():
    """[(name, bases, contig_off, contig names)] of the 30 genomes of tests/golden/genomes/genomes30.npz."""
    d = np.load(os.path.join(GOLD, "genomes", "genomes30.npz"))
    packed, off = d["packed"], d["contig_off"]
    codes = np.stack([(packed >> (2 * k)) & 3 for k in range(4)], axis=1).reshape(-1)[: off[-1]]
    allb = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    allb[d["exc_pos"]] = d["exc_chr"]
    out = []
    for g in range(int(d["genome_of"].max()) + 1):
        idx = np.nonzero(d["genome_of"] == g)[0]
        lo, hi = off[idx[0]], off[idx[-1] + 1]
        out.append(("g%02d" % g, allb[lo:hi].copy(), (off[idx[0]: idx[-1] + 2] - lo).astype(np.int64), [str(x) for x in d["names"][idx]]))
    return out


@pytest.fixture(scope="module")
def genomes():
    return load_genomes()


def write_fna(path, bases, off, names):
    with gzip.open(path, "wb", compresslevel=1) as f:
        for k, nm in enumerate(names):
            seq = bases[off[k]: off[k + 1]].tobytes()
            f.write(b">" + nm.encode() + b"\n")
            for j in range(0, len(seq), 80):
                f.write(seq[j: j + 80] + b"\n")


KINDS = [dict(error_model="illumina"), dict(error_model="uniform", error_rate=0.02), dict(error_model="uniform", error_rate=0.6),
         dict(paired_end=True, insert=400), dict(error_model="illumina", paired_end=True, insert=400)]


def test_device_bytes_equal_restatement(genomes, monkeypatch):
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")              # internal ranges of 1,000 reads
    cases = [("toy", *sr.toy_genome())] + [(name, bases, off) for name, bases, off, _ in genomes[:2]]
    for name, bases, off in cases:
        g = _native.Genome(bases, off, 0)
        try:
            for kind in KINDS:
                g.set_library(**kind)
                for L in (50, 150, 300):
                    if kind.get("insert", L) < L:
                        continue
                    lid = training.library_id(name, L)
                    got = g.simulate(L, 2600, 7, lid)
                    assert np.array_equal(got, sr.simulate(bases, off, L, 0, 2600, 7, lid, **kind)), (name, kind, L)
                    part = g.simulate(L, 1301, 7, lid, first=899)     # starts inside the first range (mid-pair), crosses the boundary at 1,000
                    assert np.array_equal(part, got[899:2200]), (name, kind, L)
            g.set_library()
            assert np.array_equal(g.simulate(150, 500, 7, 1), sr.simulate(bases, off, 150, 0, 500, 7, 1))
        finally:
            g.close()


def test_exact_invariants(genomes):
    name, bases, off, _ = genomes[4]
    g = _native.Genome(bases, off, 0)
    try:
        for L in (100, 150):
            lid = training.library_id(name, L)
            plain = g.simulate(L, 3000, 2, lid)
            g.set_library("uniform", 0.0)
            assert np.array_equal(g.simulate(L, 3000, 2, lid), plain)
            g.set_library(paired_end=True, insert=L)
            pe = g.simulate(L, 6000, 2, lid)
            assert np.array_equal(pe[0::2], plain)
            assert np.array_equal(pe[1::2], np.stack([sr.revcomp(r) for r in plain]))
            g.set_library()
            assert np.array_equal(g.simulate(L, 3000, 2, lid), plain)
    finally:
        g.close()


def _compare_library_pass(eng, g, n, seed, lid):
    got = eng.train_library(g, n, seed, lid, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)
    assert eng.stats()["reads"] == n
    eng.search(g.simulate(eng.read_len, n, seed, lid))
    want = eng.grid_classify(training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=0)
    assert got[0].sum() > 0
    return got


def test_train_library_equals_pinned_path(genomes, monkeypatch):
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")              # a library of 5,500 reads in six ranges
    name, bases, off, _ = genomes[3]
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(150)
        lid = training.library_id(name, 150)
        g.set_library("illumina")
        _compare_library_pass(eng, g, 5500, 11, lid)
        g.set_library("uniform", 0.01, paired_end=True, insert=320)
        _compare_library_pass(eng, g, 5500, 11, lid)
    finally:
        eng.close()
        g.close()


def test_errors_reach_the_search(genomes):
    """At the loosest grid cell an Illumina-error library classifies fewer reads than the error-free library of the same seed and id."""
    name, bases, off, _ = genomes[5]
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(150)
        lid = training.library_id(name, 150)
        n = training.library_reads(10, int(off[-1]), 150)
        plain = eng.train_library(g, n, 1, lid, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)[0][0, -1, 0].sum()
        g.set_library("illumina")
        err = eng.train_library(g, n, 1, lid, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)[0][0, -1, 0].sum()
        print("reads classified at the loosest cell, %d reads: error-free %d, illumina %d" % (n, plain, err))
        assert 0 < err < plain
    finally:
        eng.close()
        g.close()


def test_abi_refusals(genomes):
    name, bases, off, _ = genomes[0]
    lib = _native.load_library()
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    longest = int(np.max(np.diff(off)))
    try:
        for rec, msg in [((0, 0, 7, 0.0), "unknown error model 7"), ((0, 0, 1, 1.5), "outside [0, 1]"), ((0, 0, 1, float("nan")), "outside [0, 1]"),
                         ((1, 0, 0, 0.0), "positive insert"), ((1, longest + 1, 0, 0.0), "no contig of at least the insert")]:
            assert lib.mc_genome_set_library(g.g, C.byref(_native.McLibrary(*rec))) != 0
            assert msg in lib.mc_last_error().decode()
        g.set_library(paired_end=True, insert=120)
        with pytest.raises(RuntimeError, match=r"insert \(120\) is shorter than the read length \(150\)"):
            g.simulate(150, 10, 1, 1)
        eng.set_run(100)
        with pytest.raises(RuntimeError, match="even number of reads"):
            eng.train_library(g, 1001, 1, 1, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)
        assert lib.mc_genome_set_library(g.g, None) == 0
        assert g.simulate(150, 10, 1, 1).shape == (10, 150)
    finally:
        eng.close()
        g.close()


def _train(args, env):
    subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_microbe_census.py")] + [str(a) for a in args], check=True, env=env, timeout=900)


def test_train_end_to_end_with_illumina_errors(genomes, tmp_path):
    """24 genomes trained at 150 bp, 10x, Illumina errors; the 6 held out simulated with errors under another seed and estimated
    with --model."""
    train_dir, held_dir = tmp_path / "train", tmp_path / "held"
    train_dir.mkdir(); held_dir.mkdir()
    sizes = {}
    for k, (name, bases, off, names) in enumerate(genomes):
        write_fna(str((train_dir if k < 24 else held_dir) / (name + ".fna.gz")), bases, off, names)
        sizes[name] = int(off[-1])
    model_dir, held_out, reads_dir = tmp_path / "model", tmp_path / "held_model", tmp_path / "reads"
    env = dict(os.environ)
    env.pop("MC_STREAM_BATCH", None)
    _train([train_dir, model_dir, "-l", "150", "-c", "10", "--error-model", "illumina"], env)
    _train([held_dir, held_out, "-l", "150", "-c", "10", "-x", "3", "--seed", "1", "--error-model", "illumina", "--write-reads", reads_dir], env)
    import json
    assert json.loads((model_dir / "model.json").read_text())["library"] == {"error_model": "illumina", "error_rate": None, "paired_end": False, "insert": None}
    errs = []
    for name in sorted(n for n in sizes if (held_dir / (n + ".fna.gz")).exists()):
        out = tmp_path / (name + ".txt")
        subprocess.run([sys.executable, os.path.join(REPO, "scripts", "run_microbe_census.py"), "--model", str(model_dir), "-l", "150", "-n", "100000000", "-e", "-g", "0",
                        str(reads_dir / "150" / (name + "-reads.fa")), str(out)], check=True, env=env, timeout=900)
        ags = float([ln.split("\t")[1] for ln in out.read_text().splitlines() if ln.startswith("average_genome_size:")][0])
        errs.append(abs(ags - sizes[name]) / sizes[name])
    med = float(np.median(errs))
    print("held-out AGS relative errors with Illumina errors %s; median %.4f" % (["%.4f" % e for e in errs], med))
    assert med <= 0.15


def test_train_paired_end(genomes, tmp_path):
    gdir = tmp_path / "genomes"
    gdir.mkdir()
    for name, bases, off, names in genomes[:6]:
        write_fna(str(gdir / (name + ".fna.gz")), bases, off, names)
    env = dict(os.environ)
    env.pop("MC_STREAM_BATCH", None)
    _train([gdir, tmp_path / "model", "-l", "150", "-c", "2", "-x", "3", "--paired-end", "--insert", "300", "--write-reads", tmp_path / "reads"], env)
    for name, bases, off, _ in genomes[:6]:
        lines = (tmp_path / "reads" / "150" / (name + "-reads.fa")).read_bytes().split(b"\n")
        heads, seqs = lines[0:-1:2], lines[1::2]
        pairs = training.library_reads(2, int(off[-1]), 150)
        assert len(heads) == 2 * pairs
        assert heads[:4] == [b">0/1", b">0/2", b">1/1", b">1/2"] and heads[-1] == b">%d/2" % (pairs - 1)
        assert all(len(s) == 150 for s in seqs)
        want = sr.simulate(bases, off, 150, 0, 2 * pairs, 0, training.library_id(name, 150), paired_end=True, insert=300)
        assert b"".join(seqs) == want.tobytes()
