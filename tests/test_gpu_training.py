"""GPU tests of the training workflow: the device library simulator against its numpy restatement, the fused library pass
(mc_train_library) against the pinned path on the same reads, the --model plumbing of run_pipeline, and training end to end."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from microbecensus_amd import _native, training
from microbecensus_amd import microbe_census as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
MASK = (1 << 64) - 1


# ---- the simulator restated (csrc/k_simulate.h) ---------------------------------------------------------------------------------
def mix64(z):
    z = (int(z) + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def simulate_np(bases, off, L, first, n, seed, lib):
    lens = np.diff(off)
    vstart = np.zeros(len(lens) + 1, dtype=np.int64)
    vstart[1:] = np.cumsum(np.maximum(0, lens - L + 1))
    total = int(vstart[-1])
    key = mix64(seed ^ mix64(lib))
    u = np.array([mix64((key + i) & MASK) % total for i in range(first, first + n)], dtype=np.int64)
    c = np.searchsorted(vstart, u, side="right") - 1
    s = off[c] + (u - vstart[c])
    return bases[s[:, None] + np.arange(L)[None, :]]


def load_genomes():
    """[(name, bases, contig_off)] of the 30 genomes of tests/golden/genomes/genomes30.npz."""
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


def test_simulate_matches_numpy(genomes, monkeypatch):
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")              # internal ranges of 1,000 reads
    for name, bases, off, _ in genomes[:2]:
        g = _native.Genome(bases, off, 0)
        try:
            for L in (50, 150, 500):
                lid = training.library_id(name, L)
                got = g.simulate(L, 2600, 7, lid)
                assert np.array_equal(got, simulate_np(bases, off, L, 0, 2600, 7, lid))
                part = g.simulate(L, 1300, 7, lid, first=900)      # starts inside the first range, crosses the boundary at 1,000
                assert np.array_equal(part, got[900:2200])
        finally:
            g.close()


def _pinned_path(eng, g, n, seed, lid):
    reads = g.simulate(eng.read_len, n, seed, lid)
    eng.search(reads)
    return eng.grid_classify(training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)


def _compare_library_pass(eng, g, n, seed, lid):
    got = eng.train_library(g, n, seed, lid, training.ALN_COVS, training.MAX_PIDS, training.MIN_SCORES)
    assert eng.stats()["reads"] == n
    want = _pinned_path(eng, g, n, seed, lid)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=0)
    assert got[0].sum() > 0


def test_train_library_equals_pinned_path(genomes, monkeypatch, tmp_path):
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")              # a library of 5,500 reads in six ranges
    name, bases, off, _ = genomes[3]
    g = _native.Genome(bases, off, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(150)
        _compare_library_pass(eng, g, 5500, 11, training.library_id(name, 150))
    finally:
        eng.close()
    # a 3-family custom marker set, built the way --gene-fams builds it
    names, seqs = _native.load_markers()
    model = _native.load_model()
    fams = model["families"][:3]
    for fi, fam in enumerate(fams):
        with gzip.open(tmp_path / (fam + ".faa.gz"), "wt") as f:
            for nm, sq, mf in zip(names, seqs, model["marker_family"]):
                if mf == fi:
                    f.write(">%s\n%s\n" % (nm, sq))
    cn, cs, cf, cfam = training.build_marker_set(training.list_families(str(tmp_path)))
    assert cfam == fams
    eng = _native.Engine(device=0, names=cn, seqs=cs, marker_family=cf, nfam=3)
    try:
        eng.set_run(100)
        _compare_library_pass(eng, g, 4200, 3, training.library_id(name, 100))
    finally:
        eng.close()
        g.close()


def _model_copy_doubled(dst):
    os.makedirs(dst, exist_ok=True)
    shutil.copy(os.path.join(_native.DATA_DIR, "markers.faa.gz"), dst)
    m = _native.load_model()
    m["coefficients"] = {k: v * 2 for k, v in m["coefficients"].items()}
    with open(os.path.join(dst, "model.json"), "w") as f:
        json.dump(m, f)


def test_model_dir_scales_ags(tmp_path):
    d = str(tmp_path / "model")
    _model_copy_doubled(d)
    fq = os.path.join(GOLD, "inputs", "example.fq.gz")
    base = {"seqfiles": [fq], "nreads": 100000}
    est0, _ = mc.run_pipeline(dict(base))
    est_m, _ = mc.run_pipeline(dict(base, model_dir=d))
    assert est_m == 2 * est0
    est_k0, _ = mc.run_pipeline(dict(base, keep_tmp=True))
    est_k, _ = mc.run_pipeline(dict(base, keep_tmp=True, model_dir=d))
    assert est_k == 2 * est_k0
    est_again, _ = mc.run_pipeline(dict(base))               # the default model after a trained one, same process
    assert est_again == est0


def test_train_end_to_end(genomes, tmp_path):
    """24 genomes trained at 150 bp, 10x; the 6 held out simulated with another seed and estimated with --model."""
    train_dir, held_dir = tmp_path / "train", tmp_path / "held"
    train_dir.mkdir(); held_dir.mkdir()
    sizes = {}
    for k, (name, bases, off, names) in enumerate(genomes):
        write_fna(str((train_dir if k < 24 else held_dir) / (name + ".fna.gz")), bases, off, names)
        sizes[name] = int(off[-1])
    model_dir, held_out, reads_dir = tmp_path / "model", tmp_path / "held_model", tmp_path / "reads"
    env = dict(os.environ)
    env.pop("MC_STREAM_BATCH", None)
    subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_microbe_census.py"), str(train_dir), str(model_dir), "-l", "150", "-c", "10"],
                   check=True, env=env, timeout=900)
    subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_microbe_census.py"), str(held_dir), str(held_out), "-l", "150", "-c", "10",
                    "-x", "3", "--seed", "1", "--write-reads", str(reads_dir)], check=True, env=env, timeout=900)
    errs = []
    for name in sorted(n for n in sizes if (held_dir / (n + ".fna.gz")).exists()):
        out = tmp_path / (name + ".txt")
        subprocess.run([sys.executable, os.path.join(REPO, "scripts", "run_microbe_census.py"), "--model", str(model_dir), "-l", "150", "-n", "100000000", "-e", "-g", "0",
                        str(reads_dir / "150" / (name + "-reads.fa")), str(out)], check=True, env=env, timeout=900)
        ags = float([ln.split("\t")[1] for ln in out.read_text().splitlines() if ln.startswith("average_genome_size:")][0])
        errs.append(abs(ags - sizes[name]) / sizes[name])
    med = float(np.median(errs))
    print("held-out AGS relative errors %s; median %.4f" % (["%.4f" % e for e in errs], med))
    assert med <= 0.15
    # training_preds.map = coefficient / rate, from the held-out run's own rates (its .hits tables)
    pars = {(r[1], r[0]): r for r in training.read_map(str(held_out / "pars.map"), header=True)}
    coeff = {r[0]: float(r[1]) for r in training.read_map(str(held_out / "coefficients.map"))}
    nrows = 0
    for L, fam, genome, true, est in training.read_map(str(held_out / "training_preds.map"), header=True):
        assert int(true) == sizes[genome]
        _, _, cov, pid, score, stat = pars[(L, fam)]
        n = training.library_reads(10.0, sizes[genome], int(L))
        rec = [r for r in training.read_map(str(reads_dir / L / (genome + ".hits")), header=True)
               if r[0] == fam and float(r[1]) == float(cov) and float(r[2]) == float(pid) and float(r[3]) == float(score)]
        assert len(rec) == 1
        count = float(rec[0][{"hits": 4, "aln": 5, "cov": 6}[stat]])
        rate = count / (n * int(L))
        if rate == 0:
            assert est == "NA"
        else:
            assert float(est) == coeff["%s_%s" % (L, fam)] / rate
        nrows += 1
    assert nrows == 6 * 30
