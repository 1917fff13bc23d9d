"""Library kinds of the training simulator on the CPU: the generator the device runs (csrc/mc_simlib.h, compiled with g++ into
tests/emul/sim_library.cpp) against its numpy restatement (simlib_restated.py), the statistics of the restated error process
against sim_functions.py's probabilities, and the refusals of a training run with a library kind."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import simlib_restated as sr
from microbecensus_amd import _native, training

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("simlib") / "sim_library")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(HERE, "emul", "sim_library.cpp")])
    return exe


def run_driver(exe, tmp_path, bases, off, L, first, n, seed, lib, error_model=None, error_rate=None, paired_end=False, insert=None):
    bf, of, out = tmp_path / "bases.bin", tmp_path / "off.bin", tmp_path / "out.bin"
    bf.write_bytes(np.asarray(bases, np.uint8).tobytes())
    of.write_bytes(np.asarray(off, np.int64).tobytes())
    subprocess.check_call([exe, str(bf), str(of), str(L), str(int(paired_end)), str(insert or 0), str(sr.MODELS[error_model]), repr(float(error_rate or 0.0)),
                           str(seed), str(lib), str(first), str(n), str(out)])
    return np.frombuffer(out.read_bytes(), dtype=np.uint8).reshape(n, L)


def fixture_genome(k=0):
    d = np.load(os.path.join(HERE, "golden", "genomes", "genomes30.npz"))
    packed, off = d["packed"], d["contig_off"]
    idx = np.nonzero(d["genome_of"] == k)[0]
    lo, hi = int(off[idx[0]]), int(off[idx[-1] + 1])
    codes = np.stack([(packed >> (2 * q)) & 3 for q in range(4)], axis=1).reshape(-1)[lo:hi]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    exc = (d["exc_pos"] >= lo) & (d["exc_pos"] < hi)
    bases[d["exc_pos"][exc] - lo] = d["exc_chr"][exc]
    return bases, (off[idx[0]: idx[-1] + 2] - lo).astype(np.int64)


KINDS = [
    dict(error_model="illumina"),
    dict(error_model="uniform", error_rate=0.05),
    dict(error_model="uniform", error_rate=0.6),              # many deletions: refused ones near the contigs' ends
    dict(error_model="uniform", error_rate=1.0),
    dict(paired_end=True, insert=300),
    dict(error_model="illumina", paired_end=True, insert=300),
    dict(error_model="uniform", error_rate=0.3, paired_end=True, insert=150),
]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "-".join("%s" % v for v in k.values()))
def test_generator_matches_restatement(driver, tmp_path, kind):
    bases, off = sr.toy_genome()
    for L in (50, 150):
        want = sr.simulate(bases, off, L, 0, 3000, 9, 77, **kind)
        got = run_driver(driver, tmp_path, bases, off, L, 0, 3000, 9, 77, **kind)
        assert np.array_equal(got, want)
        part = run_driver(driver, tmp_path, bases, off, L, 1001, 999, 9, 77, **kind)      # an odd start: a range may split a pair
        assert np.array_equal(part, want[1001:2000])


def test_generator_on_a_fixture_genome(driver, tmp_path):
    bases, off = fixture_genome(2)
    for L, kind in ((100, dict(error_model="illumina")), (300, dict(error_model="illumina", paired_end=True, insert=500))):
        want = sr.simulate(bases, off, L, 5000, 4000, 3, training.library_id("g02", L), **kind)
        assert np.array_equal(run_driver(driver, tmp_path, bases, off, L, 5000, 4000, 3, training.library_id("g02", L), **kind), want)


def test_exact_invariants():
    bases, off = sr.toy_genome()
    L = 120
    lens = np.diff(off)
    vstart = np.concatenate([[0], np.cumsum(np.maximum(0, lens - L + 1))])
    key = sr.mix64(4 ^ sr.mix64(8))
    u = np.array([sr.mix64((key + i) & sr.MASK) % int(vstart[-1]) for i in range(500)])
    c = np.searchsorted(vstart, u, side="right") - 1
    single = bases[(off[c] + u - vstart[c])[:, None] + np.arange(L)[None, :]]              # k_simulate.h's default library
    assert np.array_equal(sr.simulate(bases, off, L, 0, 500, 4, 8), single)
    assert np.array_equal(sr.simulate(bases, off, L, 0, 500, 4, 8, error_model="uniform", error_rate=0.0), single)
    pe = sr.simulate(bases, off, L, 0, 1000, 4, 8, paired_end=True, insert=L)
    assert np.array_equal(pe[0::2], single)
    assert np.array_equal(pe[1::2], np.stack([sr.revcomp(r) for r in single]))
    # an error model never moves a start: the paired-end mates of a longer insert still pair up
    pe3 = sr.simulate(bases, off, L, 0, 1000, 4, 8, paired_end=True, insert=300)
    pe3e = sr.simulate(bases, off, L, 0, 1000, 4, 8, paired_end=True, insert=300, error_model="illumina")
    assert np.mean(np.all(pe3[:, :20] == pe3e[:, :20], axis=1)) > 0.99
    assert not np.array_equal(pe3, pe3e)


def test_reverse_complement_keeps_case_and_other_bytes():
    assert sr.revcomp(np.frombuffer(b"ACGTacgtNRn-", np.uint8)).tobytes() == b"-nRNacgtACGT"


def _z_ok(k, n, p, z=5.0):
    return abs(k - n * p) <= z * np.sqrt(max(n * p * (1 - p), 1e-300)) + 1


def test_error_statistics():
    """About 200 k reads of the restatement: per-position error rates, the 0.8 / 0.1 / 0.1 split, uniform bases."""
    rng_bases = np.random.default_rng(11).integers(0, 4, 4_000_000)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng_bases]
    off = np.array([0, 1_500_000, 4_000_000], dtype=np.int64)
    log = []
    sr.simulate(bases, off, 150, 0, 200_000, 1, 2, error_model="illumina", log=log)
    for j, e, _ in log:
        if j >= 150:
            break
        p = min(1.0, sr.p_error("illumina", None, j))
        assert _z_ok(int(np.count_nonzero(e)), len(e), p), j
    tail = sum(int(np.count_nonzero(e)) for j, e, _ in log if j >= 120)
    assert tail > 0
    log = []
    sr.simulate(bases, off, 100, 0, 200_000, 3, 4, error_model="uniform", error_rate=0.05, log=log)
    n_base = sum(len(e) for _, e, _ in log)
    ev = np.concatenate([e for _, e, _ in log])
    xs = np.concatenate([x[e > 0] for _, e, x in log])
    n_err = int(np.count_nonzero(ev))
    assert _z_ok(n_err, n_base, 0.05)
    for code, p in ((1, 0.8), (2, 0.1)):
        assert _z_ok(int(np.count_nonzero(ev == code)), n_err, p), code
    assert _z_ok(int(np.count_nonzero((ev == 3) | (ev == 4))), n_err, 0.1)
    for b in b"ACGT":
        assert _z_ok(int(np.count_nonzero(xs == b)), len(xs), 0.25), chr(b)
    # a uniform rate of 1: every consumed base is an error
    log = []
    sr.simulate(bases, off, 60, 0, 2000, 5, 6, error_model="uniform", error_rate=1.0, log=log)
    assert all(np.all(e > 0) for _, e, _ in log)


def test_thresholds():
    thr = sr.thresholds("illumina", None)
    assert thr[233] < 1 << 32 and thr[234] == 1 << 32
    assert thr[0] == int((3e-3 + 3.3e-8) / 100 * 2 ** 32) == 128850
    assert sr.thresholds("uniform", 0.0) == [0] * sr.NTHR and sr.thresholds("uniform", 1.0) == [1 << 32] * sr.NTHR
    # the kind cut points: within 2^-16 of 0.8 and 0.9
    assert abs(sr.SUB / 65536 - 0.8) < 2 ** -16 and abs(sr.INS / 65536 - 0.9) < 2 ** -16


# ---- the training run: refusals, model record, reads file ---------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was opened")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Genome", boom)


def _genome_dir(tmp_path, n, contig=500):
    d = tmp_path / "genomes"
    d.mkdir(exist_ok=True)
    for i in range(n):
        with gzip.open(d / ("g%d.fna.gz" % i), "wt") as f:
            f.write(">c\n%s\n" % ("ACGT" * (contig // 4)))
    return str(d)


REFUSED = [
    (dict(error_model="uniform"), "needs an error rate"),
    (dict(error_rate=0.01), "only with the uniform error model"),
    (dict(error_model="illumina", error_rate=0.01), "only with the uniform error model"),
    (dict(error_model="uniform", error_rate=1.5), r"outside \[0, 1\]"),
    (dict(error_model="sanger"), "unknown error model"),
    (dict(paired_end=True), "needs an insert"),
    (dict(insert=300), "only with a paired-end library"),
    (dict(paired_end=True, insert=120), "insert 120 is shorter than the read length 150"),
    (dict(paired_end=True, insert=600), "no contig of at least 600 bp"),
]


@pytest.mark.parametrize("kw,msg", REFUSED, ids=[m for _, m in REFUSED])
def test_library_refusals(tmp_path, no_engine, kw, msg):
    gd = _genome_dir(tmp_path, 3)
    out = str(tmp_path / "out")
    with pytest.raises(training.TrainingError, match=msg):
        training.train(gd, out, [100, 150], 10, xfolds=2, **kw)
    assert not os.path.exists(out)


@pytest.mark.parametrize("args,msg", [(["--error-model", "uniform"], "needs an error rate (--error-rate)"),
                                      (["--error-rate", "0.1"], "only with the uniform error model"),
                                      (["--paired-end"], "needs an insert (--insert)"),
                                      (["--paired-end", "--insert", "100"], "insert 100 is shorter than the read length 150")])
def test_cli_library_refusals(tmp_path, args, msg):
    gd = _genome_dir(tmp_path, 2)
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_microbe_census.py"), gd, str(tmp_path / "o"), "-l", "150", "-c", "10", "-x", "2"] + args,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and msg in r.stderr, r.stderr
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_microbe_census.py"), gd, str(tmp_path / "o"), "-l", "150", "-c", "10", "--error-model", "sanger"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "invalid choice" in r.stderr


def test_model_library_record(tmp_path):
    names, seqs = ["m0", "m1"], ["MKV", "MKL"]
    args = (names, seqs, [0, 0], ["BA1"], [150], {"150": {"BA1": [0.0, 100.0, 23.0, "hits"]}}, {"150_BA1": 5.0}, {"150_BA1": 1.0})
    training.write_model(str(tmp_path / "a"), *args)
    training.write_model(str(tmp_path / "b"), *args, library=training.library_record())
    assert (tmp_path / "a" / "model.json").read_bytes() == (tmp_path / "b" / "model.json").read_bytes()
    assert "library" not in json.loads((tmp_path / "a" / "model.json").read_text())
    rec = training.library_record("illumina", None, True, 300)
    training.write_model(str(tmp_path / "c"), *args, library=rec)
    m = json.loads((tmp_path / "c" / "model.json").read_text())
    assert m["library"] == {"error_model": "illumina", "error_rate": None, "paired_end": True, "insert": 300}
    assert training.library_record("uniform", 0.01) == {"error_model": "uniform", "error_rate": 0.01, "paired_end": False, "insert": None}


def test_paired_reads_file(tmp_path):
    reads = np.frombuffer(b"AAAACCCCGGGGTTTT", np.uint8).reshape(4, 4)
    training.write_reads(str(tmp_path / "r" / "pe.fa"), reads, paired_end=True)
    assert (tmp_path / "r" / "pe.fa").read_bytes() == b">0/1\nAAAA\n>0/2\nCCCC\n>1/1\nGGGG\n>1/2\nTTTT\n"
    training.write_reads(str(tmp_path / "r" / "se.fa"), reads)
    assert (tmp_path / "r" / "se.fa").read_bytes().startswith(b">0\nAAAA\n>1\nCCCC\n")
