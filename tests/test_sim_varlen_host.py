"""The simulator's reference read-length mode on the CPU (no GPU): the generator the device runs (csrc/mc_simlib.h, mc_sim_walk_ref,
compiled with g++ into tests/emul/sim_library_varlen.cpp) against its Python restatement (simlib_varlen_restated.py), byte for byte;
every read is L + insertions - deletions bases long; under error model none the mode gives the default mode's reads."""
import os
import subprocess

import numpy as np
import pytest

import simlib_restated as sr
import simlib_varlen_restated as svr

HERE = os.path.dirname(os.path.abspath(__file__))

KINDS = [dict(), dict(error_model="illumina"), dict(error_model="uniform", error_rate=0.05), dict(error_model="uniform", error_rate=0.3),
         dict(error_model="illumina", paired_end=True, insert=260), dict(paired_end=True, insert=200)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("simvl") / "sim_library_varlen")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(HERE, "emul", "sim_library_varlen.cpp")])
    return exe


def run_driver(exe, tmp_path, bases, off, L, first, n, seed, lib, error_model=None, error_rate=None, paired_end=False, insert=None):
    bf, of, out, oo = tmp_path / "bases.bin", tmp_path / "off.bin", tmp_path / "out.bin", tmp_path / "offs.bin"
    bf.write_bytes(np.asarray(bases, np.uint8).tobytes())
    of.write_bytes(np.asarray(off, np.int64).tobytes())
    subprocess.check_call([exe, str(bf), str(of), str(L), "1" if paired_end else "0", str(insert or 0), str(sr.MODELS[error_model]), repr(float(error_rate or 0.0)),
                           str(seed), str(lib), str(first), str(n), str(out), str(oo)])
    return np.fromfile(out, np.uint8), np.fromfile(oo, np.int64)


@pytest.mark.parametrize("k", range(len(KINDS)))
def test_generator_equals_restatement(driver, tmp_path, k):
    kind = KINDS[k]
    bases, off = sr.toy_genome()
    L = 150
    got_b, got_o = run_driver(driver, tmp_path, bases, off, L, 17, 600, 99, 12345, **kind)
    want_b, want_o, events = svr.simulate_varlen(bases, off, L, 17, 600, 99, 12345, **kind)
    assert (got_o == want_o).all() and got_b.tobytes() == want_b.tobytes()
    lens = np.diff(want_o)
    assert (lens == np.array([L + i - d for i, d in events])).all()
    assert got_o[0] == 0 and got_o[-1] == len(got_b) == lens.sum()
    if kind.get("error_model"):
        assert (lens != L).any()


@pytest.mark.parametrize("k", [0, 5])
def test_no_errors_gives_the_default_reads(k):
    bases, off = sr.toy_genome()
    L = 120
    b, o, _ = svr.simulate_varlen(bases, off, L, 0, 300, 7, 99, **KINDS[k])
    fixed = sr.simulate(bases, off, L, 0, 300, 7, 99, **KINDS[k])
    assert (np.diff(o) == L).all() and b.tobytes() == fixed.tobytes()
