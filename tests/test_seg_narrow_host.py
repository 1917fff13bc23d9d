"""The one-word form of the SEG masking - mc_seg_mask_fx2<McBits64> of csrc/mc_core.h, what a lane of the narrow k_translate_seg restates
for frames of at most 63 residues - against the same function with McBits192 and against the oracle's rs_translate6(), byte for byte,
at EVERY read length of the narrow range (18 ... 191 bp), on a dense set (periodic, mosaic and long-stretch reads: nearly every frame has
something to mask) and a sparse one (one periodic read in ten among reads the oracle masks nothing on) of tests/seg_cases.py.  No GPU:
tests/emul/seg_narrow.cpp is built with g++.

The narrow form's work list has four entries (63 / 13, the bound written at MC_SEG_STK); seg_narrow gives it an array of exactly four and
counts the pushes that find it full: there must be none.  The McBits64 primitives are held to McBits192 on their own (seg_narrow
primitives): next and prev from every position on sets over every n <= 63 - the empty set, bit 0, bit 62 and both among them -, every
range up to (0, 62), shifts by 0 ... 63, and the flags of every segment of a frame."""
import os
import re
import subprocess

import numpy as np
import pytest

import seg_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "seg_narrow.cpp")
LENGTHS = list(range(18, 192))
N_DENSE, N_SPARSE = 60, 50


@pytest.fixture(scope="module")
def seg_narrow(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_narrow") / "seg_narrow")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def seg_narrow_asan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_narrow_asan") / "seg_narrow_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def oracle_lib():
    port = os.path.join(sc.REPO, "oracle", "librapsearch_port.so")
    src = os.path.join(sc.REPO, "oracle", "rapsearch_port.c")
    if not os.path.exists(port) or os.path.getmtime(port) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", os.path.join(sc.REPO, "oracle"), "librapsearch_port.so"])
    return sc.oracle_lib()


def dense_set(L, n):
    return sc.make_reads(L, n, seed=7, families=("periodic", "mosaic", "long"), dirty=False, with_witness=False)


def run_frames(exe, reads, tmp):
    """seg_narrow frames on the reads: ((n, 2, 6, MC_FP) frames - form 0 McBits192, 1 McBits64 -, pushes onto a full list per form, stderr)."""
    n, L = reads.shape
    reads.tofile(str(tmp / "reads.bin"))
    p = subprocess.run([exe, "frames", str(tmp / "reads.bin"), str(L), str(tmp / "frames.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.stdout, p.stderr[-3000:])
    m = re.match(r"reads (\d+) frames (\d+) full_list_pushes (\d+) (\d+)", p.stdout)
    assert m and int(m.group(1)) == n and int(m.group(2)) == 6 * n, p.stdout
    return np.fromfile(str(tmp / "frames.bin"), np.uint8).reshape(n, 2, 6, sc.MC_FP), (int(m.group(3)), int(m.group(4))), p.stderr


def check_lengths(exe, kind, lengths, tmp):
    masked = 0
    for L in lengths:
        reads = dense_set(L, N_DENSE) if kind == "dense" else sc.sparse_set(L, N_SPARSE, seed=7)
        want, lens = sc.oracle_frames(reads)
        got, full, err = run_frames(exe, reads, tmp)
        assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
        for f in range(6):
            assert (want[:, f, lens[f]:] == sc.MC_INV).all()
        assert np.array_equal(got[:, 1], got[:, 0]), "L %d, %s: McBits64 differs from McBits192" % (L, kind)
        assert np.array_equal(got[:, 1], want), "L %d, %s: McBits64 differs from the oracle" % (L, kind)
        assert full == (0, 0), "L %d, %s: pushes onto a full work list %s" % (L, kind, full)
        masked += int(sc.masked_by_oracle(reads, want).sum())
    return masked


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_narrow_form_equals_wide_form_and_oracle_at_every_length(kind, seg_narrow, oracle_lib, tmp_path):
    masked = check_lengths(seg_narrow, kind, LENGTHS, tmp_path)
    print("%s: %d lengths, %d reads each, %d residues masked by the oracle in all" % (kind, len(LENGTHS), N_DENSE if kind == "dense" else N_SPARSE, masked))
    assert masked > 1000 * (10 if kind == "dense" else 1)           # the sets give SEG something to do


def test_the_dense_set_fills_the_frames(oracle_lib):
    """At 189 - 191 bp (frames of 62 and 63 residues) nearly every frame of the dense set has a masked residue, and some frame is masked
    up to its last residue: positions 61 and 62 of the one-word sets are used."""
    for L in (189, 190, 191):
        reads = dense_set(L, N_DENSE)
        want, lens = sc.oracle_frames(reads)
        m = sc.masked_by_oracle(reads, want)
        assert m.any(2).mean() > 0.9
        assert any(m[:, f, lens[f] - 1].any() for f in range(6))
    assert max(lens) == 63


def test_mask_primitives_against_the_wide_form(seg_narrow):
    p = subprocess.run([seg_narrow, "primitives"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    m = re.match(r"primitives (\d+) mismatches (\d+)", p.stdout)
    assert p.returncode == 0 and m and int(m.group(1)) > 1000000 and int(m.group(2)) == 0, (p.stdout, p.stderr[-3000:])


def test_narrow_form_under_sanitizers(seg_narrow_asan, oracle_lib, tmp_path):
    """seg_narrow built with AddressSanitizer + UBSan, run as itself: the primitives (a shift by 64 is a runtime error there), and the
    frames at the lengths where the form changes a path - the four-entry work list is an array of exactly four."""
    p = subprocess.run([seg_narrow_asan, "primitives"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout, p.stderr[-3000:])
    assert re.match(r"primitives \d+ mismatches 0", p.stdout), p.stdout
    check_lengths(seg_narrow_asan, "dense", [18, 33, 36, 100, 150, 186, 188, 189, 190, 191], tmp_path)
    check_lengths(seg_narrow_asan, "sparse", [150, 191], tmp_path)
