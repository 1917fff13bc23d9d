"""Translation + SEG masking of the four per-frame forms of csrc/mc_core.h - mc_seg_mask (plain), mc_seg_mask_ws, mc_seg_mask_fx and
mc_seg_mask_fx2 (what a lane of k_translate_seg restates) - against the oracle's rs_translate6(), byte for byte, on reads built for
SEG's corners (tests/seg_cases.py) at every read length where the code takes another path.  No GPU: tests/emul/seg_forms.cpp is
built with g++ and runs the forms without the marker index; the oracle is called through ctypes (seg_cases.oracle_frames, which
states the map between the oracle's residue codes and the dense ones; 0xA0 is MC_INV).

The forms keep Seg::segseq's recursion as a work list.  Before its bound (MC_SEG_STK in mc_core.h) the list held eight entries
(sixteen in the plain form), remainders shorter than the window included, and a push onto a full list was dropped silently: on these
sets the three kernel-side forms then differed from the oracle in 5 frames of 143,400 each (508, 509 and 510 bp), the witness read
among them, and the plain form in none; on periodic reads alone, 600 per length, the first difference came at 412 bp.
seg_forms counts a push onto a full list; the count must be 0."""
import os
import re
import subprocess

import numpy as np
import pytest

import seg_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("mc_seg_mask", "mc_seg_mask_ws", "mc_seg_mask_fx", "mc_seg_mask_fx2")
# every L from 18 to 60 (frames under 8 residues get no SEG, 8 - 11 residues W = 8, from 12 on W = 12), and the neighbourhoods of
# the lengths the product is run at; 340 is the first length with a frame over 101 residues (Seg::trim's minlen = n - 100)
LENGTHS = list(range(18, 61)) + [99, 100, 101, 149, 150, 151, 249, 250, 251, 252, 299, 300, 301, 340, 341, 342, 508, 509, 510]


def set_size(L):
    return 300 if L <= 60 else 500 if L < 500 else 1000


@pytest.fixture(scope="module")
def seg_forms(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_forms") / "seg_forms")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "emul", "seg_forms.cpp")])
    return exe


@pytest.fixture(scope="module")
def oracle_lib():
    port = os.path.join(sc.REPO, "oracle", "librapsearch_port.so")
    src = os.path.join(sc.REPO, "oracle", "rapsearch_port.c")
    if not os.path.exists(port) or os.path.getmtime(port) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", os.path.join(sc.REPO, "oracle"), "librapsearch_port.so"])
    return sc.oracle_lib()


def run_forms(exe, reads, tmp):
    """Starts seg_forms on the reads; finish() returns ((n, 4, 6, MC_FP) frames, pushes onto a full list)."""
    n, L = reads.shape
    reads.tofile(str(tmp / "reads.bin"))
    p = subprocess.Popen([exe, str(tmp / "reads.bin"), str(L), str(tmp / "forms.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def finish():
        out, err = p.communicate()
        assert p.returncode == 0, (out, err[-3000:])
        m = re.match(r"reads (\d+) frames (\d+) full_list_pushes (\d+)", out)
        assert m and int(m.group(1)) == n and int(m.group(2)) == 6 * n, out
        return np.fromfile(str(tmp / "forms.bin"), np.uint8).reshape(n, 4, 6, sc.MC_FP), int(m.group(3)), err
    return finish


@pytest.mark.parametrize("L", LENGTHS)
def test_forms_equal_the_oracle(L, seg_forms, oracle_lib, tmp_path):
    """All four forms == rs_translate6() on every frame of the set (no frame is left out: the rows are compared whole, MC_INV behind
    each frame's length included), and no push found the work list full."""
    n = set_size(L)
    reads = sc.make_reads(L, n, seed=1)
    finish = run_forms(seg_forms, reads, tmp_path)                   # (runs beside the oracle's loop)
    want, lens = sc.oracle_frames(reads)
    share, ten, big, mid = sc.check_conditions(L, reads, want, lens)
    got, full, _ = finish()
    bad = {FORMS[k]: int((got[:, k] != want).any(2).sum()) for k in range(4)}
    print("L %d: %d frames per form; masked share %.3f, frames with >= 10 blocks %.3f, with a block > 100: %d, of 16-100: %d; differing frames %s; pushes onto a full list %d"
          % (L, 6 * n, share, ten, big, mid, bad, full))
    for f in range(6):
        assert (want[:, f, lens[f]:] == sc.MC_INV).all()
    assert not any(bad.values()), bad
    assert full == 0


def test_the_witness_frame(seg_forms, oracle_lib, tmp_path):
    """The read that first showed a dropped remainder, alone: frame 1's last masked block is 28 residues long in every form (the
    eight-entry list masked only its right 19)."""
    reads = sc.witness(510).reshape(1, 510)
    want, lens = sc.oracle_frames(reads)
    got, full, _ = run_forms(seg_forms, reads, tmp_path)()
    plain = sc.translate6(reads)
    f = sc.WITNESS_FRAME
    assert bytes(plain[0, f, :169]) == bytes(["ARNDCQEGHILKMFPSTWYV".index(a) for a in sc.WITNESS_PROTEIN])
    assert sc.blocks_of(want[0, f, :lens[f]] == sc.MC_INV)[-1] == 28
    for k, name in enumerate(FORMS):
        assert np.array_equal(got[0, k], want[0]), name
    assert full == 0


def test_forms_under_sanitizers(oracle_lib, tmp_path):
    """seg_forms built with AddressSanitizer + UBSan, run as itself on the 510-bp set (the work list is an array indexed by the
    number of entries): clean, and still the oracle's frames."""
    exe = str(tmp_path / "seg_forms_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(HERE, "emul", "seg_forms.cpp")])
    reads = sc.make_reads(510, 600, seed=1)
    finish = run_forms(exe, reads, tmp_path)
    want, _ = sc.oracle_frames(reads)
    got, full, err = finish()
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert np.array_equal(got, np.repeat(want[:, None], 4, 1)) and full == 0


def test_the_switch_points_of_the_launch():
    """seg_cases.launch_stages_reads restates the launch's choice between the two forms of k_translate_seg; these are its switches,
    which tests/test_gpu_translate_seg.py runs on both sides - and there the restatement is held to what the launch reports."""
    f = sc.launch_stages_reads
    assert [L for L in range(19, 511) if f(L) != f(L - 1)] == sc.SWITCHES
    assert f(18) and f(188) and not f(189) and f(238) and not f(510)
