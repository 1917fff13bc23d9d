"""k_translate_seg itself - six-frame translation and the wave-wide SEG (mc_seg_wave, csrc/k_translate_seg.h) - against the oracle's
rs_translate6(), byte for byte, on reads built for SEG's corners (tests/seg_cases.py).  The frames are read back with
Engine.set_run(L), upload, run_range(0, n) and debug_stage(0); every frame of every read is compared up to its length, and
everything behind the length must be MC_INV.  The CPU emulation has no part in this comparison: mc_seg_wave numbers the windows of
all pending stretches of a wave, finds an item's place with a sqrtf guess, chooses run lengths of 1, 2, 4 or 8 per batch and
reduces with LDS atomics - it has no CPU form.

MC_TS_STAGED (the form of the kernel: reads staged in LDS, or read from global memory) is read once per process, so every case runs
in a child process of its own, one after the other, each under `timeout -k 10` with its own limit.  A child that ends by a signal,
at its limit or with an error (a HIP error raises in the worker) fails its test with its output, and every later case of the
module then fails at once without starting anything on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_cases as sc

pytestmark = pytest.mark.gpu
REPO = sc.REPO

_ABNORMAL = []          # the cases whose child ended abnormally: nothing more is started behind them
_ORACLE = {}            # oracle frames per set, computed once and shared (never modified)

_WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from microbecensus_amd import _native
reads = np.load(sys.argv[3])
eng = _native.Engine(device=0)
eng.set_run(reads.shape[1])
if sys.argv[2] == "frames":
    eng.upload(reads)
    eng.run_range(0, reads.shape[0])
    np.save(sys.argv[4], eng.debug_stage(0))
    np.save(sys.argv[4] + ".form.npy", eng.debug_stage(5).reshape(-1).view("<u4"))
else:
    rows, _ = eng.search(reads)
    np.save(sys.argv[4], rows)
eng.close()
"""
LIMIT = 120             # seconds per child (measured: a child takes under a second, most of it the engine's start)


def _child(case, mode, reads, tmp, staged=None):
    if _ABNORMAL:
        pytest.fail("not started: the child of case %s ended abnormally earlier in this module" % _ABNORMAL[0], pytrace=False)
    w = tmp / "worker.py"
    w.write_text(_WORKER)
    np.save(str(tmp / "reads.npy"), np.ascontiguousarray(reads))
    env = dict(os.environ)
    env.pop("MC_TS_STAGED", None)
    if staged is not None:
        env["MC_TS_STAGED"] = staged
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, str(w), REPO, mode, str(tmp / "reads.npy"), str(tmp / "out.npy")]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=LIMIT + 30)
    except subprocess.TimeoutExpired as e:
        _ABNORMAL.append(case)
        pytest.fail("%s: no end after %d s\n%s" % (case, LIMIT + 30, e.stdout), pytrace=False)
    if p.returncode != 0:
        _ABNORMAL.append(case)
        pytest.fail("%s: exit status %d\n%s" % (case, p.returncode, p.stdout[-4000:]), pytrace=False)
    out = np.load(str(tmp / "out.npy"))
    if mode == "frames":                                             # ... and the form of the kernel the launch says it ran
        return out, int(np.load(str(tmp / "out.npy.form.npy"))[0])
    return out


def _oracle(key, reads):
    if key not in _ORACLE:
        want, lens = sc.oracle_frames(reads)
        want.setflags(write=False)
        _ORACLE[key] = (want, lens)
    return _ORACLE[key]


def _check_frames(case, key, reads, tmp, staged=None):
    n, L = reads.shape
    got, form = _child(case, "frames", reads, tmp, staged)
    want, lens = _oracle(key, reads)
    assert form == (int(staged) if staged is not None else int(sc.launch_stages_reads(L))), "the launch ran the other form of the kernel"
    if key[0] == "set":                                              # a full set: it holds what the issue asks of one
        sc.check_conditions(L, reads, want, lens)
    fp = ((L // 3 + 2) + 3) & ~3                                     # the frame pitch of mc_set_run
    assert got.shape == (6 * n, fp), got.shape
    got = got.reshape(n, 6, fp)
    bad = 0
    for f in range(6):
        bad += int((got[:, f, :lens[f]] != want[:, f, :lens[f]]).any(1).sum())
        assert (got[:, f, lens[f]:] == sc.MC_INV).all(), "frame %d: residues behind the frame's length" % f
    masked = int(((want == sc.MC_INV) & (sc.translate6(reads) != sc.MC_INV)).sum())
    print("%s: %d frames compared (%d reads of %d bp, MC_TS_STAGED %s, reads %s), %d residues masked by the oracle, %d frames differ"
          % (case, 6 * n, n, L, "unset" if staged is None else staged, "staged in LDS" if form else "from global memory", masked, bad))
    assert bad == 0
    return want, lens


def _set_size(L):
    return 300 if L <= 36 else 600 if L <= 151 else 400


# 18, 23, 24: the first frames of 8 residues.  33, 35, 36: W = 8 and W = 12 in frames of one read.  Odd lengths: a block's reads
# start at every byte alignment (head and tail of the staging copy).  188 ... 239: both sides of every switch of the launch
# (seg_cases.SWITCHES; every case asserts that the launch ran the form seg_cases.launch_stages_reads expects).
LENGTHS = [18, 23, 24, 33, 35, 36, 100, 101, 150, 151, 188, 189, 236, 237, 238, 239, 300, 342, 509, 510]


@pytest.mark.parametrize("L", LENGTHS)
def test_frames_at_the_launch_s_own_choice(L, tmp_path):
    reads = sc.make_reads(L, _set_size(L), seed=3)
    _check_frames("L%d" % L, ("set", L), reads, tmp_path)


@pytest.mark.parametrize("staged", ["1", "0"], ids=["reads_staged_in_lds", "reads_from_global"])
@pytest.mark.parametrize("L", [100, 151, 300, 510])
def test_frames_in_both_forms(L, staged, tmp_path):
    """Both forms of the kernel on the same set (the oracle's frames are those of the case above).  At 510 bp read 0 is the whole
    witness read: the frame that lost a remainder lies inside a full set."""
    reads = sc.make_reads(L, _set_size(L), seed=3)
    want, lens = _check_frames("L%d staged %s" % (L, staged), ("set", L), reads, tmp_path, staged)
    if L == 510:
        assert sc.blocks_of(want[0, sc.WITNESS_FRAME, :lens[sc.WITNESS_FRAME]] == sc.MC_INV)[-1] == 28


@pytest.mark.parametrize("n", [1, 9, 10, 11, 1001])
def test_read_counts_around_a_workgroup(n, tmp_path):
    """A workgroup owns ten reads: one read, one short of a workgroup, exactly one, one more, and 100 workgroups plus one read."""
    reads = sc.make_reads(150, 1001, seed=5, with_witness=False)[:n]
    _check_frames("n%d" % n, ("count", n), reads, tmp_path)


def test_many_pending_stretches_per_wave(tmp_path):
    """No control reads: nearly every frame of a wave has a stretch pending in every batch, so the batches have many items.  That
    they take the runs of 8 windows follows from mc_seg_wave's rule (the smallest run whose items fit one round); nothing here
    observes the run length, and every set ends with batches of few pending lanes, which take the short runs."""
    reads = sc.make_reads(300, 400, seed=7, families=("periodic", "mosaic", "long"), dirty=False, with_witness=False)
    want, lens = _check_frames("dense", ("dense",), reads, tmp_path)
    per_read = sc.masked_by_oracle(reads, want).any(2).sum(1)
    assert per_read.mean() > 5.5                                     # of 6 frames per read


def test_few_pending_stretches_per_wave(tmp_path):
    """One periodic read per workgroup among reads the oracle masks nothing on: only the six lanes of that read ever have a stretch
    pending, so the batches have few items (the short runs, by the same rule: inferred, not observed)."""
    reads = sc.sparse_set(300, 400, seed=7)
    want, lens = _check_frames("sparse", ("sparse",), reads, tmp_path)
    per_read = sc.masked_by_oracle(reads, want).any(2).sum(1)
    assert np.array_equal(np.flatnonzero(per_read), np.arange(3, 400, 10))   # one read in ten has anything masked, and each of them has
    print("sparse: %d of 400 reads have a masked frame, %.1f frames each" % ((per_read > 0).sum(), per_read[per_read > 0].mean()))


def test_the_witness_frame_alone(tmp_path):
    reads = sc.witness(510).reshape(1, 510)
    want, lens = _check_frames("witness", ("witness",), reads, tmp_path)
    assert sc.blocks_of(want[0, sc.WITNESS_FRAME, :lens[sc.WITNESS_FRAME]] == sc.MC_INV)[-1] == 28


def test_masks_are_carried_through_the_search(tmp_path):
    """End to end: 300 marker-gene reads of 510 bp with 60 - 120 bp in the middle replaced by periodic or mosaic content - every m8
    row equal to the oracle's, so the masks are the ones the seeds and the extensions see."""
    from test_gpu_pipeline import _oracle_rows, _rows, assert_rows_equal
    L, n = 510, 300
    reads = sc.control_reads(n, L, seed=41).copy()
    r = sc.Lcg(43)
    for i in range(n):
        k = r.between(60, 120)
        at = (L - k) // 2
        prot = sc.periodic(r, k // 3 + 1) if i % 2 else sc.mosaic(r, k // 3 + 1)
        reads[i, at:at + k] = sc.encode(prot, k, i % 3, r)
    rows = _child("end to end", "rows", reads, tmp_path)
    want = _oracle_rows(reads)
    print("end to end: %d rows over %d reads" % (len(want), n))
    assert len(want) > 100
    assert_rows_equal(_rows(rows), want)
