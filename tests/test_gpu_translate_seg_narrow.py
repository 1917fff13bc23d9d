"""The narrow instantiation of k_translate_seg (csrc/k_translate_seg.h: one-word SEG bit sets, a four-entry work list and rows for the 60
lanes that have a frame, for reads up to 191 bp) against the oracle's rs_translate6(), byte for byte, at the smallest shapes at which
it can go wrong:

    18            first frames of 6 residues (no SEG at all)
    33, 36        W = 8 and W = 12 in the frames of one read
    100, 150      the flagship lengths
    186, 188, 189 frames of 62 and 63 residues; both sides of the launch's switch from staged to direct reads
    191           the last narrow length
    192, 195      frames of 64 and 65 residues: these must run the wide form

Each length runs at 1, 9, 10, 11 and 21 reads (a workgroup owns ten) of a dense set (periodic, mosaic and long-stretch reads: nearly every
lane has a stretch pending) and of a sparse one (one periodic read in ten: lanes 60 - 63 and the idle lanes are dealt the others'
windows), in both forms of MC_TS_STAGED.  The frames are read back with debug_stage(0); everything behind a frame's length must be MC_INV.
Every case asserts what the launch reports: stage 6 (narrow 1 / wide 0) and stage 5, which stays seg_cases.launch_stages_reads(L) - the
choice made from the wide layout's sizes - where MC_TS_STAGED is unset.

MC_TS_STAGED is read once per process: every case is a child process, one after the other, each under `timeout -k 10`.  A child that
ends by a signal, at its limit or with an error fails its test with its output, and every later case of the module then fails at once
without starting anything on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_cases as sc

pytestmark = pytest.mark.gpu
REPO = sc.REPO

_ABNORMAL = []
_SETS = {}              # per length: the two sets and the oracle's frames of them, computed once and shared (never modified)

COUNTS = [1, 9, 10, 11, 21]
NARROW = [18, 33, 36, 100, 150, 186, 188, 189, 191]
WIDE = [192, 195]
LIMIT = 120             # seconds per child (a child takes about a second, most of it the engine's start)

_WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from microbecensus_amd import _native
mode, src, dst = sys.argv[2], sys.argv[3], sys.argv[4]
z = np.load(src)
out = {}
if mode == "frames":
    eng = _native.Engine(device=0)
    eng.set_run(z["dense"].shape[1])
    for kind in ("dense", "sparse"):
        eng.upload(z[kind])
        for n in [int(x) for x in z["counts"]]:
            eng.run_range(0, n)
            out["%s_%d" % (kind, n)] = eng.debug_stage(0)
            out["%s_%d_form" % (kind, n)] = np.array([eng.debug_stage(5).reshape(-1).view("<u4")[0], eng.debug_stage(6).reshape(-1).view("<u4")[0]])
    eng.close()
else:
    reads, ranges = z["reads"], [tuple(int(x) for x in r) for r in z["ranges"]]
    model = _native.load_model()
    L = reads.shape[1]
    eng = _native.Engine(device=0)                 # the yardstick: one range at a time
    eng.set_run(L, model["pars"][str(L)], model["families"])
    eng.upload(reads)
    for i, (first, count) in enumerate(ranges):
        eng.run_range(first, count, first)
        out["want_rows_%d" % i], out["want_best_%d" % i] = eng.rows(), eng.best_hits()
    eng.close()
    eng = _native.Engine(device=0)                 # end(i), begin(i + 1), results of i: ranges 2 and 3 are translated by the lookahead
    eng.set_run(L, model["pars"][str(L)], model["families"])
    eng.upload(reads)
    eng.run_range(0, reads.shape[0], 0)            # (pools that hold the whole set: a range larger than the pools gives the lookahead up)
    ahead0 = eng.ranges_translated_ahead()
    eng.range_begin(ranges[0][0], ranges[0][1], ranges[0][0])
    for i in range(len(ranges)):
        eng.range_end()
        if i + 1 < len(ranges):
            eng.range_begin(ranges[i + 1][0], ranges[i + 1][1], ranges[i + 1][0])
        out["got_rows_%d" % i], out["got_best_%d" % i] = eng.rows(), eng.best_hits()
    out["ahead"] = np.array([eng.ranges_translated_ahead() - ahead0])
    out["form"] = np.array([eng.debug_stage(5).reshape(-1).view("<u4")[0], eng.debug_stage(6).reshape(-1).view("<u4")[0]])
    eng.close()
np.savez(dst, **out)
"""


def _child(case, mode, tmp, staged=None, **arrays):
    if _ABNORMAL:
        pytest.fail("not started: the child of case %s ended abnormally earlier in this module" % _ABNORMAL[0], pytrace=False)
    w = tmp / "worker.py"
    w.write_text(_WORKER)
    np.savez(str(tmp / "in.npz"), **arrays)
    env = dict(os.environ)
    env.pop("MC_TS_STAGED", None)
    if staged is not None:
        env["MC_TS_STAGED"] = staged
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, str(w), REPO, mode, str(tmp / "in.npz"), str(tmp / "out.npz")]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=LIMIT + 30)
    except subprocess.TimeoutExpired as e:
        _ABNORMAL.append(case)
        pytest.fail("%s: no end after %d s\n%s" % (case, LIMIT + 30, e.stdout), pytrace=False)
    if p.returncode != 0:
        _ABNORMAL.append(case)
        pytest.fail("%s: exit status %d\n%s" % (case, p.returncode, p.stdout[-4000:]), pytrace=False)
    return np.load(str(tmp / "out.npz"))


def _sets(L):
    if L not in _SETS:
        n = max(COUNTS)
        dense = sc.make_reads(L, n, seed=7, families=("periodic", "mosaic", "long"), dirty=False, with_witness=False)
        sparse = sc.sparse_set(L, n, seed=7)
        s = {"dense": (dense,) + tuple(sc.oracle_frames(dense)), "sparse": (sparse,) + tuple(sc.oracle_frames(sparse))}
        for reads, want, _ in s.values():
            reads.setflags(write=False)
            want.setflags(write=False)
        _SETS[L] = s
    return _SETS[L]


@pytest.mark.parametrize("staged", [None, "1", "0"], ids=["launch_s_choice", "reads_staged_in_lds", "reads_from_global"])
@pytest.mark.parametrize("L", NARROW + WIDE)
def test_frames_equal_the_oracle(L, staged, tmp_path):
    s = _sets(L)
    case = "L%d staged %s" % (L, staged)
    out = _child(case, "frames", tmp_path, staged, dense=s["dense"][0], sparse=s["sparse"][0], counts=np.array(COUNTS))
    fp = ((L // 3 + 2) + 3) & ~3                                     # the frame pitch of mc_set_run
    want_form = [int(staged) if staged is not None else int(sc.launch_stages_reads(L)), 1 if L in NARROW else 0]
    assert (L // 3 <= 63) == (L in NARROW)
    for kind in ("dense", "sparse"):
        reads, want, lens = s[kind]
        masked = sc.masked_by_oracle(reads, want)
        if L >= 33:
            assert masked.any(), "the %s set gives SEG nothing to do at %d bp" % (kind, L)
        for n in COUNTS:
            got, form = out["%s_%d" % (kind, n)], [int(x) for x in out["%s_%d_form" % (kind, n)]]
            assert form == want_form, "%s, %s, %d reads: the launch reports staged %d, narrow %d" % (case, kind, n, form[0], form[1])
            assert got.shape == (6 * n, fp), got.shape
            got = got.reshape(n, 6, fp)
            bad = 0
            for f in range(6):
                bad += int((got[:, f, :lens[f]] != want[:n, f, :lens[f]]).any(1).sum())
                assert (got[:, f, lens[f]:] == sc.MC_INV).all(), "%s, %s, %d reads, frame %d: residues behind the frame's length" % (case, kind, n, f)
            print("%s, %s, %d reads: %d frames compared, %d residues masked by the oracle, %d frames differ" % (case, kind, n, 6 * n, int(masked[:n].sum()), bad))
            assert bad == 0


def _fields_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def test_ranges_translated_by_the_lookahead(tmp_path):
    """Three consecutive ranges of 150 bp through range_end(i), range_begin(i + 1): ranges 2 and 3 are translated by the lookahead, by the
    narrow form.  Rows and best hits equal those of run_range, one range at a time; the last range ends in a partial workgroup."""
    from microbecensus_amd import synth
    ranges = [(0, 700), (700, 700), (1400, 707)]
    reads = synth.GenomeReads(device="cpu", seed=20261001).single(2107, 150).numpy()
    out = _child("lookahead", "ahead", tmp_path, None, reads=reads, ranges=np.array(ranges))
    assert int(out["ahead"][0]) == 2
    assert [int(x) for x in out["form"]] == [int(sc.launch_stages_reads(150)), 1]
    nrows = 0
    for i in range(3):
        assert _fields_equal(out["got_rows_%d" % i], out["want_rows_%d" % i]), "rows of range %d" % i
        assert _fields_equal(out["got_best_%d" % i], out["want_best_%d" % i]), "best hits of range %d" % i
        nrows += len(out["want_rows_%d" % i])
    print("lookahead: %d rows over 3 ranges" % nrows)
    assert nrows > 300
