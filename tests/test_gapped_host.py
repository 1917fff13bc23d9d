"""What the gapped stage's GPU unit tests (test_gpu_gapped_units.py) rest on, without a GPU: on every designed flank of the case set
(tests/gapped_cases.py) the two host-compilable statements of the extension (csrc/mc_core.h) against the oracle's AlignGapped
(rs_align_gapped of oracle/rapsearch_port.c: three trace planes and a traceback, where mc_core.h carries the path statistics forwards);
the populations of the flank classes; the inverse of k_gap_dedupe's mixer and the equal-tag pairs against a restatement of the hash.
tests/emul/gapped_win.cpp is built with g++ and runs mc_align_gapped and, over a plain array of the kernels' packed cells,
mc_align_gapped_win at the product's two windows."""
import numpy as np
import pytest

import gapped_cases as gc


@pytest.fixture(scope="module")
def world():
    return gc.world()


@pytest.fixture(scope="module")
def forms(world, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gapped_win")
    return gc.host_forms(gc.build_host_forms(tmp), world.flanks, tmp)[0]


@pytest.fixture(scope="module")
def want(world):
    return np.array([f["o"] for f in world.flanks])                 # gain, c1, c2, ident, steps, runs, gapcols, width, rows


def test_full_size_form_equals_the_oracle(world, forms, want):
    """mc_align_gapped == rs_align_gapped in all seven numbers on every designed flank, and never gives up on 1,200 columns."""
    bad = np.flatnonzero((forms[:, 0, :7] != want[:, :7]).any(1))
    assert not len(bad), [(world.flanks[k]["cls"], forms[k, 0, :7].tolist(), want[k, :7].tolist()) for k in bad[:10]]
    assert not forms[:, 0, 7].any()


@pytest.mark.parametrize("k", (1, 2))
def test_windowed_form(world, forms, want, k):
    """mc_align_gapped_win over packed cells at W = 36 and W = 64: it reports `overflow` exactly when the oracle's band is W columns
    wide or wider (a reading of the oracle alone: the largest j - (jStart - 1) over the cells it writes), the accessor reports a
    run count that left its five bits on every flank whose best path has 32 gap runs or more and whose band stays inside, and on
    every flank with neither the seven numbers are the oracle's."""
    W = (gc.WIN, gc.WIN2)[k - 1]
    over, ovf, wide = forms[:, k, 7].astype(bool), forms[:, k, 8].astype(bool), want[:, 7] >= W
    assert np.array_equal(over, wide), "W %d: overflow where the band is narrower, or none where it is wider: flanks %s" % (W, np.flatnonzero(over != wide)[:20])
    many = want[:, 5] >= 32
    assert ovf[many & ~wide].all()
    ok = ~over & ~ovf
    bad = np.flatnonzero(ok & (forms[:, k, :7] != want[:, :7]).any(1))
    assert not len(bad), [(world.flanks[i]["cls"], forms[i, k, :7].tolist(), want[i, :7].tolist()) for i in bad[:10]]
    print("W %d: %d flanks; %d leave the window by width, %d by a run count (%d of them with fewer than 32 runs on the best path: another live path had 32), %d equal the oracle"
          % (W, len(over), int(over.sum()), int((ovf & ~over).sum()), int((ovf & ~over & ~many).sum()), int(ok.sum())))


def test_class_populations(world, want):
    """Every class of flank the GPU tests count on is there: 20 members of a class that is a range, both directions counted, 4 of a
    class that is one value; the run-count flanks stay inside the 64-column window by width; 20 flanks reach k_gapped by width and 4
    by run count; W against W gains 11 a residue."""
    pop = gc.populations(world)
    pop["not_extended"] = world.unextended
    print("\n".join("%-18s %d" % kv for kv in sorted(pop.items())))
    for name in ("ordinary", "not_extended", "nothing_gained", "masked_odd", "ended_early", "runs40_up", "w17_35", "w38_63", "w66_up"):
        assert pop.get(name, 0) >= 20, name
    for name in ("largest", "largest_mismatch", "runs31", "runs32", "runs33", "w35", "w36", "w37", "w63", "w64", "w65"):
        assert pop.get(name, 0) >= 4, name
    cls = np.array([f["cls"] for f in world.flanks])
    side = np.array([f["side"] for f in world.flanks])
    n1 = np.array([len(f["q"]) for f in world.flanks])
    n2 = np.array([len(f["s"]) for f in world.flanks])
    assert (want[cls == "runs", 7] < gc.WIN2).all()
    by_width, by_runs = want[:, 7] >= gc.WIN2, (want[:, 5] >= 32) & (want[:, 7] < gc.WIN2)
    print("to k_gapped by width %d, by run count %d; to the second window by width %d" % (by_width.sum(), by_runs.sum(), (want[:, 7] >= gc.WIN).sum()))
    assert by_width.sum() >= 20 and by_runs.sum() >= 4
    assert (want[cls == "largest", 0] == 11 * n1[cls == "largest"]).all()
    assert (want[cls == "nothing_gained", 0] == 0).all() and (want[cls == "ended_early", 8] < n1[cls == "ended_early"]).all()
    o = cls == "ordinary"
    assert (side[o] == 0).sum() == (side[o] == 1).sum()
    assert set(n1[o]) == set(gc.N1_SIZES) and set(gc.N1_SIZES) | {200, 600, gc.DLEN_MAX - 1} <= set(n2[o])
    # the first subject carries a left flank of 3 residues, the last subject a right flank (every right flank ends on its subject's last residue)
    f0 = world.flanks[0]
    assert world.tasks[f0["task"]]["sidx"] == 0 and f0["side"] == 1 and len(f0["s"]) == 3
    last = [t for t in world.tasks if t["read"] != gc.TASK_NONE and t["sidx"] == len(world.subjects) - 1]
    assert last and all(world.seg_flanks(world.segment(t))[0] is not None for t in last)
    assert (world.frames[:256, :, :169] == gc.MC_INV).any() and any((s == gc.MC_INV).any() for s in world.subjects)
    assert all(world.legal(t) for t in world.tasks)


def _hash_restated(read, sidx, frame, qs, ds, qe):
    """k_gap_dedupe's hash of a segment, once more, in 64-bit numpy arithmetic (wrapping)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        h = (u(read) << u(32)) ^ (u(sidx) << u(12)) ^ u(frame)
        h ^= (u(qs & 0xFFFF) << u(48)) ^ (u(ds & 0xFFFF) << u(20)) ^ (u(qe & 0xFFFF) << u(3))
        h = h * u(0x9E3779B97F4A7C15)
        h ^= h >> u(29)
        h = h * u(0xBF58476D1CE4E5B9)
        h ^= h >> u(32)
    return int(h)


def test_mixer_inverse_and_equal_tag_pairs(world):
    """unmix is the mixer's inverse, and the equal-tag pairs are what they are built to be: legal, different segments whose hashes -
    by a restatement of the hash - agree in the tag (bits 27 - 63) and in the slot at both table sizes the GPU test uses."""
    rng = np.random.default_rng(7)
    for x in [0, 1, (1 << 64) - 1] + [int(v) for v in rng.integers(0, 1 << 63, 2000, dtype=np.uint64)]:
        assert gc.unmix(gc.mix(x)) == x and gc.mix(gc.unmix(x)) == x
    segs = {world.segment(t) for t in world.tasks if t["read"] != gc.TASK_NONE}
    for seg in list(segs)[:500]:
        assert gc.mix(gc.seg_word(*seg)) == _hash_restated(*seg)
    assert len(world.pairs) >= 8
    masks = [gc.table_slots(len(world.tasks)) - 1, gc.small_table(world) - 1]
    for a, b in world.pairs:
        ha, hb = _hash_restated(*a), _hash_restated(*b)
        assert a != b and a in segs and b in segs
        assert ha >> 27 == hb >> 27 and all(ha & m == hb & m for m in masks)
    print("%d equal-tag pairs; fields that differ: %s" % (len(world.pairs), sorted({n for a, b in world.pairs for n, x, y in zip(gc.NEAR_FIELDS, a, b) if x != y})))


def test_sanitized_window_check(world, want, tmp_path):
    """gapped_win built with AddressSanitizer + UBSan, run as itself on every designed flank - each flank in an array of exactly its
    length, the window an array of exactly W cells accessed with bounds checks: clean, and still the oracle's numbers."""
    exe = gc.build_host_forms(tmp_path, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    got, err = gc.host_forms(exe, world.flanks, tmp_path)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert np.array_equal(got[:, 0, :7], want[:, :7])
