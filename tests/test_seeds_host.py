"""What the seed stage's GPU unit tests (test_gpu_seeds_units.py) rest on, without a GPU: on every hit of the case set (tests/seed_cases.py)
the host statement of the seed evaluation (csrc/mc_core.h: mc_eval_seed_core, mc_make_hsp) against the oracle's rs_extend_hit, and on
every row of the enumeration set mc_enumerate_seeds against rs_seed_ranges - the pieces rs_search_read itself runs, exported by
oracle/rapsearch_port.c; the populations of the hit classes; the legality of every hit.  tests/emul/seeds.cpp is built with g++."""
import numpy as np
import pytest

import seed_cases as sd


@pytest.fixture(scope="module")
def world():
    return sd.world()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sd.build_host(tmp_path_factory.mktemp("seeds_host"))


def test_every_hit_is_a_legal_state_of_the_pipeline(world):
    bad = [(k, h["cls"]) for k, h in enumerate(world.hits) if not sd.legal(world, h)]
    assert not bad, bad[:20]
    assert (world.frames <= sd.MC_INV).all() and all((world.frames[:, f, sd.QLEN[f]:] == sd.MC_INV).all() for f in range(6))
    assert len(world.hits) < 1 << 17                                 # (the hit's number rides in the low 17 bits of its chrono word)


def test_evaluation_equals_the_oracle(world, exe, tmp_path):
    """mc_eval_seed_core and mc_make_hsp == rs_extend_hit on every hit: dropped or not, the grown seed, the walks' extents, score and
    identities, the gapped trigger, CalRes' record and its rounded log E - exactly."""
    res, loge, _, post, bstart, _ = sd.host_seeds(exe, tmp_path, world.frames, world.subjects, sd.L_NT, world.hits, [])
    want = np.array([sd.want_result(h, o) for h, o in zip(world.hits, world.want)])
    bad = np.flatnonzero((res[:, :22] != want).any(1))
    assert not len(bad), [(int(k), world.hits[k]["cls"], res[k, :22].tolist(), want[k].tolist()) for k in bad[:10]]
    done = np.flatnonzero(want[:, 0] == 1)
    assert len(done) and all(loge[k] == world.want[k]["loge"] for k in done), [(int(k), loge[k], world.want[k]["loge"]) for k in done if loge[k] != world.want[k]["loge"]][:10]
    # the index the product builds on the subjects is the one the oracle searches
    assert np.array_equal(post, world.db.post) and np.array_equal(bstart.astype(np.int64), world.db.bstart)


def test_class_populations(world):
    """Every class of hit the GPU tests count on is there, by the oracle's answers alone."""
    pop = sd.populations(world)
    print("\n".join("%-45s %d" % kv for kv in sorted(pop.items())))
    missing = [c for c in sd.REQUIRED if not pop.get(c)]
    assert not missing, missing


@pytest.mark.parametrize("L", sd.ENUM_LENGTHS)
def test_enumeration_equals_the_oracle(exe, tmp_path, L):
    """mc_enumerate_seeds == rs_seed_ranges on every row of the enumeration set, range by range in order: position, bucket, seed
    length, key residues, the postings' range and the phase number."""
    w = sd.enum_world()
    fr, want, hits = sd.enum_want(w, L, sd.ENUM_READS)
    _, _, got, post, bstart, _ = sd.host_seeds(exe, tmp_path, fr, w.subjects, L, [], list(range(sd.ENUM_READS * 6)))
    assert np.array_equal(post, w.db.post) and np.array_equal(bstart.astype(np.int64), w.db.bstart)
    for row, (g, o) in enumerate(zip(got, want)):
        assert g == o, (row, [x for x in zip(g, o) if x[0] != x[1]][:5], len(g), len(o))
    sizes = [r[5] - r[4] for o in want for r in o]
    print("L %d: %d ranges, %d hits; ranges of 1: %d, of more than 64: %d" % (L, len(sizes), len(hits), sizes.count(1), sum(s > 64 for s in sizes)))
    assert len(hits) > 500 and any(not o for o in want)


def test_enumeration_world(tmp_path):
    """The enumeration set holds what it is built to hold, read off the oracle's index and ranges: buckets of one posting, first-residue
    groups of RT_LONG keys and of RT_LONG + 1, a bucket with more than 30 postings and 10 different keys or more, postings with fewer than four
    key residues, a read with more than 256 positions that have a range, wholly invalid frames."""
    w = sd.enum_world()
    fr, ranges, hits = sd.enum_want(w, sd.L_NT, sd.ENUM_READS)
    keys = np.ctypeslib.as_array(sd.lib().rs_db_keys(w.db.h), (len(w.db.post),)).copy()
    sizes = np.diff(w.db.bstart)
    assert (sizes == 1).sum() > 1000
    big = int(np.argmax(sizes))
    assert sizes[big] > 30 and len(set(keys[w.db.bstart[big]:w.db.bstart[big + 1]].tolist())) >= 10
    groups = set()
    for b in np.flatnonzero(sizes >= sd.RT_LONG - 1):
        k = keys[w.db.bstart[b]:w.db.bstart[b + 1]] >> 12
        groups |= {int(c) for c in np.bincount(k, minlength=16)[:10]}
    assert {sd.RT_LONG - 1, sd.RT_LONG, sd.RT_LONG + 1, sd.RT_LONG + 2} <= groups
    short = {0x0FFF, 0x00FF, 0x000F}                                # (one, two, three key residues; a subject's last six residues are no posting)
    assert all(((keys & m) == m).any() for m in short)
    tails = {int(p) for p, k in zip(w.db.post, keys) if (k & 0xF) == 0xF}
    assert sum(h[2] in tails for h in hits) >= 10, "no hit on a posting with a short key"
    per_read = [len({(f, r[0]) for f in range(6) for r in ranges[6 * rd + f]}) for rd in range(sd.ENUM_READS)]
    assert max(per_read) > 256 and per_read[2] == 0 and not ranges[6 * 3]
    assert (fr[2] == sd.MC_INV).all()


def test_sanitized_host_statements(world, tmp_path):
    """seeds.cpp built with AddressSanitizer + UBSan, run as itself on every hit and on the short reads' rows: clean, and still the oracle's numbers."""
    exe = sd.build_host(tmp_path, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"))
    res, _, _, _, _, err = sd.host_seeds(exe, tmp_path, world.frames, world.subjects, sd.L_NT, world.hits, [0, 1, 2, 3, 4, 5])
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
    want = np.array([sd.want_result(h, o) for h, o in zip(world.hits, world.want)])
    assert np.array_equal(res[:, :22], want)
