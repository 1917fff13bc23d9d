"""The kernels of the seed stage (csrc/k_enumerate.h: k_enumerate, k_enumerate_q, k_enumerate_count; csrc/k_eval_seeds.h: k_post8,
k_eval_seeds<false | true>), each on inputs built to reach its own edges - the suite otherwise runs them inside mc_run_range only, on
the hits natural reads happen to produce: none controls where an X-drop walk stands when the drop is exactly the threshold, where a
grown seed hands over from registers to loops, how many records the evaluation is dealt, or how full a wave's queue and blocks are.
tests/emul/device_seeds.hip includes the library's kernel headers and is built here with the library's flags; every case is one child
process (order_cases.run_child), and every comparison is exact - as multisets where the kernels define no order.

The reference of every hit is the oracle's rs_extend_hit, of every row's seeds rs_seed_ranges (oracle/rapsearch_port.c: the pieces
rs_search_read itself runs); tests/test_seeds_host.py holds the host statements to them and asserts that every class of hit is there -
never from a device output."""
import numpy as np
import pytest

import gapped_cases as gc
import order_cases as oc
import seed_cases as sd

pytestmark = pytest.mark.gpu

NONE = sd.TASK_NONE
LIMIT = 60                                                            # seconds per child
SEEDTASK = np.dtype([("read", "<u4"), ("chrono", "<u4"), ("posting", "<u4"), ("w3", "<u4")])
CAND_SCORE = 40                                                       # an HSP of this raw score or more makes its read a candidate


def bits_of(score):
    """CalRes' rounded bit score (BlastStat::rawScore2Bit, gapped parameters)."""
    return np.floor((score * 0.267 - np.log(0.041)) / sd.LN2 * 100.0 + 0.5) / 100.0


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return oc.harness("device_seeds", tmp_path_factory)


@pytest.fixture(scope="module")
def world():
    return sd.world()


@pytest.fixture(scope="module")
def base(world):
    return sd.sections(world.frames, world.subjects, sd.L_NT) + [sd.hit_array(world.hits)]


def _untouched(b):
    return (np.frombuffer(b, np.uint8) == 0xEE).all()


def test_post8(harness, world, base, tmp_path):
    """k_post8: every posting's record is MC_POST8(posting, place in the residue array, rest of the subject) and the 24 residues around
    the place - from 8 in front of it, MC_INV where the array's room begins - postings within 8 residues of the array's two ends
    included; the guard words behind the records are intact.
    Time limit 60 s (measured on the MI355X: 0.43 s; the harness, built once per module, 7.5 s)."""
    out = oc.run_child(harness, "post8", base[:4], tmp_path, LIMIT)
    got = np.frombuffer(out[0], "<u8").reshape(-1, 4)
    post, res = np.frombuffer(out[2], "<u4").astype(np.uint64), np.frombuffer(out[3], np.uint8)
    off, dense = oc.pack(world.subjects, np.uint8)
    assert np.array_equal(res, dense) and np.array_equal(post, world.db.post) and _untouched(out[1])
    s, dpos = (post >> np.uint64(11)).astype(np.int64), (post & np.uint64(0x7FF)).astype(np.int64)
    at = off[s].astype(np.int64) + dpos
    rem = off[s + 1].astype(np.int64) - at
    assert np.array_equal(got[:, 0], post | (at.astype(np.uint64) << np.uint64(26)) | (rem.astype(np.uint64) << np.uint64(50)))
    room = np.concatenate([np.full(64, sd.MC_INV, np.uint8), dense, np.full(64, sd.MC_INV, np.uint8)])
    around = room[(at + 56)[:, None] + np.arange(24)[None, :]]
    assert np.array_equal(got[:, 1:].copy().view(np.uint8).reshape(-1, 24), around)
    assert (at < 8).any() and (at + 16 > len(dense)).any()
    print("%d postings, %d within 8 residues of the array's start, %d of its end" % (len(post), (at < 8).sum(), (at + 16 > len(dense)).sum()))


# ---- k_eval_seeds ---------------------------------------------------------------------------------------------------------------------------
def run_eval(harness, base, tmp_path, case, n, places, which, ranges, cap_hsps, cap_gaps, says=0xFFFFFFFF, cand=1):
    arrays = base + [np.asarray(places, np.uint32), np.asarray(which, np.int32), np.array([n, int(ranges), cap_hsps, cap_gaps, says, cand, 0], np.uint32),
                     np.array([bits_of(CAND_SCORE) - 0.001])]
    out = oc.run_child(harness, case, arrays, tmp_path, LIMIT, verb="eval")
    return dict(hsps=np.frombuffer(out[0], oc.HSP), hkeys=np.frombuffer(out[1], "<u8"), hplace=np.frombuffer(out[2], "<u8"), gaps=np.frombuffer(out[3], gc.TASK),
                low=np.frombuffer(out[4], "u1"), cand=np.frombuffer(out[5], "u1"), counters=np.frombuffer(out[6], "<u4"), guards=out[7:11], raw=out)


def expected(world, which):
    """The gap tasks and HSPs the oracle says the records make - record k carries hit which[k] - as sorted tuples, and low, cand."""
    gaps, hsps = [], []
    low, cand = np.zeros(sd.NREADS, np.uint8), np.zeros(sd.NREADS, np.uint8)
    for k, i in enumerate(which):
        h, o = world.hits[i], world.want[i]
        if o["why"] != sd.EXTENDED:
            continue
        chrono = (h["frame"] << 25) | (h["qpos"] << 17) | k
        if o["gapped"]:
            gaps.append((h["read"], chrono, h["sidx"], o["qp"], o["dp"], o["L"], o["qfwd"], o["qbwd"], o["score"], o["nmatch"]))
        elif o["kept"]:
            hsps.append((h["read"], chrono, h["sidx"], o["score"], h["frame"], o["alnlen"], o["mism"], 0, o["nmatch"], o["qaas"], o["qaae"], o["ds"], o["de"], o["qnts"], o["qnte"], o["loge"]))
            if o["loge"] < 1.0: low[h["read"]] = 1
            if o["score"] >= CAND_SCORE: cand[h["read"]] = 1
    return sorted(gaps), sorted(hsps), low, cand


def check_eval(r, world, n, which, cap_hsps, cap_gaps, cand=1):
    """Everything k_eval_seeds wrote, against the oracle: the records field by field, the words beside each HSP, low and cand, the
    padding and the counters, what lies behind the pools' fills and in the guards."""
    c = r["counters"]
    want_gaps, want_hsps, want_low, want_cand = expected(world, which)
    assert c[sd.C_OVERFLOW] == 0 and c[sd.C_TASKS] == n
    nh, ng = int(c[sd.C_HSPS]), int(c[sd.C_GAPS])
    assert nh % 256 == 0 and ng % 256 == 0 and nh <= cap_hsps and ng <= cap_gaps
    hs, gs = r["hsps"][:nh], r["gaps"][:ng]
    real_h, real_g = hs["read"] != NONE, gs["read"] != NONE
    assert (~real_h).sum() == c[sd.C_HPAD] and (~real_g).sum() == c[sd.C_GPAD]
    assert (r["hkeys"][:nh][~real_h] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert sorted(tuple(x) for x in gs[real_g].tolist()) == want_gaps
    assert sorted(tuple(x) for x in hs[real_h].tolist()) == want_hsps
    k = hs[real_h]
    u = np.uint64
    assert np.array_equal(r["hkeys"][:nh][real_h], (k["read"].astype(u) << u(43)) | (k["sidx"].astype(u) << u(28)) | k["chrono"].astype(u))
    assert np.array_equal(r["hplace"][:nh][real_h], (k["score"].astype(u) << u(41)) | oc.place_words(k).astype(u))
    assert np.array_equal(r["low"], want_low) and np.array_equal(r["cand"], want_cand if cand else np.zeros_like(want_cand))
    assert _untouched(r["hsps"][nh:].tobytes()) and _untouched(r["hkeys"][nh:].tobytes()) and _untouched(r["hplace"][nh:].tobytes()) and _untouched(r["gaps"][ng:].tobytes())
    assert all(_untouched(g) for g in r["guards"])
    return len(want_hsps), len(want_gaps)


def blocks(k):
    return (k + 255) // 256 * 256


def roomy(world, which):
    """Pools that cannot overflow whatever waves the records are dealt to: a block per wave that can have a record, and the records'."""
    waves = min(256 * sd.EV_BPC * 4, 2 * len(which) + 2)
    return 256 * waves + blocks(len(which))


@pytest.mark.parametrize("form", ("records", "posting_indices", "posting_indices_no_cand"))
def test_eval_world(harness, world, base, tmp_path, form):
    """Both forms of k_eval_seeds on every hit of the world, shuffled, with padding records singly and in runs among them: the gap tasks
    field by field and the HSPs against the oracle's CalRes record, as multisets; hkeys and hplace beside each HSP; low and cand at a
    bar of 40 raw score - and once with cand == nullptr; C_HSPS and C_GAPS multiples of 256, C_HPAD and C_GPAD what is padded.
    Time limit 60 s per child (measured on the MI355X: 0.39 - 0.44 s a case)."""
    rng = np.random.default_rng(5)
    which = rng.permutation(len(world.hits))
    gapsize = rng.choice([0, 0, 0, 1, 1, 2, 63, 64, 65], len(which))
    places = np.cumsum(gapsize + 1) - 1
    n = int(places[-1]) + 1 + 17
    cap = roomy(world, which)
    r = run_eval(harness, base, tmp_path, "world_" + form, n, places, which, form != "records", cap, cap, cand=0 if form.endswith("no_cand") else 1)
    nh, ng = check_eval(r, world, n, which, cap, cap, cand=0 if form.endswith("no_cand") else 1)
    with_hsp = len({h[0] for h in expected(world, which)[1]})         # (neither mark is everywhere or nowhere: HSPs of 31 .. 36 are kept above the E-value bar)
    assert 0 < r["low"].sum() < with_hsp and (form.endswith("no_cand") or 0 < r["cand"].sum() < with_hsp)
    print("%d records, %d hits, %d HSPs, %d gap tasks; %d reads low, %d candidates" % (n, len(which), nh, ng, r["low"].sum(), r["cand"].sum()))


@pytest.mark.parametrize("ranges", (0, 1))
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1023, 1024, 1025))
def test_eval_record_counts(harness, world, base, tmp_path, n, ranges):
    """Pools of 0, 1, 63, 64, 65, 1023, 1024 and 1025 records, all of them hits: around a chunk and around a group of sixteen chunks.
    Time limit 60 s per child (measured on the MI355X: 0.31 - 0.41 s a case)."""
    which = (np.random.default_rng(n).permutation(len(world.hits)))[np.arange(n) % len(world.hits)]
    cap = roomy(world, which)
    r = run_eval(harness, base, tmp_path, "count_%d_%d" % (n, ranges), n, np.arange(n), which, ranges, cap, cap)
    check_eval(r, world, n, which, cap, cap)


@pytest.mark.parametrize("ranges", (0, 1))
def test_eval_full_queues(harness, world, base, tmp_path, ranges):
    """A chunk of 63 hits that all pass the gate and a padding record, then seven chunks whose 64 hits all pass it: the wave's queue
    holds 63, then 127 survivors, chunk after chunk.
    Time limit 60 s per child (measured on the MI355X: 0.34 - 0.37 s a case)."""
    ok = [k for k, o in enumerate(world.want) if o["why"] == sd.EXTENDED]
    rng = np.random.default_rng(127)
    which = rng.choice(ok, 63 + 7 * 64)
    places = np.concatenate([np.arange(63), 64 + np.arange(7 * 64)])
    cap = roomy(world, which)
    r = run_eval(harness, base, tmp_path, "queues_%d" % ranges, 8 * 64, places, which, ranges, cap, cap)
    check_eval(r, world, 8 * 64, which, cap, cap)


DEAL_SIZES = (sd.STATIC_RECORDS - 64, sd.STATIC_RECORDS, sd.STATIC_RECORDS + 1, sd.STATIC_RECORDS + 3 * sd.EV_GROUP * 64)


@pytest.mark.parametrize("ranges", (0, 1))
@pytest.mark.parametrize("n", DEAL_SIZES)
def test_eval_deal(harness, world, base, tmp_path, n, ranges):
    """Pools as large as what the waves take by their number (5,242,880 records), a chunk less, a record more and three groups more,
    all padding (made by the harness on the device) but for hits in the last chunk dealt by number, in the first group dealt through
    C_EVCHUNK and in the pool's last chunk: every hit is evaluated exactly once.
    Time limit 60 s per child (measured on the MI355X: 0.31 - 0.43 s a case, 84 MB of padding records included)."""
    S = sd.STATIC_RECORDS
    places = set(range(min(n, S) - 64, min(n, S))) | set(range(S, min(n, S + sd.EV_GROUP * 64))) | set(range((n - 1) // 64 * 64, n))
    places = np.array(sorted(places))
    which = np.random.default_rng(n & 0xFFFF).permutation(len(world.hits))[np.arange(len(places)) % len(world.hits)]
    cap = roomy(world, which)
    r = run_eval(harness, base, tmp_path, "deal_%d_%d" % (n, ranges), n, places, which, ranges, cap, cap)
    check_eval(r, world, n, which, cap, cap)
    if n > S:
        assert r["counters"][sd.C_EVCHUNK] >= (n - S + sd.EV_GROUP * 64 - 1) // (sd.EV_GROUP * 64)
    print("%d records, %d hits at %d .. %d; C_EVCHUNK %d" % (n, len(places), places[0], places[-1], r["counters"][sd.C_EVCHUNK]))


@pytest.mark.parametrize("ranges", (0, 1))
def test_eval_caps(harness, world, base, tmp_path, ranges):
    """All hits in records 0 .. 1023 - one wave writes them, so block use is determinate: 300 HSPs and 724 gap tasks, two and three blocks.
    Pools of exactly those blocks: no overflow, every record right.  One slot less in the HSP pool: C_OVERFLOW is 2; in the gap pool:
    3; the guards behind the pools are untouched.  *ntasks_p = cap_tasks + 1: nothing is written and no counter moves.
    Time limit 60 s per child (measured on the MI355X: 1.30 s a case, four children)."""
    hsp = [k for k, o in enumerate(world.want) if o["why"] == sd.EXTENDED and not o["gapped"] and o["kept"]]
    gap = [k for k, o in enumerate(world.want) if o["why"] == sd.EXTENDED and o["gapped"]]
    rng = np.random.default_rng(300)
    which = rng.permutation(np.concatenate([rng.choice(hsp, 300), rng.choice(gap, 724)]))
    ch, cg = blocks(300), blocks(724)
    r = run_eval(harness, base, tmp_path, "caps_exact_%d" % ranges, 1024, np.arange(1024), which, ranges, ch, cg)
    assert check_eval(r, world, 1024, which, ch, cg) == (300, 724)
    assert r["counters"][sd.C_HSPS] == ch and r["counters"][sd.C_GAPS] == cg
    for code, caps in ((2, (ch - 1, cg)), (3, (ch, cg - 1))):
        r = run_eval(harness, base, tmp_path, "caps_short_%d_%d" % (code, ranges), 1024, np.arange(1024), which, ranges, *caps)
        assert r["counters"][sd.C_OVERFLOW] == code and all(_untouched(g) for g in r["guards"])
    r = run_eval(harness, base, tmp_path, "caps_ntasks_%d" % ranges, 1024, np.arange(1024), which, ranges, ch, cg, says=1025)
    want = np.zeros(sd.C_N, np.uint32)
    want[sd.C_TASKS] = 1025
    assert np.array_equal(r["counters"][:sd.C_N], want)
    assert all(_untouched(b) for b in r["raw"][:4]) and all(_untouched(g) for g in r["guards"]) and not r["low"].any() and not r["cand"].any()


# ---- the seed kernels -----------------------------------------------------------------------------------------------------------------------
KINDS = {"plain": 0, "queues": 1, "counting": 2}


def run_enumerate(harness, tmp_path, w, case, L, nreads, kind, cap):
    fr, _, hits = sd.enum_want(w, L, nreads)
    out = oc.run_child(harness, case, sd.sections(fr, w.subjects, L) + [np.array([KINDS[kind], cap], np.uint32)], tmp_path, LIMIT, verb="enumerate")
    return np.frombuffer(out[0], SEEDTASK), np.frombuffer(out[1], "<u4"), out[2], np.frombuffer(out[3], "<u4"), np.frombuffer(out[4], "<u4"), hits


@pytest.mark.parametrize("nreads", (1, 15, 16, 17, 33))
@pytest.mark.parametrize("L", sd.ENUM_LENGTHS)
@pytest.mark.parametrize("kind", tuple(KINDS))
def test_enumerate(harness, tmp_path, kind, L, nreads):
    """k_enumerate, k_enumerate_q and k_enumerate_count on the constructed database and reads (seed_cases.EnumWorld), 1, 15, 16, 17 and 33
    reads of 510 and of 30 bases: the multiset of (read, hit order, posting, seed length, key residues) - a posting index mapped to its
    posting for k_enumerate_q, position in the residue array and rest of the subject checked for the other two - is the oracle's ranges
    expanded per posting; C_TASKS counts the hits and the padding records, and nothing lies behind it.
    Time limit 60 s per child (measured on the MI355X: 0.29 - 0.39 s a case)."""
    w = sd.enum_world()
    want = sd.enum_want(w, L, nreads)[2]
    cap = len(want) + 2048 * 300
    pool, c, guard, post, off, _ = run_enumerate(harness, tmp_path, w, "enumerate", L, nreads, kind, cap)
    assert np.array_equal(post, w.db.post)
    nt = int(c[sd.C_TASKS])
    assert c[sd.C_OVERFLOW] == 0 and nt <= cap and _untouched(pool[nt:].tobytes()) and _untouched(guard)
    used = pool[:nt]
    real = used[used["read"] != NONE]
    assert len(real) == len(want) and (kind != "plain" or nt == len(want))
    seedlen, nkey = (real["w3"] >> 24) & 15, real["w3"] >> 28
    if kind == "queues":
        assert (real["posting"] < len(post)).all()
        read, posting = real["read"], post[real["posting"]]
    else:
        read, posting = real["read"] & 0x1FFFFF, real["posting"]
        s, dpos = posting >> 11, posting & 0x7FF
        assert np.array_equal(real["w3"] & 0xFFFFFF, off[s] + dpos) and np.array_equal(real["read"] >> 21, off[s + 1] - off[s] - dpos)
    got = sorted(zip(read.tolist(), real["chrono"].tolist(), posting.tolist(), seedlen.tolist(), nkey.tolist()))
    assert got == want, "first differences: %s" % [x for x in zip(got, want) if x[0] != x[1]][:5]
    print("%s, %d reads of %d bases: %d hits in %d records" % (kind, nreads, L, len(want), nt))


@pytest.mark.parametrize("kind", tuple(KINDS))
def test_enumerate_overflow(harness, tmp_path, kind):
    """A task pool that ends within one block (2,048 records) in front of the hits' own number - one record for k_enumerate, which
    pads nothing: the overflow is flagged and nothing is written behind the pool.
    Time limit 60 s per child (measured on the MI355X: 0.34 - 0.39 s a case)."""
    w = sd.enum_world()
    want = sd.enum_want(w, sd.L_NT, sd.ENUM_READS)[2]
    cap = len(want) - 1 if kind == "plain" else (len(want) - 1) // 2048 * 2048
    pool, c, guard, _, _, _ = run_enumerate(harness, tmp_path, w, "overflow", sd.L_NT, sd.ENUM_READS, kind, cap)
    assert c[sd.C_OVERFLOW] == 1 and _untouched(guard)
