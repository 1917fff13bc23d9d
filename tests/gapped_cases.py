"""Inputs of the gapped stage's unit tests (test_gapped_host.py on the CPU, test_gpu_gapped_units.py on the device), and the oracle's
side of every comparison: rs_align_gapped() of oracle/rapsearch_port.c through ctypes - AlignGapped with three trace planes and a
traceback, where csrc/mc_core.h carries the path statistics forwards.

One WORLD, built once per process by seeded numpy: synthetic frames (nreads x 6 x FP dense codes, MC_INV behind a frame's length), one
subject per flank (letters, as the index builder reads them), and McGapTask records.  Every record is a legal state of the pipeline:
reads of 510 bases (frames of 170 / 169 / 169 residues), subjects of at most MC_GAP_W - 8 residues, indices in range; the harnesses
check that again before they launch anything.  A flank is laid out so that its task extends on that side only: a right flank's segment
starts at subject offset 0 (nothing to the left), a left flank's segment ends on the subject's last residue.

The flank classes are those of DESIGN.md 5.1; where a class cannot be written down - a number of gap runs, a band width - the builder
searches candidates with the oracle under the fixed seed.  What the search established about two classes:
* An extension that the X-drop test ends in row 1 or in row 2 was not found, and the rule explains why.  AlignGapped leaves its row
  loop early only when jStart >= jEnd.  The trimming rule sets jStart <= bestJ and the X-drop exit of a row sets jEnd = j > bestJ, so
  once a cell has scored above 0 the rows run to n1; with best = 0 (bestJ = 0) the exit needs h(i, 1) < -26.98, and h(i, 1) >=
  -(11 + i) - 5: row 11 at the earliest (200,000 random flanks of 3 - 7 poorly matching residues: none ended before its last row).
  The class kept is "ended early": the oracle ran fewer than n1 rows (it reports the rows it ran).
* Equal tag, different segment: all pairings exist.  The pairs are found by inverting the mixer on a hash that differs from a legal
  segment's in bits 16 - 26 only (neither tag nor slot at either table size) and decoding the fields; a decoded pair differs in read,
  subject, frame and all three coordinates at once, since the inverse scatters the eleven changed bits over the whole word.  Four more
  pairs are equal in the whole hash without any search: the hashed word is not injective (subject and subject offset overlap in it).
  Real reads meet equal tags on different segments too: the end-to-end tests notice when the comparison of the records is taken
  out; the unit test pins the case."""
import ctypes as C
import os
import subprocess

import numpy as np

import order_cases as oc
import seg_cases as sc

MC_INV = sc.MC_INV
L_NT = 510
FP = sc.MC_FP                                                     # 172
QLEN = tuple((L_NT - f % 3) // 3 for f in range(6))               # 170, 169, 169, ...
GAP_W = oc.define("MC_GAP_W", "k_gapped.h")                       # 1200
WIN, WIN2 = oc.define("MC_GAP_WIN", "k_gapped.h"), oc.define("MC_GAP_WIN2", "k_gapped.h")   # 36, 64
DLEN_MAX = GAP_W - 8
TASK_NONE = 0xFFFFFFFF
NREADS = 4096                                                     # (most carry random residues: the equal-tag pairs need a wide range of reads)
AA = "ARNDCQEGHILKMFPSTWYV"
ODD = "X*/BZUJO-"                                                 # what mc_dense_of_char makes MC_INV of: the only non-standard dense code
C_OVERFLOW, C_RETRY, C_ITEMS, C_RETRY2, C_HSPS, C_GTAKE, C_GTAKE2 = 5, 8, 11, 12, 2, 30, 31      # (mc_hip_common.h's enum)

TASK = np.dtype([("read", "<u4"), ("chrono", "<u4"), ("sidx", "<u4"), ("qp", "<i2"), ("dp", "<i2"), ("L", "<i2"), ("qfwd", "<i2"), ("qbwd", "<i2"),
                 ("score", "<i2"), ("nmatch", "<i2")], align=True)
assert TASK.itemsize == 28
FOUT = np.dtype([(n, "<i2") for n in ("gain", "c1", "c2", "ident", "steps", "runs", "gapcols", "over")])
ORACLE_NAMES = ("gain", "c1", "c2", "ident", "steps", "runs", "gapcols", "width", "rows")

DENSE_TO_ORACLE = np.full(32, 0xA0, np.uint8)                     # seg_cases' statement of the map, read the other way
for _o, _d in sc.ORACLE_TO_DENSE.items():
    DENSE_TO_ORACLE[_d] = _o


def oracle(q, s):
    """rs_align_gapped on two flanks in walking order (dense codes): (gain, c1, c2, ident, steps, runs, gapcols, width, rows)."""
    lib = sc.oracle_lib()
    if not hasattr(lib, "_gapped_ready"):
        lib.rs_align_gapped.restype = C.c_int
        lib.rs_align_gapped.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        lib._gapped_ready = True
    out = (C.c_int * 8)()
    g = lib.rs_align_gapped(DENSE_TO_ORACLE[q].tobytes(), DENSE_TO_ORACLE[s].tobytes(), len(q), len(s), out)
    return (g,) + tuple(out)


# ---- the hash of k_gap_dedupe, restated; its inverse ------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
K1, K2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9
K1_INV, K2_INV = pow(K1, -1, 1 << 64), pow(K2, -1, 1 << 64)


def seg_word(read, sidx, frame, qs, ds, qe):
    return ((read << 32) ^ (sidx << 12) ^ frame ^ ((qs & 0xFFFF) << 48) ^ ((ds & 0xFFFF) << 20) ^ ((qe & 0xFFFF) << 3)) & M64


def mix(h):
    h = h * K1 & M64
    h ^= h >> 29
    h = h * K2 & M64
    return h ^ (h >> 32)


def unmix(h):
    """The inverse: x ^= x >> 32 undoes itself; the multiplications by their inverses modulo 2^64; x ^= x >> 29 is undone by
    x ^ x >> 29 ^ x >> 58 (the third term restores what the second one disturbed; 87 >= 64 ends it)."""
    h ^= h >> 32
    h = h * K2_INV & M64
    h = h ^ (h >> 29) ^ (h >> 58)
    return h * K1_INV & M64


def _unmix_np(h):
    h = h ^ (h >> np.uint64(32))
    h = h * np.uint64(K2_INV)
    h = h ^ (h >> np.uint64(29)) ^ (h >> np.uint64(58))
    return h * np.uint64(K1_INV)


def table_slots(ngaps):
    """The product's rule (mc_hip.hip, stage_b): 65,536 slots, doubled until there are two per task."""
    slots = 1 << 16
    while slots < 2 * ngaps:
        slots <<= 1
    return slots


def small_table(w):
    """The smallest power of two above the number of distinct segments: the table under load (one slot at least stays free)."""
    n, slots = len({w.segment(t) for t in w.tasks if t["read"] != TASK_NONE}), 1
    while slots <= n:
        slots <<= 1
    return slots


# ---- the world ------------------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self):
        self.rng = np.random.default_rng(20261019)
        self.frames = self.rng.integers(0, 20, (NREADS, 6, FP)).astype(np.uint8)
        for f in range(6):
            self.frames[:, f, QLEN[f]:] = MC_INV
        self.subjects = []                                           # dense codes per subject
        self.tasks = []                                              # dicts of the record's fields
        self.flanks = []                                             # dict(cls, task, side, q, s, o): one per designed flank
        self.slot = 0
        self.unextended = 0                                          # designed tasks with 0, 1 or 2 residues on a side: no item

    def rand(self, n):
        return self.rng.integers(0, 20, n).astype(np.uint8)

    def add_flank(self, cls, q, s, st, score=40):
        """A task whose flank on one side is (q, s), both in walking order, and which has nothing to extend on the other side."""
        q, s = np.asarray(q, np.uint8), np.asarray(s, np.uint8)
        n1, n2 = len(q), len(s)
        while QLEN[self.slot % 6] - n1 < 1:
            self.slot += 1
        read, frame = divmod(self.slot, 6)
        self.slot += 1
        assert read < 256                                            # (the designed flanks live in the first reads)
        qlen = QLEN[frame]
        seglen = int(self.rng.integers(1, min(qlen - n1, DLEN_MAX - n2) + 1))
        seg = self.rand(seglen)
        row = self.frames[read, frame]
        if st > 0:
            qs = qlen - n1 - seglen
            row[qs + seglen:qlen] = q
            self.subjects.append(np.concatenate([seg, s]))
            ds = 0
        else:
            qs = n1
            row[:n1] = q[::-1]
            self.subjects.append(np.concatenate([s[::-1], seg]))
            ds = n2
        t = dict(read=read, chrono=(frame << 25) | int(self.rng.integers(0, 1 << 25)), sidx=len(self.subjects) - 1, qp=qs, dp=ds, L=seglen, qfwd=0, qbwd=0,
                 score=score, nmatch=seglen // 2)
        self.tasks.append(t)
        if n1 > 2 and n2 > 2:
            self.flanks.append(dict(cls=cls, task=len(self.tasks) - 1, side=0 if st > 0 else 1, q=q, s=s, o=oracle(q, s)))
        else:
            self.unextended += 1
        return len(self.tasks) - 1

    # -- what a record says: its segment, the flanks of a segment
    def segment(self, t):
        return (t["read"], t["sidx"], t["chrono"] >> 25, t["qp"] - t["qbwd"], t["dp"] - t["qbwd"], t["qp"] + t["L"] + t["qfwd"])

    def seg_flanks(self, seg):
        """(right, left): each None where the reference does not extend, else (q, s) in walking order."""
        read, sidx, frame, qs, ds, qe = seg
        row, sub = self.frames[read, frame], self.subjects[sidx]
        qlen, dlen, de = QLEN[frame], len(sub), ds + (qe - qs)
        right = (row[qe:qlen], sub[de:]) if qlen - qe > 2 and dlen - de > 2 else None
        left = (row[:qs][::-1], sub[:ds][::-1]) if qs > 2 and ds > 2 else None
        return right, left

    def legal(self, t):
        if t["read"] == TASK_NONE:
            return True
        read, sidx, frame, qs, ds, qe = self.segment(t)
        return (read < NREADS and sidx < len(self.subjects) and frame < 6 and t["L"] >= 1 and t["qfwd"] >= 0 and t["qbwd"] >= 0 and 0 <= qs < qe <= QLEN[frame]
                and ds >= 0 and ds + (qe - qs) <= len(self.subjects[sidx]))

    def records(self, tasks=None):
        tasks = self.tasks if tasks is None else tasks
        rec = np.zeros(len(tasks), TASK)
        for k, t in enumerate(tasks):
            for n in TASK.names:
                rec[n][k] = t[n]
        return rec

    def sections(self):
        """What every verb of the harness reads first: L, FP, nreads; the frames; the subjects as letters and their offsets."""
        letters = np.frombuffer((AA + "X").encode(), np.uint8)
        off, res = oc.pack(self.subjects, np.uint8)
        text = letters[res].copy()
        inv = np.flatnonzero(res == MC_INV)
        text[inv] = np.frombuffer(ODD.encode(), np.uint8)[np.arange(len(inv)) % len(ODD)]     # every letter the builder turns into MC_INV, in turn
        return [np.array([L_NT, FP, NREADS], np.int32), self.frames, text, off]


def mutate(rng, q, subs, indels):
    """A copy of q with a share of substitutions and of single and multi-residue insertions and deletions."""
    out, i = [], 0
    while i < len(q):
        r = rng.random()
        if r < indels / 2:
            i += int(rng.integers(1, 4))                             # deletion
            continue
        if r < indels:
            out += list(rng.integers(0, 20, int(rng.integers(1, 4))))   # insertion
        out.append(int(rng.integers(0, 20)) if rng.random() < subs else int(q[i]))
        i += 1
    return np.array(out, np.uint8)


def fit(rng, s, n2):
    return np.concatenate([s, rng.integers(0, 20, max(0, n2 - len(s))).astype(np.uint8)])[:n2]


N1_SIZES = (3, 4, 15, 16, 17, 35, 36, 37, 63, 64, 65, 100, 168, 169)
N2_MORE = (200, 600, "longest")
W_, C_, H_, A_, T_ = (AA.index(c) for c in "WCHAT")
WIDTH_CLASSES = (("w17_35", 17, 35), ("w35", 35, 35), ("w36", 36, 36), ("w37", 37, 37), ("w38_63", 38, 63), ("w63", 63, 63), ("w64", 64, 64), ("w65", 65, 65),
                 ("w66_up", 66, 10 ** 6))
RUN_CLASSES = (("runs31", 31, 31), ("runs32", 32, 32), ("runs33", 33, 33), ("runs40_up", 40, 10 ** 6))


def run_flanks(k, rng):
    """k gaps: blocks of three residues of W, C, H, Y, P (at least 21 a block, at least 9 after the gap that follows it; every block
    drawn anew, so that no shift of the whole flank aligns as well) separated alternately by a residue inserted into the subject and one
    inserted into the query."""
    strong = np.array([AA.index(c) for c in "WCHYP"])
    q, s = [], []
    for b in range(k + 1):
        blk = [int(x) for x in strong[rng.permutation(5)[:3]]]
        q += blk; s += blk
        if b < k:
            (s if b % 2 == 0 else q).append(int(rng.integers(0, 20)))
    return np.array(q, np.uint8), np.array(s, np.uint8)


def climbs_for_widths(rng, quota):
    """Climbs from periodic pairs of flanks (every diagonal a period apart scores alike): one to three residues are changed at a time
    and the change is kept when the oracle's width does not shrink; each time the width grows and the flank gains something, the
    pair is yielded for every class of quota ({(lo, hi): members wanted}) that still wants it."""
    for _ in range(400):
        if not any(quota.values()):
            return
        n1, n2, per = int(rng.integers(60, 170)), int(rng.integers(150, 1151 if rng.random() < 0.3 else 400)), int(rng.integers(10, 16))
        u = rng.integers(0, 20, per).astype(np.uint8)
        q, s = np.tile(u, 20)[:n1].copy(), np.tile(u, 120)[:n2].copy()
        m = rng.random(n2) < 0.3
        s[m] = rng.integers(0, 20, int(m.sum()))
        o, stall, top = oracle(q, s), 0, max(hi for (lo, hi), n in quota.items() if n) if any(quota.values()) else 0
        while stall < 300 and o[7] < min(top, 150):
            q2, s2 = q.copy(), s.copy()
            for _ in range(int(rng.integers(1, 4))):
                if rng.random() < 0.4:
                    q2[rng.integers(0, n1)] = rng.integers(0, 20)
                else:
                    s2[rng.integers(0, n2)] = rng.integers(0, 20)
            o2 = oracle(q2, s2)
            grew = o2[7] > o[7]
            stall = 0 if grew else stall + 1
            if o2[7] >= o[7]:
                q, s, o = q2, s2, o2
            if grew and o[0] > 0:
                for (lo, hi), n in quota.items():
                    if n and lo <= o[7] <= hi:
                        quota[(lo, hi)] -= 1
                        yield q.copy(), s.copy()
                        break


def build_world():
    w = World()
    rng = w.rng
    # ordinary.  The first subject of the world carries a left flank of 3 residues (the fetch-ahead's 16 bytes reach into the padding in
    # front of the residue array); the last task added below is a right flank, which ends on the last residue of the last subject.
    q = w.rand(15)
    w.add_flank("ordinary", q, q[:3], -1)
    k = 0
    for n1 in N1_SIZES:
        for n2 in N1_SIZES + N2_MORE:
            for st in (1, -1):
                q = w.rand(n1)
                if n2 == "longest":
                    if n1 < 100:                                     # (the longest subject flank against every long query flank only: 1 + n1 + n2 residues of DP each)
                        continue
                    m = DLEN_MAX - 1
                else:
                    m = n2
                s = fit(rng, mutate(rng, q, (k % 11) / 100.0, (k % 4) / 100.0), m)
                w.add_flank("ordinary", q, s, st)
                k += 1
    # not extended: 0, 1 or 2 residues on one side or on both
    for n1, n2 in [(a, b) for a in (0, 1, 2) for b in (0, 1, 2, 40)] + [(40, b) for b in (0, 1, 2)]:
        for st in (1, -1):
            w.add_flank("not_extended", w.rand(n1), w.rand(n2), st)
    # nothing gained: W against C (-2) everywhere
    for n in (3, 5, 16, 17, 40, 64, 100, 169, 30, 31, 32, 33):
        for st in (1, -1):
            w.add_flank("nothing_gained", np.full(n, W_, np.uint8), np.full(n + (n % 3) * 7, C_, np.uint8), st)
    # masked and odd residues
    for k in range(24):
        q = w.rand(40 + 5 * k)
        s = fit(rng, mutate(rng, q, 0.05, 0.02), len(q) + 6)
        for _ in range(1 + k % 4):
            a = int(rng.integers(0, len(q) - 8)); q[a:a + int(rng.integers(1, 9))] = MC_INV
        s[rng.integers(0, len(s), 1 + k % 9)] = MC_INV
        w.add_flank("masked_odd", q, s, 1 if k % 2 else -1)
    # largest score: W against W, and one mismatch at the first, the middle, the last position
    for n in (169, 100):
        for st in (1, -1):
            w.add_flank("largest", np.full(n, W_, np.uint8), np.full(n, W_, np.uint8), st)
            for at in (0, n // 2, n - 1):
                s = np.full(n, W_, np.uint8); s[at] = C_
                w.add_flank("largest_mismatch", np.full(n, W_, np.uint8), s, st)
    # 32 gap runs and more (found with the oracle: the construction aims at k runs - a gap whose inserted residue scores well enough is
    # taken as a mismatch instead - and the oracle's count decides the class); a few with 34 - 39 runs ride along
    quota = {31: 4, 32: 4, 33: 4, 36: 4, 40: 20}
    for _ in range(3000):
        if not any(quota.values()):
            break
        q, s = run_flanks(int(rng.integers(33, 48)), rng)
        o = oracle(q, s)
        key = 40 if o[5] >= 40 else o[5]
        if len(q) <= 169 and quota.get(key, 0) > 0:
            quota[key] -= 1
            w.add_flank("runs", q, s, 1 if quota[key] % 2 else -1)
    # wide bands, found with the oracle: a climb from a periodic pair of flanks (every diagonal a period apart scores alike), one to three
    # residues changed at a time and kept when the width does not shrink, until the width is in the class aimed at.  (A plateau of
    # zero-score pairs does not do it: with best = 0 the X-drop exit fires on the first dead cell of a row, at column 1 from row 17
    # on, and the widest band of A against T is 32 columns.)
    quota = {(lo, hi): (4 if lo == hi else 20) for _, lo, hi in WIDTH_CLASSES if lo == hi}
    quota.update({(lo, hi): 20 for _, lo, hi in WIDTH_CLASSES if lo != hi})           # (the single widths first: a pair counts for one class)
    for k, (q, s) in enumerate(climbs_for_widths(rng, quota)):
        w.add_flank("wide", q, s, 1 if k % 2 else -1)
    # ended early: poor flanks, kept when the oracle ran fewer rows than the query flank has
    for k in range(60):
        q, s = w.rand(20 + k), w.rand(30 + 2 * k)
        if oracle(q, s)[8] < len(q):
            w.add_flank("ended_early", q, s, 1 if k % 2 else -1)
    q = w.rand(64)
    w.add_flank("ordinary", q, fit(rng, mutate(rng, q, 0.05, 0.01), 70), 1)
    w.nflank_tasks = len(w.tasks)
    _task_sets(w)
    assert all(w.legal(t) for t in w.tasks) and len(w.tasks) < (1 << 27) - 2 and max(len(s) for s in w.subjects) <= DLEN_MAX
    return w


GROUP_SIZES = (1, 2, 3, 64, 65, 257, 5000)
NEAR_FIELDS = ("read", "sidx", "frame", "qs", "ds", "qe")


def task_of(w, seg, rng, score=None):
    """A record of the segment: where the seed grew from and how far the ungapped extension went differ, the segment does not."""
    read, sidx, frame, qs, ds, qe = seg
    n = qe - qs
    L = int(rng.integers(1, n + 1))
    qbwd = int(rng.integers(0, n - L + 1))
    return dict(read=read, chrono=(frame << 25) | int(rng.integers(0, 1 << 25)), sidx=sidx, qp=qs + qbwd, dp=ds + qbwd, L=L, qfwd=n - L - qbwd, qbwd=qbwd,
                score=int(rng.integers(20, 60)) if score is None else score, nmatch=int(rng.integers(0, n + 1)))


def _task_sets(w):
    rng = w.rng
    extra, w.groups, w.near, w.pairs = [], [], [], []
    # groups: host segments with both flanks to extend, in subjects of their own
    for g, size in enumerate(GROUP_SIZES):
        q = w.rand(170)
        sub = fit(rng, mutate(rng, q, 0.08, 0.02), 150 + 40 * g)
        w.subjects.append(sub)
        seg = (256 + g, len(w.subjects) - 1, 0, 30 + g, 28 + g, 90 + 3 * g)
        w.frames[256 + g, 0, :170] = q
        w.groups.append((seg, size))
        extra += [task_of(w, seg, rng) for _ in range(size)]
    # a group none of whose flanks gains anything (the members still get their HSPs), and one with a score that keeps no HSP
    w.subjects.append(np.full(200, C_, np.uint8))
    w.frames[270, 0, :170] = W_
    for size, score in ((5, 45), (4, 3)):
        seg = (270, len(w.subjects) - 1, 0, 40 + size, 50, 100)
        w.groups.append((seg, size))
        extra += [task_of(w, seg, rng, score) for _ in range(size)]
    # near misses: two segments equal in five of the six compared quantities
    base = (300, w.groups[0][0][1], 3, 20, 25, 60)
    for k, name in enumerate(NEAR_FIELDS):
        other = list(base)
        other[k] += 1
        w.near.append((base, tuple(other), name))
        extra += [task_of(w, base, rng), task_of(w, tuple(other), rng)]
    # equal tag, different segment
    w.pairs = equal_tag_pairs(w, 12)
    # ... and equal in the whole hash: the subject (from bit 12) and the subject offset (from bit 20) overlap in the hashed word, so
    # subject s at offset d and subject s ^ 256 at offset d ^ 1 are one word
    roomy = [x for x in range(256) if min(len(w.subjects[x]), len(w.subjects[x ^ 256])) >= 120]
    for k in range(4):
        a = (310 + k, roomy[k], k, 10 + k, 40 + 2 * k, 50 + 3 * k)
        b = (a[0], a[1] ^ 256, a[2], a[3], a[4] ^ 1, a[5])
        assert seg_word(*a) == seg_word(*b)
        w.pairs.append((a, b))
    for a, b in w.pairs:
        extra += [task_of(w, a, rng), task_of(w, b, rng)]
    # scattered over the array, with padding records singly, in runs of 63 and at the end
    order = rng.permutation(len(extra))
    none = dict(read=TASK_NONE, chrono=0, sidx=0, qp=0, dp=0, L=0, qfwd=0, qbwd=0, score=0, nmatch=0)
    for k, e in enumerate(order):
        w.tasks.append(extra[e])
        if k % 700 == 5:
            w.tasks.append(dict(none))
        if k % 2100 == 9:
            w.tasks += [dict(none) for _ in range(63)]
    w.tasks += [dict(none) for _ in range(17)]


def _mix_np(h):
    h = h * np.uint64(K1)
    h = h ^ (h >> np.uint64(29))
    h = h * np.uint64(K2)
    return h ^ (h >> np.uint64(32))


def equal_tag_pairs(w, want):
    """Pairs of legal, different segments whose hashes agree in bits 27 - 63 (the tag) and 0 - 15 (the slot at either table size):
    the hash of a legal segment with bits 16 - 26 changed, inverted, and kept where the word decodes to a legal segment - bits 11, 31
    and 56 - 63 clear, a frame below 6, a read of the world, 0 <= qs < qe within the frame, the segment inside its subject.  Bits
    12 - 30 hold sidx ^ ds << 8: the subject's low 8 bits are given, its upper bits are tried and decide the low 7 bits of ds."""
    rng = w.rng
    nsub = len(w.subjects)
    dlen = np.array([len(s) for s in w.subjects])
    pairs = []
    flips = np.arange(1, 2048, dtype=np.uint64) << np.uint64(16)
    for _ in range(40):
        if len(pairs) >= want:
            break
        m = 1024
        sidx = rng.integers(0, nsub, m); frame = rng.integers(0, 6, m); qs = rng.integers(0, 100, m); read = rng.integers(0, NREADS, m)
        n = np.minimum(rng.integers(1, 61, m), dlen[sidx])
        ds = (rng.random(m) * (dlen[sidx] - n + 1)).astype(np.int64)
        word = np.array([seg_word(*t) for t in zip(read.tolist(), sidx.tolist(), frame.tolist(), qs.tolist(), ds.tolist(), (qs + n).tolist())], np.uint64)
        x = _unmix_np((_mix_np(word)[:, None] ^ flips[None, :]))
        u = np.uint64
        ok = ((x >> u(56)) == 0) & (((x >> u(31)) & u(1)) == 0) & (((x >> u(11)) & u(1)) == 0) & ((x & u(7)) < 6) & (((x >> u(32)) & u(0xFFFF)) < NREADS)
        for i, j in zip(*np.nonzero(ok)):
            xv = int(x[i, j])
            a = (int(read[i]), int(sidx[i]), int(frame[i]), int(qs[i]), int(ds[i]), int(qs[i] + n[i]))
            fr, qe, rd, q2 = xv & 7, (xv >> 3) & 0xFF, (xv >> 32) & 0xFFFF, (xv >> 48) & 0xFF
            if not q2 < qe <= QLEN[fr]:
                continue
            v = (xv >> 12) & 0x7FFFF
            for hi in range((nsub >> 8) + 1):
                s2, d2 = (v & 0xFF) | (hi << 8), (((v >> 8) & 0x7F) ^ hi) | ((v >> 15) << 7)
                if s2 < nsub and d2 + (qe - q2) <= dlen[s2]:
                    b = (rd, s2, fr, q2, d2, qe)
                    ha, hb = mix(seg_word(*a)), mix(seg_word(*b))
                    assert hb >> 27 == ha >> 27 and hb & 0xFFFF == ha & 0xFFFF and b != a
                    pairs.append((a, b))
                    break
    return pairs[:want]


_world = []


def world():
    if not _world:
        _world.append(build_world())
    return _world[0]


# ---- what the oracle says about the world --------------------------------------------------------------------------------------------------
def flank_class(f):
    """The classes a designed flank belongs to: its builder's, and those the oracle's width, runs and rows put it in."""
    o = dict(zip(ORACLE_NAMES, f["o"]))
    out = [f["cls"]] if f["cls"] not in ("runs", "wide") else []
    if f["cls"] == "runs":
        out += [n for n, lo, hi in RUN_CLASSES if lo <= o["runs"] <= hi]
    if f["cls"] == "wide":
        out += [n for n, lo, hi in WIDTH_CLASSES if lo <= o["width"] <= hi]
    return out


def populations(w):
    pop = {}
    for f in w.flanks:
        for c in flank_class(f):
            pop[c] = pop.get(c, 0) + 1
    return pop


def segment_results(w):
    """Per distinct segment of the task array: the oracle's numbers of its (right, left) flank, None where the side is not extended."""
    if not hasattr(w, "_seg_results"):
        res = {}
        for t in w.tasks:
            if t["read"] != TASK_NONE:
                seg = w.segment(t)
                if seg not in res:
                    res[seg] = tuple(None if fl is None else oracle(*fl) for fl in w.seg_flanks(seg))
        w._seg_results = res
    return w._seg_results


# ---- the host statements of the extension (tests/emul/gapped_win.cpp) -----------------------------------------------------------------------
WIN_SRC = os.path.join(oc.EMUL, "gapped_win.cpp")


def build_host_forms(tmp, flags=("-O2",)):
    exe = str(tmp / "gapped_win")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-o", exe, WIN_SRC])
    return exe


def host_forms(exe, flanks, tmp):
    """gapped_win on flanks (dicts with q, s in walking order and side): ((flanks, 3, 9) int32 - gain, c1, c2, ident, steps, runs,
    gapcols, overflow, ovf of the full-size form and of the windows MC_GAP_WIN and MC_GAP_WIN2 - and the program's stderr)."""
    o1, q = oc.pack([f["q"] for f in flanks], np.uint8)
    o2, s = oc.pack([f["s"] for f in flanks], np.uint8)
    oc.write_sections(tmp / "flanks.in", [o1, q, o2, s, np.array([1 if f["side"] == 0 else -1 for f in flanks], np.int8)])
    p = subprocess.run([exe, str(tmp / "flanks.in"), str(tmp / "flanks.out"), str(WIN), str(WIN2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.frombuffer(oc.read_sections(tmp / "flanks.out")[0], "<i4").reshape(len(flanks), 3, 9), p.stderr


def item_pool(w):
    """Every flank the DP launches can be given: the designed ones first, then both sides of the other tasks (the members of a group
    are items of their own with one flank).  dict(item, q, s, side, o, cls) each."""
    if not hasattr(w, "_pool"):
        pool = [dict(item=2 * f["task"] + f["side"], q=f["q"], s=f["s"], side=f["side"], o=f["o"], cls=f["cls"]) for f in w.flanks]
        res = segment_results(w)
        for p in range(w.nflank_tasks, len(w.tasks)):
            t = w.tasks[p]
            if t["read"] == TASK_NONE:
                continue
            seg = w.segment(t)
            for side, fl in enumerate(w.seg_flanks(seg)):
                if fl is not None:
                    pool.append(dict(item=2 * p + side, q=fl[0], s=fl[1], side=side, o=res[seg][side], cls="member"))
        w._pool = pool
    return w._pool


# ---- a read set for the product library whose flanks leave the 64-column window by width -----------------------------------------------------
WITNESS_ANCHOR = 30


def wide_witness(nreads=6, width=70):
    """(names, subjects as letters, reads (n x 510 bases)): read k is the back-translation of 30 residues shared with subject k - the
    seeds and the ungapped segment - and a query flank of 140 residues whose band against the rest of the subject is `width` columns
    wide or wider by the oracle.  The flanks begin with W against D, N, P (-12 together): the ungapped X-drop extension ends on the
    shared residues, so the gapped extension starts where the flank was designed to start.  The climb of climbs_for_widths, with
    those three pairs left alone."""
    rng = np.random.default_rng(64)
    n1 = QLEN[0] - WITNESS_ANCHOR
    stop_q, stop_s = [W_] * 3, [AA.index(c) for c in "DNP"]
    names, subjects, reads = [], [], []
    for _ in range(200):
        if len(reads) == nreads:
            break
        n2, per = int(rng.integers(250, 500)), int(rng.integers(10, 16))
        u = rng.integers(0, 20, per).astype(np.uint8)
        q, s = np.tile(u, 20)[:n1].copy(), np.tile(u, 60)[:n2].copy()
        m = rng.random(n2) < 0.3
        s[m] = rng.integers(0, 20, int(m.sum()))
        q[:3], s[:3] = stop_q, stop_s
        o, stall = oracle(q, s), 0
        while stall < 300 and not (o[7] >= width and o[0] > 0):
            q2, s2 = q.copy(), s.copy()
            for _ in range(int(rng.integers(1, 4))):
                if rng.random() < 0.4:
                    q2[rng.integers(3, n1)] = rng.integers(0, 20)
                else:
                    s2[rng.integers(3, n2)] = rng.integers(0, 20)
            o2 = oracle(q2, s2)
            stall = 0 if o2[7] > o[7] else stall + 1
            if o2[7] >= o[7]:
                q, s, o = q2, s2, o2
        if o[7] >= width and o[0] > 0:
            anchor = rng.permutation(20)[:WITNESS_ANCHOR % 20].tolist() + rng.permutation(20).tolist()      # 30 residues, no repeat within 10
            prot = "".join(AA[x] for x in anchor + q.tolist())
            names.append("wide%d" % len(reads))
            subjects.append("".join(AA[x] for x in anchor + s.tolist()))
            reads.append(np.frombuffer("".join(sc.CODON[a] for a in prot).encode(), np.uint8))
    assert len(reads) == nreads
    return names, subjects, np.stack(reads)
