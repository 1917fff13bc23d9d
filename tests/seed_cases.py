"""Inputs of the seed stage's unit tests (test_seeds_host.py on the CPU, test_gpu_seeds_units.py on the device), and the oracle's side of
every comparison: rs_extend_hit() and rs_seed_ranges() of oracle/rapsearch_port.c through ctypes - the body of ExtendSeq2Set's posting
loop with the two ungapped walks of AlignSeqs, and the ranges Searching hands to ExtendSeq2Set, the pieces rs_search_read itself runs.

One WORLD, built once per process by seeded numpy: synthetic frames (nreads x 6 x FP dense codes, MC_INV behind a frame's length),
subjects (letters, as the index builder reads them) and seed hits (read, frame, qpos, sidx, dpos, seedlen, nkey).  Every hit is a legal
state of the pipeline: its seed matches by reduced-alphabet group over seedlen residues (as far as the subject reaches) - 9 / 3 exact,
10 / 4 with one substitution at seed offset 3 .. 6, or the generic form's 6 .. 9 with nkey = seedlen - 6 - indices are in range and
(sidx, dpos) is a posting of the index built on the subjects; the harnesses check that again before they launch anything.

A hit is made from a template: the query's row and a subject laid on one diagonal, the columns (query residue, subject residue) given
outwards from the seed by score and group - what is not given is drawn at random.  What class a hit belongs to is never taken from the
template: the oracle's answer decides, and for what happens inside a walk (which the oracle does not report) a plain restatement of
AlignFwd / AlignBwd here, which classify() holds to the oracle's extents, score and identities on every hit."""
import ctypes as C
import os

import numpy as np

import gapped_cases as gc
import order_cases as oc
import seg_cases as sc

MC_INV = sc.MC_INV
L_NT = gc.L_NT
FP = gc.FP
QLEN = gc.QLEN
AA = gc.AA
TASK_NONE = 0xFFFFFFFF
NREADS = 640
DENSE_TO_ORACLE = gc.DENSE_TO_ORACLE
EV_GROUP = oc.define("MC_EV_GROUP", "k_eval_seeds.h")                  # 16
EV_BPC = oc.define("MC_EV_BPC", "k_eval_seeds.h")                      # 5
STATIC_RECORDS = 256 * EV_BPC * 4 * EV_GROUP * 64                      # what the waves of k_eval_seeds take by their number: 5,242,880


def _enum(names):
    """The places of counters in mc_hip_common.h's enum (C_TASKS = 0 first, one name after the other)."""
    import re
    text = open(os.path.join(oc.CSRC, "mc_hip_common.h")).read()
    body = re.search(r"enum\s*\{\s*C_TASKS\b(.*?)\}", text, re.S).group(0)
    body = re.sub(r"//[^\n]*", "", body)
    order = [t.strip().split("=")[0].strip() for t in body[body.index("{") + 1:body.rindex("}")].split(",") if t.strip()]
    return [order.index(n) for n in names], len(order) - (1 if order[-1] == "C_N" else 0)


(C_TASKS, C_GAPS, C_HSPS, C_OVERFLOW, C_EVCHUNK, C_HPAD, C_GPAD), C_N = _enum(("C_TASKS", "C_GAPS", "C_HSPS", "C_OVERFLOW", "C_EVCHUNK", "C_HPAD", "C_GPAD"))

B62 = np.array([  # order ARNDCQEGHILKMFPSTWYV (the matrix of the BLAST distribution)
    [4, -1, -2, -2, 0, -1, -1, 0, -2, -1, -1, -1, -1, -2, -1, 1, 0, -3, -2, 0],
    [-1, 5, 0, -2, -3, 1, 0, -2, 0, -3, -2, 2, -1, -3, -2, -1, -1, -3, -2, -3],
    [-2, 0, 6, 1, -3, 0, 0, 0, 1, -3, -3, 0, -2, -3, -2, 1, 0, -4, -2, -3],
    [-2, -2, 1, 6, -3, 0, 2, -1, -1, -3, -4, -1, -3, -3, -1, 0, -1, -4, -3, -3],
    [0, -3, -3, -3, 9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1],
    [-1, 1, 0, 0, -3, 5, 2, -2, 0, -3, -2, 1, 0, -3, -1, 0, -1, -2, -1, -2],
    [-1, 0, 0, 2, -4, 2, 5, -2, 0, -3, -3, 1, -2, -3, -1, 0, -1, -3, -2, -2],
    [0, -2, 0, -1, -3, -2, -2, 6, -2, -4, -4, -2, -3, -3, -2, 0, -2, -2, -3, -3],
    [-2, 0, 1, -1, -3, 0, 0, -2, 8, -3, -3, -1, -2, -1, -2, -1, -2, -2, 2, -3],
    [-1, -3, -3, -3, -1, -3, -3, -4, -3, 4, 2, -3, 1, 0, -3, -2, -1, -3, -1, 3],
    [-1, -2, -3, -4, -1, -2, -3, -4, -3, 2, 4, -2, 2, 0, -3, -2, -1, -2, -1, 1],
    [-1, 2, 0, -1, -3, 1, 1, -2, -1, -3, -2, 5, -1, -3, -1, 0, -1, -3, -2, -2],
    [-1, -1, -2, -3, -1, 0, -2, -3, -2, 1, 2, -1, 5, 0, -2, -1, -1, -1, -1, 1],
    [-2, -3, -3, -3, -2, -3, -3, -3, -1, 0, 0, -3, 0, 6, -4, -2, -2, 1, 3, -1],
    [-1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4, 7, -1, -1, -4, -3, -2],
    [1, -1, 1, 0, -1, 0, 0, 0, -1, -2, -2, 0, -1, -2, -1, 4, 1, -3, -2, -2],
    [0, -1, 0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1, 1, 5, -2, -2, 0],
    [-3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1, 1, -4, -3, -2, 11, 2, -3],
    [-2, -2, -2, -3, -2, -1, -2, -3, 2, -1, -1, -2, -1, 3, -3, -2, -2, 2, 7, -1],
    [0, -3, -3, -3, -1, -2, -2, -3, -3, 3, 1, -2, 1, -1, -2, -2, 0, -3, -1, 4]])
SUB = np.full((21, 21), -5, np.int64)                                # -5 wherever MC_INV is involved
SUB[:20, :20] = B62
GROUPS = ("A", "KR", "EDNQ", "C", "G", "H", "ILVM", "FYW", "P", "ST")
GRP = np.full(21, 10, np.int64)
for _g, _s in enumerate(GROUPS):
    for _c in _s:
        GRP[AA.index(_c)] = _g
LN2 = 0.6931471805599453
XDROP = (7.0 * LN2 - 2.0099154790312257) / 0.318                     # 8.94: the walk goes on at a drop of 8 and stops at 9
XFLOOR = int(np.floor(XDROP))
GAP_TRIGGER = (25.0 * LN2 - 2.0099154790312257) / 0.318              # 48.17: 48 stays ungapped, 49 goes to the gapped extension
TRIG = int(np.ceil(GAP_TRIGGER))
# column kinds: pairs of dense codes by (score, same group?)
PAIRS = {}
for _a in range(20):
    for _b in range(20):
        PAIRS.setdefault((int(SUB[_a, _b]), bool(GRP[_a] == GRP[_b]), _a == _b), []).append((_a, _b))


class RsHit(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("why", "qp", "dp", "L", "seed_score", "seed_ident", "qfwd", "qbwd", "score", "nmatch", "gapped", "kept",
                                          "qaas", "qaae", "ds", "de", "qnts", "qnte", "alnlen", "mism")] + [("loge", C.c_double)]


class RsRange(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pos", "bucket", "seedlen", "nkey", "nst", "ned", "phase")]


EXTENDED, PAST_END, REDUNDANT, GATE = 0, 1, 2, 3
HIT_FIELDS = tuple(n for n, _ in RsHit._fields_)


def lib():
    l = sc.oracle_lib()
    if not hasattr(l, "_seeds_ready"):
        l.rs_db_load_rapdb.restype = C.c_void_p
        l.rs_db_load_rapdb.argtypes = [C.c_char_p]
        l.rs_db_postings.restype = C.POINTER(C.c_uint32)
        l.rs_db_postings.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        l.rs_db_bucket_starts.restype = C.POINTER(C.c_int64)
        l.rs_db_bucket_starts.argtypes = [C.c_void_p]
        l.rs_db_keys.restype = C.POINTER(C.c_uint16)
        l.rs_db_keys.argtypes = [C.c_void_p]
        l.rs_extend_hit.restype = C.c_int
        l.rs_extend_hit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RsHit)]
        l.rs_seed_ranges.restype = C.c_int
        l.rs_seed_ranges.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(RsRange), C.c_int]
        l._seeds_ready = True
    return l


def letters_of(subjects):
    """The subjects as the index builder reads them: letters, every letter it turns into MC_INV in turn - but for '/', which the
    reference codes as a residue of its own (the group string "S/T"): a subject with it is not a case of this set."""
    table = np.frombuffer((AA + "X").encode(), np.uint8)
    off, res = oc.pack(subjects, np.uint8)
    text = table[res].copy()
    inv = np.flatnonzero(res == MC_INV)
    odd = np.frombuffer(gc.ODD.replace("/", "").encode(), np.uint8)
    text[inv] = odd[np.arange(len(inv)) % len(odd)]
    return off, text


class Db:
    """The oracle's database of a list of subjects (dense codes): the library's writer of prerapsearch's format makes the file - held
    byte for byte to prerapsearch's own by tests/test_rapdb.py - and rs_db_load_rapdb reads it."""

    def __init__(self, subjects, tmp):
        from microbecensus_amd import _native
        off, text = letters_of(subjects)
        seqs = [text[off[k]:off[k + 1]].tobytes().decode() for k in range(len(subjects))]
        path = os.path.join(str(tmp), "seeds_db")
        _native.rapdb_write(["s%d" % k for k in range(len(seqs))], seqs, path)
        self.h = lib().rs_db_load_rapdb(path.encode())
        assert self.h
        n = C.c_int64()
        p = lib().rs_db_postings(self.h, C.byref(n))
        self.post = np.ctypeslib.as_array(p, (n.value,)).copy()
        self.bstart = np.ctypeslib.as_array(lib().rs_db_bucket_starts(self.h), (1000001,)).copy()
        self.index_of = {int(v): k for k, v in enumerate(self.post)}

    def extend(self, row, qlen, frame, qpos, sidx, dpos, seedlen, nkey):
        """rs_extend_hit on one hit of subject sidx: dict of the oracle's answer."""
        out = RsHit()
        lib().rs_extend_hit(self.h, L_NT, frame, sidx, DENSE_TO_ORACLE[row[:qlen]].tobytes(), qlen, qpos, None, 0, dpos, seedlen, nkey, C.byref(out))
        return {n: getattr(out, n) for n in HIT_FIELDS}

    def ranges(self, row, qlen, frame, cap=1 << 16):
        """rs_seed_ranges on one frame: list of (pos, bucket, seedlen, nkey, nst, ned, phase)."""
        buf = (RsRange * cap)()
        n = lib().rs_seed_ranges(self.h, frame, DENSE_TO_ORACLE[row[:qlen]].tobytes(), qlen, buf, cap)
        assert n <= cap
        return [(r.pos, r.bucket, r.seedlen, r.nkey, r.nst, r.ned, r.phase) for r in buf[:n]]


# ---- AlignFwd / AlignBwd once more, step by step: what happens inside a walk -------------------------------------------------------------
def walk(a, b, s0):
    """The reference's walk over the columns (a[i], b[i]) in walking order from the score s0.  Returns dict(bl, gain, id, steps: the
    columns walked, end: 'none' (no column), 'limit', 'xdrop' or 'floor' (run < -20), drops: best - run behind every step)."""
    lim = min(len(a), len(b))
    run = best = s0
    bl = bi = idn = 0
    drops, end = [], "none"
    for i in range(lim):
        run += int(SUB[a[i], b[i]]); idn += int(a[i] == b[i])
        if run > best:
            best, bl, bi = run, i + 1, idn
        drops.append(best - run)
        if i + 1 >= lim:
            end = "limit"; break
        if run < -20:
            end = "floor"; break
        if run < best - XDROP:
            end = "xdrop"; break
    return dict(bl=bl, gain=best - s0, id=bi, steps=len(drops), end=end, drops=drops, lim=lim)


def would_raise(a, b, s0, w, upto):
    """Had the walk not stopped behind step w['steps']: would columns steps .. upto - 1 have raised best?"""
    run = s0 + w["gain"] - w["drops"][-1]
    best = s0 + w["gain"]
    for i in range(w["steps"], min(upto, w["lim"])):
        run += int(SUB[a[i], b[i]])
        if run > best:
            return True
    return False


# ---- the world ------------------------------------------------------------------------------------------------------------------------------
def P(score, same_group=False, ident=False):
    return PAIRS[(score, same_group or ident, ident)]


class World:
    def __init__(self):
        self.rng = np.random.default_rng(20261021)
        self.frames = self.rng.integers(0, 20, (NREADS, 6, FP)).astype(np.uint8)
        for f in range(6):
            self.frames[:, f, QLEN[f]:] = MC_INV
        self.subjects = []
        self.hits = []                                               # dict(read, frame, qpos, sidx, dpos, seedlen, nkey, cls: the template's name)
        self.slot = 6                                                # (read 0 is laid out by hand)

    def pick(self, pairs):
        return pairs[int(self.rng.integers(0, len(pairs)))]

    def col(self, kind):
        """A column (query residue, subject residue) of a kind: an int score of a pair of different groups, 'I' identical, 'I<n>' identical
        with score n, 'G' same group but not identical, 'Xq' / 'Xd' / 'Xx' MC_INV on the query's side, the subject's, both; a pair as it is."""
        if isinstance(kind, tuple):
            return kind
        if isinstance(kind, int):
            return self.pick(P(kind))
        if kind == "I":
            x = int(self.rng.integers(0, 20)); return (x, x)
        if kind[0] == "I":
            return self.pick(P(int(kind[1:]), ident=True))
        if kind == "G":
            return self.pick([p for (s, g, i), v in PAIRS.items() if g and not i for p in v])
        x = int(self.rng.integers(0, 20))
        return {"Xq": (MC_INV, x), "Xd": (x, MC_INV), "Xx": (MC_INV, MC_INV)}[kind]

    def next_row(self, frame=None):
        while frame is not None and self.slot % 6 != frame:
            self.slot += 1
        read, fr = divmod(self.slot, 6)
        self.slot += 1
        assert read < NREADS
        return read, fr

    def template(self, cls, seed, fwd=(), bwd=(), qpos=40, dpos=40, dlen=None, frame=None, dtail=None):
        """A hit whose seed's columns are `seed` (kinds), with the columns `fwd` behind it and `bwd` in front of it (outwards).  The seed
        stands at qpos in the frame and at dpos in the subject; the subject has dlen residues (default: it reaches 30 residues past the
        frame on both sides where it can).  dtail: the subject ends dtail residues behind the seed's first one."""
        read, fr = self.next_row(frame)
        qlen = QLEN[fr]
        q = self.frames[read, fr]
        n = len(seed)
        if dtail is not None:
            dlen = dpos + dtail
        if dlen is None:
            dlen = dpos + (qlen - qpos) + 30
        self.subjects.append(self.rng.integers(0, 20, dlen).astype(np.uint8))
        sidx = len(self.subjects) - 1
        d = self.subjects[sidx]
        cols = [self.col(k) for k in seed]
        for k, (a, b) in enumerate(cols):
            if qpos + k < qlen: q[qpos + k] = a
            if dpos + k < dlen: d[dpos + k] = b
        for k, kind in enumerate(fwd):
            a, b = self.col(kind)
            if qpos + n + k < qlen: q[qpos + n + k] = a
            if dpos + n + k < dlen: d[dpos + n + k] = b
        for k, kind in enumerate(bwd):
            a, b = self.col(kind)
            if qpos - 1 - k >= 0: q[qpos - 1 - k] = a
            if dpos - 1 - k >= 0: d[dpos - 1 - k] = b
        self.hits.append(dict(read=read, frame=fr, qpos=qpos, sidx=sidx, dpos=dpos, seedlen=n, nkey=4 if n == 10 else n - 6, cls=cls))
        return len(self.hits) - 1


STRONG9 = ["I6", "I5", "I4", "I7", "I5", "I4", "I6", "I5", "I4"]       # nine identical residues: 46
STOP = -4                                                             # a column that ends growth: different groups


def seed10(at, rest="I"):
    """Ten columns, identical but for one substitution between groups at seed offset `at`."""
    return [rest if k != at else -1 for k in range(10)]


def other_group(rng, x):
    """A residue of another group than x's that scores below 0 against it."""
    c = [y for y in range(20) if GRP[y] != GRP[x] and SUB[x, y] < 0]
    return c[int(rng.integers(0, len(c)))]


def build_world():
    w = World()
    rng = w.rng
    # ---- read 0, frame 0 and subject 0: grown seeds that begin at 0 .. 8 of the first row of the frames and of the first subject of the
    # residue array (the backward walk's 8-byte loads reach into the room in front of both).  Nine subjects share the row's first
    # residues, nine rows the subject's: the residue in front of the seed differs in group (a 9-mer is not redundant, growth ends),
    # the ones in front of that are identical - the walk goes to the row's / the subject's first residue.
    w.subjects.append(rng.integers(0, 20, 120).astype(np.uint8))
    row0, sub0 = w.frames[0, 0], w.subjects[0]
    for k in range(9):
        d = rng.integers(0, 20, 140).astype(np.uint8)
        d[60 - k:69] = row0[:k + 9]
        if k: d[59] = other_group(rng, row0[k - 1])
        d[69] = other_group(rng, row0[k + 9])
        w.subjects.append(d)
        w.hits.append(dict(read=0, frame=0, qpos=k, sidx=len(w.subjects) - 1, dpos=60, seedlen=9, nkey=3, cls="first_row"))
        read, fr = w.next_row()
        q = w.frames[read, fr]
        q[60 - k:69] = sub0[:k + 9]
        if k: q[59] = other_group(rng, sub0[k - 1])
        q[69] = other_group(rng, sub0[k + 9])
        w.hits.append(dict(read=read, frame=fr, qpos=60, sidx=0, dpos=k, seedlen=9, nkey=3, cls="first_subject"))
    # ---- growth: forward to 9 .. 18 and more, backward by 0 .. 10 and more, ended by a mismatch
    for f in range(0, 12):
        for b in range(0, 12):
            w.template("growth", seed10(3 + (f + b) % 4), fwd=["G" if (k + f) % 3 == 0 else "I" for k in range(f)] + [STOP], bwd=["I" if (k + b) % 4 else "G" for k in range(b)] + [STOP])
    for f in range(0, 12):
        w.template("growth9", ["I"] * 9, fwd=["I"] * f + [STOP], bwd=[STOP])
    # ... ended by the frame's end and by the subject's end, forward
    for f in (0, 1, 5, 6, 7, 8, 9, 12):
        for fr in (0, 1):
            qlen = QLEN[fr]
            w.template("growth_frame_end", ["I"] * 9, fwd=["I"] * f, bwd=[STOP], qpos=qlen - 9 - f, dpos=30, frame=fr)
            w.template("growth_subject_end", ["I"] * 9, fwd=["I"] * (f + 3), bwd=[STOP], qpos=50, dpos=30, dtail=9 + f)
            w.template("growth_both_end", ["I"] * 9, fwd=["I"] * f, bwd=[STOP], qpos=qlen - 9 - f, dpos=30, dtail=9 + f, frame=fr)
    # ... backward (10-mers: a 9-mer whose residue in front matches is redundant)
    for b in (0, 1, 6, 7, 8, 9, 10, 12):
        w.template("growth_frame_start", seed10(4), fwd=[STOP], bwd=["I"] * 14, qpos=b, dpos=40)
        w.template("growth_subject_start", seed10(5), fwd=[STOP], bwd=["I"] * 14, qpos=40, dpos=b)
        w.template("growth_both_start", seed10(6), fwd=[STOP], bwd=["I"] * 14, qpos=b, dpos=b)
    # ---- the generic form's seeds of 6 .. 9 residues, grown to 9 and beyond or stopped short of it
    NINE = ["I6", "I5", "I7", "I6", "I5", "I4", "I5", "I4", "I6"]
    for n in (6, 7, 8, 9):
        for f in range(0, 13):
            w.template("generic", NINE[:n], fwd=["I"] * f + [STOP], bwd=[STOP])
        for tail in range(max(n, 7), n + 5):                          # (a subject's last six residues are no posting)
            w.template("generic_tail", NINE[:n], fwd=["I"] * 8, bwd=[STOP], dtail=tail)
    # ---- redundant and past the end
    for n in (9, 10, 7):
        w.template("redundant", (["I"] * 10)[:n], fwd=[STOP], bwd=["G"])
        w.template("redundant", (["I"] * 10)[:n], fwd=[STOP], bwd=["I"], qpos=0)
        w.template("redundant", (["I"] * 10)[:n], fwd=[STOP], bwd=["I"], dpos=0)
        for tail in range(7, n):
            w.template("past_end", (["I"] * 10)[:n], bwd=[STOP], dtail=tail)
    # ---- the gate: seed scores 9 .. 13 and 2 .. 5 identities, 9-mers and 10-mers with their substitution, as far as BLOSUM62 has them (a
    # pair of one group never scores below 0 and an identical one never below 4: a legal hit with 4 identities scores 12 at least - the
    # score bar decides nothing that the identities have not decided)
    for s in (9, 10, 11, 12, 13):
        for ids in (2, 3, 4, 5):
            for ten in (False, True):
                for _ in range(200):
                    cols = [w.col(k) for k in ["I4"] * ids + ["G"] * (9 - ids)]
                    if ten: cols.insert(3 + (s + ids) % 4, w.col(-4 + (s % 2)))
                    if sum(int(SUB[a, b]) for a, b in cols) == s:
                        order = rng.permutation(9)               # (a 10-mer keeps its columns where they are: the substitution stands at offset 3 .. 6)
                        w.template("gate", cols if ten else [cols[k] for k in order], fwd=[STOP], bwd=[STOP])
                        break
    for ids in (3, 4):                                               # ... and high scores with few identities: W, Y, F among each other
        for _ in range(6):
            cols = [w.pick(P(11, ident=True)) for _ in range(ids)] + [w.pick(P(3, True) + P(2, True) + P(1, True)) for _ in range(9 - ids)]
            w.template("gate", [cols[k] for k in rng.permutation(9)], fwd=[STOP], bwd=[STOP])
    # ---- the walks.  Forward: a 9-mer of 46 whose growth ends at once on both sides; the walk's columns follow the column that ended
    # growth.  The limit min(n1, n2), ended by the frame, by the subject, by both - and the residues behind the subject's end (the next
    # subject's first ones) identical to the frame's, the residues in front of its start (the last ones of the subject before) likewise
    LIMS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
    for lim in LIMS + ("longest",):
        for who in ("frame", "subject", "both"):
            for fill in ("I", "mixed"):
                fr = int(rng.integers(0, 6))
                qlen = QLEN[fr]
                n = qlen - 9 if lim == "longest" else lim
                cols = [STOP] + ["I"] * (n + 8) if fill == "I" else [STOP] + [("I", -1, "I", "G", -2, "I")[int(rng.integers(0, 6))] for _ in range(n + 8)]
                # forward
                qpos = qlen - 9 - n if who in ("frame", "both") else max(0, qlen - 9 - n - 20)
                dt = 9 + n if who in ("subject", "both") else 9 + n + 20
                k = w.template("walk_fwd_%s" % who, STRONG9, fwd=cols, bwd=[STOP], qpos=qpos, dpos=30 if qpos else 0, dtail=dt, frame=fr)
                if who == "frame" and w.slot < NREADS * 6:           # the subject goes on behind the frame's end as the next row of the frames does
                    h, nxt = w.hits[k], w.frames.reshape(-1, FP)[w.slot]     # (w.slot: the row after this template's)
                    at = h["dpos"] + 9 + n + (FP - qlen)
                    w.subjects[h["sidx"]][at:at + 8] = nxt[:8]
                if who == "subject":                                 # the next subject goes on where this one ends, as the frame does
                    a = w.frames[w.hits[k]["read"], fr][qpos + 9 + n:qpos + 9 + n + 12]
                    w.subjects.append(np.concatenate([a, rng.integers(0, 20, 20)]).astype(np.uint8))
                # backward
                qpos = n if who in ("frame", "both") else n + 20
                dpos = n if who in ("subject", "both") else n + 20
                if qpos + 9 <= qlen:
                    if who == "subject":                             # the subject in front ends as the frame goes on towards its start
                        w.subjects.append(rng.integers(0, 20, 32).astype(np.uint8))
                    k = w.template("walk_bwd_%s" % who, STRONG9, fwd=[STOP], bwd=cols, qpos=qpos, dpos=dpos, frame=fr)
                    if who == "frame":                               # ... and in front of the frame's start as the row before does
                        h = w.hits[k]
                        fp = (fr - 1) % 6
                        prv = w.frames.reshape(-1, FP)[h["read"] * 6 + fr - 1]
                        at = dpos - n - (FP - QLEN[fp])
                        w.subjects[h["sidx"]][at - 8:at] = prv[QLEN[fp] - 8:QLEN[fp]]
                    if who == "subject":
                        w.subjects[w.hits[k]["sidx"] - 1][-12:] = w.frames[w.hits[k]["read"], fr][qpos - dpos - 12:qpos - dpos]
    # ... the drop: best - run reaches exactly floor(xdrop) (the walk goes on) or floor(xdrop) + 1 (it stops) at each of the eight places
    # of a turn; behind it a stretch that would raise best - in the same turn, in the next one; a return to exactly best
    for side in ("fwd", "bwd"):
        for lead in range(0, 17):                                    # identical residues in front of the drop: the drop's place in the turn
            for parts in ((-4, -4), (-3, -3, -2), (-4, -4, -1), (-3, -3, -3), (-4, -3, -3), ("Xq", -4), (-4, "Xd")):
                for then in (["I11"] * 3, ["I4"] * 8 + ["I11"] * 3, [-4] * 12):
                    cols = [STOP] + ["I5"] * (lead + 1) + list(parts) + then + [-4] * 4
                    if side == "fwd":
                        w.template("drop_fwd", STRONG9, fwd=cols, bwd=[STOP], qpos=20, dpos=25)
                    else:
                        w.template("drop_bwd", STRONG9, fwd=[STOP], bwd=cols, qpos=60, dpos=70)
        for lead in range(0, 9):                                     # back to exactly best: - 4 + 4 (A / A) twice, then down
            cols = [STOP] + ["I5"] * (lead + 1) + [-4, "I4", -4, "I4", -3, -3, -3, -3]
            w.template("tie_" + side, STRONG9, fwd=cols if side == "fwd" else [STOP], bwd=[STOP] if side == "fwd" else cols, qpos=50, dpos=55)
    # ... MC_INV inside a walk on either side
    for k in range(16):
        cols = [STOP] + [("I", "I", "Xq", "I", "Xd", "I", "I", "Xx")[(j + k) % 8] for j in range(20)]
        w.template("inv", STRONG9, fwd=cols if k % 2 else [STOP], bwd=[STOP] if k % 2 else cols, qpos=60, dpos=70)
    # ---- the outcome: final scores around the gapped trigger (46 + what the walk gains), around CalRes' bar of 30, the same place twice
    for x in (4, 5, 6, 7, 8, 9, 11):
        for side in ("fwd", "bwd"):
            cols = [-4, "I%d" % x] + [-4] * 4
            w.template("trigger", STRONG9, fwd=cols if side == "fwd" else [STOP], bwd=[STOP] if side == "fwd" else cols)
    for s in range(26, 36):
        for _ in range(400):
            low = int(rng.integers(0, 7))
            cols = [w.col("I4") for _ in range(low)] + [w.col("I") for _ in range(6 - low)] + [w.col("G") for _ in range(3)]
            if sum(int(SUB[a, b]) for a, b in cols) == s:
                w.template("bar30", [cols[k] for k in rng.permutation(9)], fwd=[STOP, STOP, STOP], bwd=[STOP, STOP, STOP])
                break
    for k in range(6):                                               # two 10-mers a residue apart around one substitution grow to the same eleven residues: one place
        a = w.template("same_place", ["I4"] * 4 + [-1] + ["I4"] * 5, fwd=["I4", STOP, STOP, STOP], bwd=[STOP] * 3, qpos=40 + k, dpos=44)
        w.hits.append(dict(w.hits[a], qpos=41 + k, dpos=45))
    # ---- the last subject: a walk that ends on the last residue of the residue array
    w.template("last_subject", STRONG9, fwd=[STOP] + ["I"] * 11, bwd=[STOP], qpos=20, dpos=30, dtail=21)
    return w


_world = []


def world():
    """The world with its database and the oracle's answer per hit (w.db, w.want)."""
    if not _world:
        w = build_world()
        import tempfile
        w.tmp = tempfile.TemporaryDirectory(prefix="seed_cases")      # (the database's two files; removed with the world)
        w.db = Db(w.subjects, w.tmp.name)
        w.want = [w.db.extend(w.frames[h["read"], h["frame"]], QLEN[h["frame"]], h["frame"], h["qpos"], h["sidx"], h["dpos"], h["seedlen"], h["nkey"]) for h in w.hits]
        _world.append(w)
    return _world[0]


def legal(w, h):
    """The seed matches by group as far as the subject reaches - with one substitution for a 10-mer - and (sidx, dpos) is a posting."""
    q, d = w.frames[h["read"], h["frame"]], w.subjects[h["sidx"]]
    qlen, n = QLEN[h["frame"]], h["seedlen"]
    if not (0 <= h["qpos"] and h["qpos"] + n <= qlen and 0 <= h["dpos"] and h["dpos"] + 6 <= len(d) and 6 <= n <= 10):
        return False
    if h["nkey"] != (4 if n == 10 else n - 6):
        return False
    m = min(n, len(d) - h["dpos"])
    miss = [k for k in range(m) if GRP[q[h["qpos"] + k]] != GRP[d[h["dpos"] + k]] or GRP[q[h["qpos"] + k]] == 10]
    if not (miss == [] or (n == 10 and len(miss) == 1 and 3 <= miss[0] <= 6)):
        return False
    return ((h["sidx"] << 11) | h["dpos"]) in w.db.index_of


# ---- what the oracle says about the world --------------------------------------------------------------------------------------------------
def classify(w, k):
    """The classes of hit k, from the oracle's answer and the walk restated (held to the oracle's answer here)."""
    h, o = w.hits[k], w.want[k]
    out = [("dropped_past_end", "dropped_redundant", "dropped_gate")[o["why"] - 1]] if o["why"] else ["extended"]
    if o["why"] in (PAST_END, REDUNDANT):
        return out
    q, d = w.frames[h["read"], h["frame"]], w.subjects[h["sidx"]]
    qlen, dlen = QLEN[h["frame"]], len(d)
    back = h["qpos"] - o["qp"]
    fl = o["L"] - back                                               # the seed as the forward growth left it
    out.append("seed%d" % h["seedlen"])
    if h["seedlen"] < 9:
        out.append("generic_grown_to_%s" % (fl if fl < 9 else "9" if fl == 9 else "10_up"))
    out.append("grow_fwd_%s" % (fl if fl <= 18 else "19_up"))
    out.append("grow_bwd_%s" % (back if back <= 10 else "11_up"))
    qe, de = h["qpos"] + fl, h["dpos"] + fl
    out.append("grow_fwd_ended_by_" + ("both" if qe == qlen and de == dlen else "frame" if qe == qlen else "subject" if de == dlen else "mismatch"))
    if back or h["nkey"] == 4:
        out.append("grow_bwd_ended_by_" + ("both" if o["qp"] == 0 and o["dp"] == 0 else "frame" if o["qp"] == 0 else "subject" if o["dp"] == 0 else "mismatch"))
    out.append("gate_score_%s" % (o["seed_score"] if 9 <= o["seed_score"] <= 13 else "other"))
    out.append("gate_ident_%s" % (o["seed_ident"] if o["seed_ident"] <= 5 else "6_up"))
    assert o["seed_score"] >= 12 or o["seed_ident"] < 4              # (BLOSUM62: see build_world)
    if o["seed_score"] >= 11 and o["seed_ident"] == 3: out.append("gate_by_ident_alone")
    if o["why"] == GATE:
        return out
    qp, dp, L, s0 = o["qp"], o["dp"], o["L"], o["seed_score"]
    for side in ("fwd", "bwd"):
        if side == "fwd":
            a, b = q[qp + L:qlen], d[dp + L:]
            n1, n2 = qlen - qp - L, dlen - dp - L
        else:
            a, b = q[:qp][::-1], d[:dp][::-1]
            n1, n2 = qp, dp
        wk = walk(a, b, s0)
        assert wk["bl"] == o["q" + side] and wk["end"] != "floor", (k, side, wk, o)
        lim = wk["lim"]
        out.append("%s_lim_%s" % (side, lim if lim in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65) else "longest" if lim >= QLEN[1] - 9 else "other"))
        if wk["end"] == "limit":
            out.append("%s_ended_by_%s" % (side, "both" if n1 == n2 else "frame" if n1 < n2 else "subject"))
            if side == "fwd" and n2 <= n1 and h["sidx"] + 1 < len(w.subjects) and n1 - n2 >= 4 and np.array_equal(w.subjects[h["sidx"] + 1][:4], a[lim:lim + 4]):
                out.append("fwd_next_subject_goes_on")
            if side == "bwd" and n2 <= n1 and h["sidx"] > 0 and n1 - n2 >= 4 and np.array_equal(w.subjects[h["sidx"] - 1][::-1][:4], a[lim:lim + 4]):
                out.append("bwd_subject_in_front_goes_on")
            rows, row = w.frames.reshape(-1, FP), h["read"] * 6 + h["frame"]
            if side == "fwd" and n1 < n2 and row + 1 < len(rows) and n2 - n1 >= FP - qlen + 4 and np.array_equal(b[lim + FP - qlen:lim + FP - qlen + 4], rows[row + 1][:4]):
                out.append("fwd_next_row_goes_on")
            gp = FP - QLEN[(h["frame"] - 1) % 6]
            if side == "bwd" and n1 < n2 and row > 0 and n2 - n1 >= gp + 4 and np.array_equal(b[lim + gp:lim + gp + 4], rows[row - 1][:QLEN[(h["frame"] - 1) % 6]][::-1][:4]):
                out.append("bwd_row_in_front_goes_on")
            if side == "fwd" and n2 <= n1 and h["sidx"] == len(w.subjects) - 1:
                out.append("fwd_ends_on_the_last_residue")
        for i, dr in enumerate(wk["drops"][:-1] if wk["end"] == "xdrop" else wk["drops"]):
            if dr == XFLOOR and i + 1 < lim:
                out.append("%s_drop_floor_goes_on_at_%d" % (side, i % 8))
        if wk["end"] == "xdrop":
            i = wk["steps"] - 1
            if wk["drops"][-1] == XFLOOR + 1:
                out.append("%s_drop_floor1_stops_at_%d" % (side, i % 8))
            if i % 8 != 7 and would_raise(a, b, s0, wk, (i | 7) + 1):
                out.append("%s_stop_then_better_in_the_same_turn" % side)
            elif would_raise(a, b, s0, wk, (i | 7) + 9):
                out.append("%s_stop_then_better_in_the_next_turn" % side)
        run = best = s0
        for i in range(wk["steps"]):
            run += int(SUB[a[i], b[i]])
            if run > best: best = run
            elif run == best and i + 1 > wk["bl"] and best == s0 + wk["gain"] and wk["bl"] > 0:
                out.append("%s_back_to_best" % side); break
        if (a[:wk["steps"]] == MC_INV).any(): out.append("%s_inv_query" % side)
        if (b[:wk["steps"]] == MC_INV).any(): out.append("%s_inv_subject" % side)
        if side == "bwd":
            if h["read"] == 0 and h["frame"] == 0 and qp <= 8: out.append("bwd_first_row_qp_%d" % qp)
            if h["sidx"] == 0 and dp <= 8: out.append("bwd_first_subject_dp_%d" % dp)
    if o["score"] in (TRIG - 1, TRIG): out.append("final_score_%s" % ("trigger" if o["gapped"] else "trigger_minus_1"))
    out.append("to_gapped" if o["gapped"] else "hsp_kept" if o["kept"] else "hsp_dropped")
    if not o["gapped"] and o["score"] in (30, 31): out.append("hsp_score_%d" % o["score"])
    return out


def place(w, k):
    h, o = w.hits[k], w.want[k]
    return (h["read"], h["sidx"], h["frame"], o["qaas"], o["qaae"], o["ds"], o["de"])


def populations(w):
    if not hasattr(w, "_pop"):
        pop, seen = {}, {}
        for k in range(len(w.hits)):
            for c in classify(w, k):
                pop[c] = pop.get(c, 0) + 1
            if w.want[k]["why"] == EXTENDED and w.want[k]["kept"]:
                seen.setdefault(place(w, k), []).append(k)
        pop["same_place_twice"] = sum(len(v) > 1 for v in seen.values())
        w._pop = pop
    return w._pop


REQUIRED = (["dropped_past_end", "dropped_redundant", "dropped_gate", "extended", "seed6", "seed7", "seed8", "seed9", "seed10",
             "generic_grown_to_9", "generic_grown_to_10_up", "gate_by_ident_alone",
             "gate_score_10", "gate_score_11", "gate_score_12", "gate_ident_3", "gate_ident_4",
             "final_score_trigger", "final_score_trigger_minus_1", "to_gapped", "hsp_kept", "hsp_dropped", "hsp_score_30", "hsp_score_31", "same_place_twice",
             "fwd_next_subject_goes_on", "bwd_subject_in_front_goes_on", "fwd_next_row_goes_on", "bwd_row_in_front_goes_on", "fwd_ends_on_the_last_residue"]
            + ["grow_fwd_%d" % v for v in range(9, 19)] + ["grow_bwd_%d" % v for v in range(0, 11)]
            + ["grow_%s_ended_by_%s" % (s, e) for s in ("fwd", "bwd") for e in ("mismatch", "frame", "subject")]
            + ["%s_lim_%s" % (s, v) for s in ("fwd", "bwd") for v in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, "longest")]
            + ["%s_ended_by_%s" % (s, e) for s in ("fwd", "bwd") for e in ("frame", "subject", "both")]
            + ["%s_drop_floor_goes_on_at_%d" % (s, k) for s in ("fwd", "bwd") for k in range(8)]
            + ["%s_drop_floor1_stops_at_%d" % (s, k) for s in ("fwd", "bwd") for k in range(8)]
            + ["%s_%s" % (s, e) for s in ("fwd", "bwd") for e in ("stop_then_better_in_the_same_turn", "stop_then_better_in_the_next_turn", "back_to_best", "inv_query", "inv_subject")]
            + ["bwd_first_row_qp_%d" % k for k in range(9)] + ["bwd_first_subject_dp_%d" % k for k in range(9)])


# ---- seed enumeration: a constructed database and reads given as frames --------------------------------------------------------------------
ENUM_READS = 33
ENUM_LENGTHS = (L_NT, 30)                                             # 510 bases, and the shortest read with a seed of every kind (frames of 10, 9, 9 residues)
RT_LONG = 8                                                           # a first-residue group of more keys than this is answered by the range table (mc_core.h)


def frame_pitch(L):
    return ((L // 3 + 2) + 3) & ~3                                   # (the library's rule: mc_hip.hip, set_len)


def same_group(rng, x):
    g = [y for y in range(20) if GRP[y] == GRP[x]]
    return g[int(rng.integers(0, len(g)))]


class EnumWorld:
    """Subjects: singles (buckets of one posting); a family of 40 copies of one ancestor with substitutions inside and between groups
    (repeated 6-mers with many keys); per size 7 .. 10 a 6-mer followed by one group in that many subjects and by another group in two
    (first-residue groups on either side of RT_LONG); subjects that end 6 .. 9 residues into a segment the reads carry (short keys).
    Reads: see frames()."""

    def __init__(self):
        rng = self.rng = np.random.default_rng(20261022)
        self.subjects = [rng.integers(0, 20, int(rng.integers(40, 300))).astype(np.uint8) for _ in range(40)]
        self.ancestor = rng.integers(0, 20, 400).astype(np.uint8)
        for k in range(40):
            s = self.ancestor[int(rng.integers(0, 30)):400 - int(rng.integers(0, 30))].copy()
            for i in range(len(s)):
                r = rng.random()
                if r < 0.25: s[i] = same_group(rng, s[i])
                elif r < 0.25 + 0.004 * k: s[i] = rng.integers(0, 20)
            if k % 10 == 3: s[int(rng.integers(0, len(s)))] = MC_INV
            self.subjects.append(s)
        self.motifs = []
        for size in (RT_LONG - 1, RT_LONG, RT_LONG + 1, RT_LONG + 2):
            m = rng.integers(0, 20, 6).astype(np.uint8)
            first = int(rng.integers(0, 20))
            second = other_group(rng, first)
            self.motifs.append((m, first, second))
            for k in range(size + 2):
                head = same_group(rng, first) if k < size else same_group(rng, second)
                body = np.concatenate([[same_group(rng, x) for x in m], [head], rng.integers(0, 20, 3)])
                self.subjects.append(np.concatenate([rng.integers(0, 20, int(rng.integers(8, 40))), body, rng.integers(0, 20, int(rng.integers(0, 40)))]).astype(np.uint8))
        self.tail_segment = rng.integers(0, 20, 24).astype(np.uint8)
        for keep in (6, 7, 8, 9, 10):
            for at in (2, 9):
                self.subjects.append(np.concatenate([rng.integers(0, 20, 30), self.tail_segment[:at + keep]]).astype(np.uint8))

    def frames(self, L, nreads=ENUM_READS):
        """(nreads, 6, FP) dense codes for reads of L bases.  Read 0: the ancestor's own segment in every frame (more kept positions than
        the position list's 256 entries at 510 bases); 1: family members' segments; 2: wholly invalid; 3: frame 0 invalid, the rest a
        subject's segment; 4 .. 7: a segment with MC_INV at one of the offsets 6 .. 9 of every eleventh window, and at the offsets 0 .. 5;
        8, 9: the tail segment at the frame's start, in its middle and at its end; 10: the motifs with each of their two groups behind them;
        11: singles' segments; the rest: random residues with a family segment in one frame - and every read once more from 16 on (a chunk
        of sixteen reads carries deferred positions over from one read to the next)."""
        rng = np.random.default_rng(L)
        want, nreads = nreads, max(nreads, ENUM_READS)
        FPL = frame_pitch(L)
        qlen = [(L - f % 3) // 3 for f in range(6)]
        fr = rng.integers(0, 20, (nreads, 6, FPL)).astype(np.uint8)

        def put(r, f, at, seg):
            if at < 0:
                seg, at = seg[-at:], 0
            if at + 10 > qlen[f]:
                at = 0
            if r < nreads:
                n = max(0, min(len(seg), qlen[f] - at))
                fr[r, f, at:at + n] = seg[:n]
        fam = self.subjects[40:80]
        for f in range(6):
            put(0, f, 0, self.ancestor[10 * f + 20:])
            put(1, f, 0, fam[7 * f][5 * f:])
            put(3, f, 0, self.subjects[f][3:])
            for r in range(4, 8):
                put(r, f, 0, fam[r + f][f:])
                for p in range(f, qlen[f], 11):
                    if p + r + 2 < qlen[f]: fr[r, f, p + r + 2] = MC_INV
                if f == 5: fr[r, f, r - 4] = MC_INV
            put(8, f, (0, 3, 40, 100, 1, 2)[f] if L == L_NT else 0, self.tail_segment)
            put(9, f, qlen[f] - (9, 10, 11, 12, 13, 24)[f], self.tail_segment)
            for k, (m, first, second) in enumerate(self.motifs):
                put(10, f, 2 + 12 * k, np.concatenate([m, [first if f % 2 else second], rng.integers(0, 20, 3)]))
            put(11, f, f, self.subjects[6 + f])
        for r in range(12, nreads):
            if r >= 16 and r - 16 < 12:
                fr[r] = fr[r - 16]
            else:
                put(r, r % 6, r, fam[r % 40][r:])
        fr[2] = MC_INV
        fr[3, 0] = MC_INV
        for f in range(6):
            fr[:, f, qlen[f]:] = MC_INV
        return fr[:want].copy()


_enum_world = []


def enum_world():
    if not _enum_world:
        import tempfile
        w = EnumWorld()
        w.tmp = tempfile.TemporaryDirectory(prefix="seed_enum")
        w.db = Db(w.subjects, w.tmp.name)
        w._want = {}
        _enum_world.append(w)
    return _enum_world[0]


def enum_want(w, L, nreads):
    """The oracle's ranges of every row of frames(L, nreads), and expanded per posting: (read, chrono, posting, seedlen, nkey)."""
    if (L, nreads) not in w._want:
        fr = w.frames(L, nreads)
        ranges, hits = [], []
        for r in range(nreads):
            for f in range(6):
                rg = w.db.ranges(fr[r, f], (L - f % 3) // 3, f)
                ranges.append(rg)
                for pos, bucket, seedlen, nkey, nst, ned, phase in rg:
                    b0 = int(w.db.bstart[bucket])
                    hits += [(r, (f << 25) | (pos << 17) | (phase << 11) | i, int(w.db.post[b0 + i]), seedlen, nkey) for i in range(nst, ned)]
        w._want[(L, nreads)] = (fr, ranges, sorted(hits))
    return w._want[(L, nreads)]


# ---- what the harnesses read -----------------------------------------------------------------------------------------------------------------
def sections(frames, subjects, L):
    """What tests/emul/seeds.cpp and every verb of device_seeds.hip but post8 read first: L, FP, reads; the frames; the subjects' letters; their offsets."""
    off, text = letters_of(subjects)
    return [np.array([L, frames.shape[2], frames.shape[0]], np.int32), frames, text, off]


def hit_array(hits):
    return np.array([[h[n] for n in ("read", "frame", "qpos", "sidx", "dpos", "seedlen", "nkey")] for h in hits], np.int32).reshape(len(hits), 7)


HOST_SRC = os.path.join(oc.EMUL, "seeds.cpp")


def build_host(tmp, flags=("-O2",)):
    import subprocess
    exe = str(tmp / "seeds")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-o", exe, HOST_SRC])
    return exe


def host_seeds(exe, tmp, frames, subjects, L, hits, rows):
    """seeds.cpp on a world: (per hit 24 int32, per hit loge, per row its ranges as lists of 7-tuples, postings, bucket starts, stderr)."""
    import subprocess
    oc.write_sections(tmp / "seeds.in", sections(frames, subjects, L) + [hit_array(hits), np.asarray(rows, np.int32)])
    p = subprocess.run([exe, str(tmp / "seeds.in"), str(tmp / "seeds.out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    s = oc.read_sections(tmp / "seeds.out")
    res = np.frombuffer(s[0], "<i4").reshape(-1, 24)
    counts, flat = np.frombuffer(s[2], "<i4"), np.frombuffer(s[3], "<i4").reshape(-1, 7)
    at = np.concatenate([[0], np.cumsum(counts)])
    ranges = [[tuple(int(v) for v in r) for r in flat[at[k]:at[k + 1]]] for k in range(len(counts))]
    return res, np.frombuffer(s[1], "<f8"), ranges, np.frombuffer(s[4], "<u4"), np.frombuffer(s[5], "<u4"), p.stderr


GAP_FIELDS = ("sidx", "qp", "dp", "L", "qfwd", "qbwd", "score", "nmatch")
HSP_FIELDS = ("score", "frame", "alnlen", "mism", "gaps", "nmatch", "qaas", "qaae", "ds", "de", "qnts", "qnte")


def want_result(h, o):
    """What the product's evaluation of a hit must say, from the oracle's answer: (result 0 / 1 / 2, the eight McGapTask fields, kept, the twelve HSP fields)."""
    if o["why"] != EXTENDED:
        return (0,) + (0,) * 8 + (0,) + (0,) * 12
    gap = (h["sidx"], o["qp"], o["dp"], o["L"], o["qfwd"], o["qbwd"], o["score"], o["nmatch"])
    if o["gapped"]:
        return (2,) + gap + (0,) + (0,) * 12
    if not o["kept"]:
        return (1,) + gap + (0,) + (0,) * 12
    return (1,) + gap + (1,) + (o["score"], h["frame"], o["alnlen"], o["mism"], 0, o["nmatch"], o["qaas"], o["qaae"], o["ds"], o["de"], o["qnts"], o["qnte"])
