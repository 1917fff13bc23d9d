"""Inputs of the ordering / finishing unit tests (test_order_host.py on the CPU, test_gpu_order_units.py on the device): seeded numpy
builds them, the harnesses under tests/emul (wave_sort_form.cpp, device_order.hip) read them as files of sections (order_io.h).
Every input is a legal state of the pipeline - sizes within the kernels' capacities, indices in range; the harness checks that again
before anything is launched."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "microbecensus_amd", "csrc")
EMUL = os.path.join(REPO, "tests", "emul")


def define(name, header):
    """The default of a capacity the library's headers define (the harness is built with the same defaults)."""
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(os.path.join(CSRC, header)).read(), re.M)
    return int(m.group(1))


FH_N = tuple(define("MC_FH_N%d" % k, "k_finish.h") for k in (1, 2, 3))           # 512, 1280, 6144
FH_MIN = define("MC_FH_MIN", "k_finish.h")                                        # 96
BIN_LIGHT = define("MC_BIN_LIGHT", "k_order.h")                                   # 32
ORDER_CAPS = tuple(define(n, "k_order.h") for n in ("MC_ORDER_SMALL", "MC_ORDER_MID", "MC_ORDER_LDS"))   # 512, 2048, 8192
MAX_M8 = define("MC_MAX_M8", "mc_core.h")                                         # 500
C_HSPS, C_HEAVY, C_ORDER, C_ORDER2, C_ORDER3, C_OTAKE, C_OTAKE2, C_OTAKE3 = 2, 9, 21, 22, 23, 24, 25, 26   # (mc_hip_common.h's enum)

HSP = np.dtype([("read", "<u4"), ("chrono", "<u4"), ("sidx", "<i4"), ("score", "<i2"), ("frame", "<i2"), ("alnlen", "<i2"), ("mism", "<i2"),
                ("gaps", "<i2"), ("nmatch", "<i2"), ("qaas", "<i2"), ("qaae", "<i2"), ("ds", "<i2"), ("de", "<i2"), ("qnts", "<i2"), ("qnte", "<i2"),
                ("loge", "<f8")], align=True)
assert HSP.itemsize == 48
PLACE_FIELDS = ("frame", "qaas", "qaae", "ds", "de")
COMPARED_FIELDS = tuple(f for f in HSP.names if f not in ("read", "chrono"))


def write_sections(path, arrays):
    with open(path, "wb") as f:
        f.write(np.uint32(len(arrays)).tobytes())
        for a in arrays:
            b = np.ascontiguousarray(a).tobytes()
            f.write(np.uint64(len(b)).tobytes())
            f.write(b)


def read_sections(path):
    raw = open(path, "rb").read()
    n, at, out = int(np.frombuffer(raw, "<u4", 1)[0]), 4, []
    for _ in range(n):
        nb = int(np.frombuffer(raw, "<u8", 1, at)[0])
        out.append(raw[at + 8:at + 8 + nb])
        at += 8 + nb
    assert at == len(raw)
    return out


# ---- the device harnesses (tests/emul/device_*.hip): one build, one child process per case ---------------------------------------------
_ABNORMAL = []          # the cases whose child ended abnormally, in any module: nothing more is started on the GPU behind them


def harness(name, tmp_path_factory):
    """tests/emul/<name>.hip built with the library's flags (a module-scoped fixture calls this: once per module)."""
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(EMUL, name + ".hip")])
    return exe


def run_child(exe, case, arrays, tmp, limit, verb=None):
    """One child process `exe <verb or case> IN OUT` under a time limit of its own; returns the sections it wrote.  A child that ends by a
    signal, at its time limit or with a HIP error fails its test with its output, and every later call - of any module - fails at once
    without starting anything.  Exit status 2, the harness refusing its input before anything was launched, is no such end."""
    if _ABNORMAL:
        pytest.fail("not started: the child of case %s ended abnormally earlier in this run" % _ABNORMAL[0], pytrace=False)
    write_sections(tmp / (case + ".in"), arrays)
    cmd = ["timeout", "-k", "10", str(limit), exe, verb or case, str(tmp / (case + ".in")), str(tmp / (case + ".out"))]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit + 30)
    except subprocess.TimeoutExpired as e:
        _ABNORMAL.append(case)
        pytest.fail("%s: no end after %d s\n%s" % (case, limit + 30, e.stdout), pytrace=False)
    if p.returncode != 0:
        if p.returncode != 2:
            _ABNORMAL.append(case)
        pytest.fail("%s: exit status %d\n%s" % (case, p.returncode, p.stdout), pytrace=False)
    return read_sections(tmp / (case + ".out"))


def pack(arrays, dtype):
    """Arrays one after the other, and where each starts."""
    off = np.zeros(len(arrays) + 1, np.uint32)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return off, (np.concatenate([np.asarray(a, dtype) for a in arrays]) if arrays else np.zeros(0, dtype)).astype(dtype)


# ---- sort keys ----------------------------------------------------------------------------------------------------------------------
WAVE_LENGTHS = (0, 1, 2, 15, 16, 17, 18, 32, 33, 63, 64, 65, 127, 128, 129, 500, 511, 512)
WAVE_LENGTHS_MORE = ((), (513, 1279, 1280), (513, 1279, 1280, 1281, 4096, 6143, 6144))   # beyond the first MAXN, for the second and third
KEY_PATTERNS = ("equal", "two", "five", "fifty", "distinct", "ascending", "descending", "organ_pipe", "adversary")


def adversary_lengths():
    return sorted(set(WAVE_LENGTHS) | set(WAVE_LENGTHS_MORE[2]) | set(range(FH_MIN + 1)))


def pattern_keys(kind, n, rng, adversary):
    i = np.arange(n, dtype=np.float64)
    if kind == "equal":
        return np.full(n, -3.5)
    if kind in ("two", "five", "fifty"):
        return rng.integers(0, {"two": 2, "five": 5, "fifty": 50}[kind], n).astype(np.float64) - 20.0
    if kind == "distinct":
        return rng.permutation(n).astype(np.float64) * 0.37 - 100.0
    if kind == "ascending":
        return i
    if kind == "descending":
        return n - i
    if kind == "organ_pipe":
        return np.minimum(i, n - 1 - i)
    assert kind == "adversary" and len(adversary[n]) == n
    return adversary[n]


def wave_sort_sets(adversary):
    """Per MAXN: (MAXN, [(length, pattern, keys)]): every length with every pattern, the random patterns twice."""
    rng = np.random.default_rng(20240611)
    sets = []
    for maxn, more in zip(FH_N, WAVE_LENGTHS_MORE):
        arrays = []
        for n in WAVE_LENGTHS + more:
            assert n <= maxn
            for kind in KEY_PATTERNS:
                for _ in range(2 if kind in ("two", "five", "fifty", "distinct") else 1):
                    arrays.append((n, kind, pattern_keys(kind, n, rng, adversary)))
        sets.append((maxn, arrays))
    return sets


def wave_input(sets):
    arrays = [np.uint32(len(sets))]
    for maxn, arrs in sets:
        off, keys = pack([k for _, _, k in arrs], np.float64)
        arrays += [np.uint32(maxn), off, keys]
    return arrays


def fallback_conditions(sets, stats_of):
    """The conditions the wave_sort case sets on its inputs: per MAXN the fallback is reached for every length >= 64, and once at least
    with more than 64 elements in the heap-sorted range.  stats_of[q]: per array (fallbacks, largest range, stack overflows)."""
    lines = []
    for (maxn, arrs), st in zip(sets, stats_of):
        st = np.asarray(st).reshape(len(arrs), 3)
        assert not st[:, 2].any(), "the formulation's stack of 64 entries overflowed"
        for n in sorted({n for n, _, _ in arrs if n >= 64}):
            assert any(st[k, 0] > 0 for k, (m, _, _) in enumerate(arrs) if m == n), "MAXN %d: no array of length %d reaches the depth-0 fallback" % (maxn, n)
        assert st[:, 1].max() > 64, "MAXN %d: no fallback range of more than 64 elements" % maxn
        lines.append("MAXN %d: %d arrays, %d reach the fallback (%d fallbacks), largest range %d" % (maxn, len(arrs), int((st[:, 0] > 0).sum()), int(st[:, 0].sum()), int(st[:, 1].max())))
    return lines


def thread_sorts_sets(adversary):
    """Per (items per thread): arrays of every length 0 .. ITEMS with every pattern, shuffled so that the lanes of a wave diverge."""
    rng = np.random.default_rng(77)
    sets = []
    for items, rounds in ((FH_MIN, 1), (16, 3)):
        arrays = [(n, kind, pattern_keys(kind, n, rng, adversary)) for _ in range(rounds) for n in range(items + 1) for kind in KEY_PATTERNS]
        sets.append((items, [arrays[k] for k in rng.permutation(len(arrays))]))
    return sets


# ---- merge sort items ---------------------------------------------------------------------------------------------------------------
MERGE_PATTERNS = ("random", "ascending", "descending", "partner_below", "partner_above", "interleaved", "low21", "padded")


def merge_items(kind, m, rng):
    k = np.arange(m, dtype=np.uint64)
    nb = m // 64
    inblock = np.concatenate([rng.permutation(64) for _ in range(nb)]).astype(np.uint64)
    block = k // np.uint64(64)
    if kind == "random":
        v = (rng.integers(0, 1 << 43, m).astype(np.uint64) << np.uint64(21)) | k
    elif kind == "ascending":
        v = k * np.uint64(3) + np.uint64(5)
    elif kind == "descending":
        v = (np.uint64(m) - k) * np.uint64(3)
    elif kind == "partner_below":          # every run lies entirely below the run to its left, at every width
        v = (np.uint64(nb - 1) - block) * np.uint64(64) + inblock
    elif kind == "partner_above":
        v = block * np.uint64(64) + inblock
    elif kind == "interleaved":            # the chunks of 64 dovetail: consecutive values lie in consecutive chunks
        v = inblock * np.uint64(nb) + block
    elif kind == "low21":                  # one (subject, hit order), told apart by the position alone
        v = (np.uint64(0x5A5A5A5A5A5) << np.uint64(21)) | rng.choice(1 << 21, m, replace=False).astype(np.uint64)
    else:                                  # a segment of n < m HSPs and MC_ITEM_OF's padding behind it
        n = m // 2 + 1 + int(rng.integers(0, m // 2 - 1))
        v = (rng.integers(0, 1 << 43, m).astype(np.uint64) << np.uint64(21)) | k
        v[n:] = (np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(21)) | k[n:]
        v[:n] = v[:n][rng.permutation(n)]
    assert len(np.unique(v)) == m
    return v


def mergesort_sets():
    rng = np.random.default_rng(4242)
    sets = []
    for cap in ORDER_CAPS:
        arrays, m = [], 64
        while m <= cap:
            arrays += [(m, kind, merge_items(kind, m, rng)) for kind in MERGE_PATTERNS]
            m *= 2
        sets.append((cap, arrays))
    return sets


# ---- the ordering step: synthetic segments ----------------------------------------------------------------------------------------------
ORDER_LENGTHS = tuple(sorted({1, 2, BIN_LIGHT - 1, BIN_LIGHT, BIN_LIGHT + 1, 63, 64, 65, 20000} | {c + d for c in ORDER_CAPS for d in (-1, 0, 1)}))
ORDER_STRUCTURES = ("one_per_subject", "one_subject", "mixed", "straddle_run", "straddle_subject", "equal_keys", "all_same", "last_starts_subject", "last_starts_run")


def _subject_sizes(kind, n, rng):
    if kind == "one_per_subject":
        return [1] * n
    if kind in ("one_subject", "all_same"):
        return [n]
    if kind in ("straddle_run", "straddle_subject"):          # subjects over the sorted positions [64 k - 2, 64 k + 62)
        cuts = [0] + list(range(62, n, 64)) + [n]
        return [b - a for a, b in zip(cuts, cuts[1:]) if b > a]
    sizes, left = [], n - (1 if kind == "last_starts_subject" else 2 if kind == "last_starts_run" and n >= 2 else 0)
    while left > 0:
        sizes.append(min(left, int(rng.integers(1, 6))))
        left -= sizes[-1]
    if kind == "last_starts_subject":
        sizes.append(1)
    if kind == "last_starts_run" and n >= 2:
        sizes.append(2)
    return sizes


def _run_sizes(kind, size, first, rng):
    if kind in ("one_per_subject", "straddle_subject"):
        return [1] * size
    if kind == "all_same":
        return [size]
    if kind == "straddle_run":                                 # the subject's first four HSPs, two on either side of a multiple of 64, are one run
        head = min(size, 4) if not first else 1
        return [head] + [1] * (size - head)
    if kind == "last_starts_run" and size == 2:
        return [1, 1]
    runs, left = [], size
    while left > 0:
        runs.append(min(left, int(rng.integers(1, 5))))
        left -= runs[-1]
    return runs


def segment(kind, n, rng):
    """A read's HSPs in the order (subject, hit order): subject, hit order, place number and score of each."""
    sizes = _subject_sizes(kind, n, rng)
    subjects = np.sort(rng.choice(32767, len(sizes), replace=False))
    sidx, chrono, place, score = [], [], [], []
    for g, (s, size) in enumerate(zip(subjects, sizes)):
        c = int(rng.integers(0, 1 << 20))
        places = []
        for run in _run_sizes(kind, size, g == 0, rng):
            p = int(rng.integers(0, 900000))
            if len(places) >= 2 and rng.random() < 0.2:
                p = places[-2]                                 # a place met again behind another one: a run of its own
            while places and p == places[-1]:
                p = int(rng.integers(0, 900000))
            places.append(p)
            base = int(rng.integers(30, 3000))
            equal = rng.random() < 0.4
            for _ in range(run):
                sidx.append(int(s)); place.append(p)
                chrono.append(c)
                if kind not in ("equal_keys", "all_same"):
                    c += int(rng.integers(1, 4))
                score.append(base if equal else base + int(rng.integers(0, 4)))
    return np.array(sidx), np.array(chrono), np.array(place), np.array(score)


def order_case():
    """The pool, the binned slots, heads and low of the order case, and per read (length, structure)."""
    rng = np.random.default_rng(31337)
    reads = []
    for n in ORDER_LENGTHS:
        for si, kind in enumerate(ORDER_STRUCTURES):
            if kind.startswith("last_starts") and not 2 <= n <= BIN_LIGHT + 1:
                continue
            if n == 20000 and kind not in ("one_subject", "mixed", "straddle_run"):
                continue
            for low in ((0, 1) if n <= ORDER_CAPS[1] else ((si + n) & 1,)):
                reads.append((n, kind, low))
    for _ in range(len(reads) // 8 + 5):
        reads.append((0, "empty", 0))                               # (low is set by the kernel that makes an HSP: never for a read without one)
    reads = [reads[k] for k in rng.permutation(len(reads))]
    assert len(reads) % 64 not in (0, 63)
    total = sum(n for n, _, _ in reads)
    rec = np.zeros(total, HSP)
    heads = np.zeros(len(reads) + 1, np.uint32)
    at = 0
    for r, (n, kind, low) in enumerate(reads):
        heads[r] = at
        if n:
            sidx, chrono, place, score = segment(kind, n, rng)
            seg = rec[at:at + n]
            binned = rng.permutation(n)                            # the order the binning left: any
            seg["read"] = r
            seg["sidx"], seg["chrono"], seg["score"] = sidx[binned], chrono[binned], score[binned]
            p = place[binned]
            seg["frame"], seg["qaas"], seg["ds"] = p % 6, (p // 6) % 150, (p // 900) % 1100
            seg["qaae"], seg["de"] = seg["qaas"] + 12, seg["ds"] + 40
        at += n
    heads[-1] = at
    rec["loge"] = 12.5 - 0.03125 * rec["score"]                  # strictly decreasing in the score, as the run tables make it
    rec["alnlen"], rec["mism"], rec["gaps"] = 30 + rec["score"] % 97, rec["score"] % 13, rec["score"] % 3
    rec["nmatch"] = rec["alnlen"] - rec["mism"]
    rec["qnts"], rec["qnte"] = np.arange(total) % 30011, np.arange(total) % 29989     # (tell the members of a run apart where their scores tie)
    where = rng.permutation(total + 100)[:total].astype(np.uint32)   # the pool: the records anywhere, unused slots among them
    pool = np.zeros(total + 100, HSP)
    pool["sidx"], pool["loge"] = -1, 99.0
    pool[where] = rec
    low = np.array([lw for _, _, lw in reads], np.uint8)
    return pool, where, heads, low, reads


def place_words(rec):
    return (rec["frame"].astype(np.int64) << 38) | (rec["qaas"].astype(np.int64) << 30) | (rec["qaae"].astype(np.int64) << 22) | (rec["ds"].astype(np.int64) << 11) | rec["de"].astype(np.int64)


def restated_stacks(seg):
    """CalRes' rule, plainly: the read's HSPs by (subject, hit order, position); of consecutive HSPs of one subject at one place keep
    the first with the lowest log E; a subject's kept HSPs newest first, the first carrying the stack's size.
    seg: the read's records in binned order.  Returns (positions in seg, stack sizes)."""
    sidx, chrono, loge, plc = seg["sidx"].tolist(), seg["chrono"].tolist(), seg["loge"].tolist(), place_words(seg).tolist()
    o = sorted(range(len(seg)), key=lambda k: (sidx[k], chrono[k], k))
    out, sizes, i = [], [], 0
    while i < len(o):
        stack, j = [], i
        while j < len(o) and sidx[o[j]] == sidx[o[i]]:
            best, e = j, j + 1
            while e < len(o) and sidx[o[e]] == sidx[o[j]] and plc[o[e]] == plc[o[j]]:
                if loge[o[e]] < loge[o[best]]:
                    best = e
                e += 1
            stack.append(o[best]); j = e
        out += stack[::-1]; sizes += [len(stack)] + [0] * (len(stack) - 1); i = j
    return out, sizes


def expected_marks(pool, slots, heads, low):
    """A read is marked when low says so or two HSPs of one subject differ in place."""
    marked = low.astype(bool) & (np.diff(heads.astype(np.int64)) > 0)
    for r in range(len(low)):
        seg = pool[slots[heads[r]:heads[r + 1]]]
        if len(seg) > 1 and not marked[r]:
            both = np.unique(np.stack([seg["sidx"].astype(np.int64), place_words(seg)], 1), axis=0)
            marked[r] = len(both) > len(np.unique(both[:, 0]))
    return marked


# ---- MergeRes' heap sort a lane per read --------------------------------------------------------------------------------------------
HEAP_ROWS = (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, MAX_M8 - 1, MAX_M8)
HEAP_NHEAVY = (1, 63, 64, 65, 200, 256 * 64 + 65)               # (the last: more than the grid of 256 waves takes in one round)
RANK_PATTERNS = ("equal", "two", "ascending", "descending", "random_ties")


def heap_words(kind, n, rng):
    i = np.arange(n, dtype=np.uint32)
    rank = {"equal": np.full(n, 7), "two": np.sort(rng.integers(0, 2, n)), "ascending": i, "descending": n - 1 - i if n else i,
            "random_ties": rng.integers(0, max(1, n // 4) + 1, n)}[kind]
    return (np.asarray(rank, np.uint32) << np.uint32(16)) | i


def heap_lanes_sets():
    rng = np.random.default_rng(500)
    sets = []
    for nheavy in HEAP_NHEAVY:
        nheads = nheavy + 3
        rows = np.zeros(nheads, np.uint32)
        listed = rng.permutation(nheads)[:nheavy]
        for k, s in enumerate(listed):
            rows[s] = HEAP_ROWS[int(rng.integers(0, len(HEAP_ROWS)))] if k < 200 else int(rng.integers(0, 5))
        for k in range(min(nheavy, len(HEAP_ROWS))):
            rows[listed[k]] = HEAP_ROWS[(k + nheavy) % len(HEAP_ROWS)]
        nseg = np.maximum(rows, 1) + rng.integers(0, 3, nheads).astype(np.uint32)
        heads = np.zeros(nheads + 1, np.uint32)
        heads[1:] = np.cumsum(nseg)
        flagged = rng.random(nheavy) >= (0.1 if nheavy > 1 else 0.0)
        heavy_first = listed.astype(np.uint32) | np.where(flagged, np.uint32(0x80000000), np.uint32(0))
        words = [heap_words(RANK_PATTERNS[(int(s) + k) % len(RANK_PATTERNS)], int(rows[s]), rng) for k, s in enumerate(range(nheads))]
        sets.append(dict(heads=heads, rows=rows, heavy_first=heavy_first, order=rng.permutation(nheavy).astype(np.uint32), words=words))
    return sets


# ---- counting sorts -----------------------------------------------------------------------------------------------------------------
COUNT_SIZES = (0, 1, 1023, 1024, 1025, 5000)
COUNT_KEYS = ("equal", "one_per_bin", "clamped", "random")


def counting_sorts_sets():
    rng = np.random.default_rng(1024)
    sets = []
    for n in COUNT_SIZES:
        for ki, kind in enumerate(COUNT_KEYS):
            shift = (0, 2)[(ki + n) & 1]
            nreads = n + 9
            k = {"equal": np.full(nreads, 300), "one_per_bin": np.arange(nreads) % 512, "clamped": 400 + np.arange(nreads) % 400,
                 "random": rng.integers(0, 700, nreads)}[kind]
            nv = ((k.astype(np.uint32) << np.uint32(shift)) | rng.integers(0, 1 << shift, nreads).astype(np.uint32))
            heavy = rng.permutation(nreads).astype(np.uint32) | (rng.integers(0, 2, nreads).astype(np.uint32) << np.uint32(31))
            sets.append(dict(kind=0, shift=shift, keys=kind, list=rng.permutation(nreads)[:n].astype(np.uint32), heavy=heavy, nv=nv))
        for kind in COUNT_KEYS:
            nreads = n + 9
            rows = {"equal": np.full(nreads, 17), "one_per_bin": np.arange(nreads) % (MAX_M8 + 1), "clamped": MAX_M8 - 50 + np.arange(nreads) % 100,
                    "random": rng.integers(0, MAX_M8 + 1, nreads)}[kind].astype(np.uint32)
            heavy_first = rng.permutation(nreads)[:n].astype(np.uint32) | np.where(rng.random(n) < 0.9, np.uint32(0x80000000), np.uint32(0))
            sets.append(dict(kind=1, shift=0, keys=kind, heavy_first=heavy_first, rows=rows))
    return sets


# ---- binning and the scan -----------------------------------------------------------------------------------------------------------
def bins_sets():
    rng = np.random.default_rng(9)
    sets = []
    for nreads, nruns, use_cand in ((300, 160, 0), (300, 160, 1), (1, 1, 0), (70, 40, 1)):
        keys = []
        for k in range(nruns):
            read = int(rng.integers(0, nreads)) if nreads > 3 else 0
            if nreads > 3 and read % 7 == 3:
                read -= 1                                          # (reads 3, 10, 17, ... never have an HSP)
            length = (1, 2, 3, 60, 64, 65, 130, 300, 700)[int(rng.integers(0, 9))] if nruns > 1 else 1
            keys += [(read << 43) | (int(rng.integers(0, 32767)) << 28) | int(rng.integers(0, 1 << 28)) for _ in range(length)]
            if k % 5 == 4:
                keys += [0xFFFFFFFFFFFFFFFF] * (-len(keys) % 64)   # padding up to the end of a wave
        if nreads == 70:
            keys = keys[:len(keys) // 256 * 256]                   # (the pool ends with a block)
        hkeys = np.array(keys, np.uint64)
        sets.append(dict(nreads=nreads, use_cand=use_cand, hkeys=hkeys, hplace=rng.integers(0, 1 << 62, len(hkeys)).astype(np.uint64),
                         cand=(rng.random(nreads) < 0.7).astype(np.uint8)))
    return sets


SCAN_SIZES = (1, 2, 1023, 1024, 1025, 4095 * 1024 + 1, 4096 * 1024)
SCAN_REFUSED = 4096 * 1024 + 1


def scan_sets():
    rng = np.random.default_rng(2)
    return [dict(inplace=k & 1, values=rng.integers(0, 1000, n).astype(np.uint32)) for k, n in enumerate(SCAN_SIZES)]
