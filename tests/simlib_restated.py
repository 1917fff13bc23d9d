"""The library simulator's formula (csrc/mc_simlib.h, csrc/k_simulate.h) restated in numpy, vectorised over reads: the bytes of
any library kind, and the log of every consumed base's error event.  Shared by the CPU and GPU tests of the simulator."""
import numpy as np

MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
EKEY = 0xA0761D6478BD642F
NTHR = 235
SUB, INS = 52429, 58982
MODELS = {None: 0, "uniform": 1, "illumina": 2}
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def mix64(z):
    z = (int(z) + GAMMA) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix64_np(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def p_error(model, rate, j):
    """p(j) of the model, uncapped (the reference's formula)."""
    if model == "illumina":
        t = float(j + 1)
        return (3e-3 + 3.3e-8 * (t * t * t * t)) / 100.0
    return float(rate) if model == "uniform" else 0.0


def thresholds(model, rate):
    return [1 << 32 if p >= 1.0 else int(p * 4294967296.0) for p in (p_error(model, rate, j) for j in range(NTHR))]


def revcomp(row):
    return COMP[np.asarray(row, dtype=np.uint8)[::-1]]


def simulate(bases, off, L, first, n, seed, lib, error_model=None, error_rate=None, paired_end=False, insert=None, log=None):
    """Rows [first, first + n) of library (seed, lib) of the given kind: uint8 (n, L).  log, a list, receives per consumed-base
    index j the tuple (j, event, drawn base) over the reads still walking (event 0 none, 1 substitution, 2 insertion, 3 deletion,
    4 deletion refused)."""
    bases = np.asarray(bases, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    span = insert if paired_end else L
    vstart = np.zeros(len(off), dtype=np.int64)
    vstart[1:] = np.cumsum(np.maximum(0, np.diff(off) - span + 1))
    total = int(vstart[-1])
    key = mix64(seed ^ mix64(lib))
    ekey = mix64(key ^ EKEY)
    i = np.arange(first, first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        frag = i >> np.uint64(1) if paired_end else i
        u = (mix64_np(np.uint64(key) + frag) % np.uint64(total)).astype(np.int64)
        r = mix64_np(np.uint64(ekey) + i)
    c = np.searchsorted(vstart, u, side="right") - 1
    cs, ce = off[c], off[c + 1]
    s = cs + (u - vstart[c])
    rev = (i & np.uint64(1)).astype(bool) if paired_end else np.zeros(n, dtype=bool)
    step = np.where(rev, -1, 1)
    p = np.where(rev, s + span - 1, s)
    thr = np.array(thresholds(error_model, error_rate), dtype=np.uint64)
    errors = error_model is not None
    out = np.zeros((n, L), dtype=np.uint8)
    o = np.zeros(n, dtype=np.int64)
    j = 0
    while True:
        a = np.nonzero(o < L)[0]
        if len(a) == 0:
            break
        pa = p[a]
        assert np.all(pa >= cs[a]) and np.all(pa < ce[a]), "a walk left its contig"
        b = bases[pa]
        b = np.where(rev[a], COMP[b], b)
        e = np.zeros(len(a), dtype=np.int64)
        x = np.zeros(len(a), dtype=np.uint8)
        if errors:
            with np.errstate(over="ignore"):
                d = mix64_np(r[a] + np.uint64((j * GAMMA) & MASK))
            err = (d >> np.uint64(32)) < thr[min(j, NTHR - 1)]
            kind = ((d >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
            x = ACGT[(d & np.uint64(3)).astype(np.int64)]
            e = np.where(err, np.where(kind < SUB, 1, np.where(kind < INS, 2, 3)), 0)
            left = np.where(step[a] > 0, ce[a] - 1 - pa, pa - cs[a])
            e = np.where((e == 3) & (left < L - o[a]), 4, e)
        if log is not None:
            log.append((j, e, x))
        keep = (e == 0) | (e == 4)
        out[a[keep], o[a[keep]]] = b[keep]
        sub = e == 1
        out[a[sub], o[a[sub]]] = x[sub]
        ins = e == 2
        out[a[ins], o[a[ins]]] = x[ins]
        o[a[keep | sub | ins]] += 1
        ins2 = ins & (o[a] < L)
        out[a[ins2], o[a[ins2]]] = b[ins2]
        o[a[ins2]] += 1
        p[a] += step[a]
        j += 1
    return out


def toy_genome(seed=5, lens=(30, 400, 5, 1200, 151, 149, 700)):
    """Contigs of ACGT, acgt, N and other bytes (IUPAC codes, '-'), some shorter than a read."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtacgtNnRY-", dtype=np.uint8)
    return alphabet[rng.integers(0, len(alphabet), int(off[-1]))], off
