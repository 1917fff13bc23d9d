"""The statement of csrc/mc_geneboot.h restated in plain Python and numpy - the yardstick of the gene bootstrap's tests.

A read's assignment is abundance_restated's best row (the four cut-offs, the highest bits, the first on a tie) with a subject below nseq.
The replicate count c[b][s] is the sum of boot_restated.weights(seed, b, q) over the reads q assigned to gene s: mc_boot.h's weights,
whose thresholds boot_restated parses out of that header.  Replicate b is used when scale[b] is finite and > 0; a used replicate's value
is float64(c[b][s]) * scale[b].  Per gene: sum and m2 added in the header's order - 256 partials, partial t over b = t, t + 256, ...
ascending, then the halving tree - and the sorted used values at floor((m - 1) * 0.025), the next, floor((m - 1) * 0.975), the next (the
next clamped to m - 1).  numpy's float64 additions and multiplications are single IEEE operations, never fused: the results are compared
with the library's bit for bit."""
import numpy as np

import abundance_restated as R
import boot_restated as br
import order_cases as oc

THREADS = oc.define("MC_GB_THREADS", "mc_geneboot.h")
MAXB = oc.define("MC_GB_MAXB", "mc_geneboot.h")
LANES = oc.define("MC_GB_LANES", "mc_geneboot.h")
TILES = oc.define("MC_GB_TILES", "mc_geneboot.h")
assert THREADS == 256 and MAXB == 4096


def assignments(rows, nseq, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """(q, subject) arrays of the assigned reads of rows as abundance_restated.rows_from_array / rows_from_m8 give them, in the order the
    reads first appear"""
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge in rows:
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge))
    qs, ss = [], []
    for q, rs in by_read.items():
        best = None
        for s, nmatch, alnlen, bits, loge in rs:
            if not R.passes(nmatch, alnlen, bits, loge, min_ident, min_aln, min_bits, max_loge):
                continue
            if best is None or best[1] < bits:
                best = (s, bits)
        if best is not None and 0 <= best[0] < nseq:
            qs.append(int(q)); ss.append(int(best[0]))
    return np.array(qs, np.int64), np.array(ss, np.int64)


def counts(q, s, nseq, B, seed):
    """c[s][b]: int64[nseq, B] (the layout of mc_gene_bootstrap's counts)"""
    out = np.zeros((nseq, B), np.int64)
    if len(q):
        for b0 in range(0, B, 256):                               # (blocks of replicates: the weight matrix stays small)
            bs = np.arange(b0, min(B, b0 + 256), dtype=np.uint64)
            w = br.weights(seed, bs[:, None], np.asarray(q, np.int64).astype(np.uint64)[None, :])      # [b, read]
            for g in np.unique(s):
                out[g, b0:b0 + len(bs)] = w[:, s == g].sum(axis=1)
    return out


def used(scale):
    scale = np.asarray(scale, np.float64)
    return np.isfinite(scale) & (scale > 0)


def _tree(part):
    part = part.copy()
    h = THREADS // 2
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def _ordered_sum(terms, use):
    """terms: float64[B]; the header's order: partial t adds its used b = t, t + 256, ... ascending from 0.0 (adding 0.0 for a skipped one
    leaves a non-negative partial as it is), then the halving tree"""
    B = len(terms)
    rows = -(-B // THREADS)
    t = np.zeros(rows * THREADS, np.float64)
    t[:B] = np.where(use, terms, 0.0)
    part = np.zeros(THREADS, np.float64)
    for r in t.reshape(rows, THREADS):
        part = part + r
    return _tree(part)


def index(m, which):
    """mc_gb_index: which in 2 .. 5 (lo, lo + 1, hi, hi + 1)"""
    at = int(float(m - 1) * (0.025 if which in (2, 3) else 0.975))
    return min(at + (1 if which in (3, 5) else 0), m - 1)


def gene_stats(c, scale):
    """the six doubles of one gene: c int64[B], scale float64[B]"""
    scale = np.asarray(scale, np.float64)
    use = used(scale)
    m = int(use.sum())
    if m == 0:
        return np.full(6, np.nan)
    with np.errstate(all="ignore"):
        v = np.asarray(c, np.int64).astype(np.uint64).astype(np.float64) * scale
        total = _ordered_sum(v, use)
        d = v - total / np.float64(m)
        m2 = _ordered_sum(d * d, use)
    x = np.sort(v[use])
    return np.array([total, m2] + [x[index(m, k)] for k in (2, 3, 4, 5)], np.float64)


def stats(cmat, scale):
    """float64[nseq, 6] of counts int64[nseq, B]; a gene without reads is computed like any other (zeros, or NaN with m == 0)"""
    cache = {}
    out = np.zeros((len(cmat), 6), np.float64)
    for s, c in enumerate(cmat):
        key = c.tobytes()
        if key not in cache:
            cache[key] = gene_stats(c, scale)
        out[s] = cache[key]
    return out


def per_tile(n, B):
    """mc_gb_per_tile: the entries of the grouped list one wave of k_geneboot_sums walks"""
    nbt = (B + LANES - 1) // LANES
    want = max(TILES // nbt, 1)
    return max((n + want - 1) // want, 64)


def same_bits(a, b):
    """two float64 arrays hold the same bits, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
