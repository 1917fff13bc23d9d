"""The statement of csrc/mc_tieboot.h restated in plain Python and numpy - the yardstick of the tie bootstrap's tests.

From rows alone: a read's tied set is ties_restated.tied_sets' (the four cut-offs, the highest bits, the distinct subjects below nseq at
that score, the first tied subject first; a read that abundance_restated does not assign adds nothing).  Every tied subject of a read of k
tied subjects is one ENTRY (q, s, share): share = 2^32 // k, and the first tied subject's has the remainder 2^32 - k (2^32 // k) added.  The
replicate share cs[s][b] is the sum over the entries of gene s of boot_restated.weights(seed, b, q) x share: Python-exact in uint64 (19 x
2^32 x 2^27 < 2^64).  Replicate b is used when scale[b] x 2^-32 is finite and > 0; the six doubles of a gene are geneboot_restated's on the
share matrix and those scales: float64(cs) x (scale x 2^-32), in the header's addition order, compared with the library's bit for bit."""
import numpy as np

import boot_restated as br
import geneboot_restated as GR
import order_cases as oc
import ties_restated as T

ONE = 1 << 32
MAXCAP = oc.define("MC_TB_MAXCAP", "mc_tieboot.h")
assert MAXCAP == 1 << 27 and 19 * ONE * MAXCAP < 1 << 64
ENTRY = np.dtype([("q", "<u4"), ("gene", "<u4"), ("share_m1", "<u4")])
assert ENTRY.itemsize == 12


def entries(rows, nseq, ids=None, **cut):
    """(q, s, share) int64 / int64 / uint64 arrays, one per (read, tied subject), in the order the reads first appear and within a read
    the first tied subject first; k: every such read's tied-set size.  rows: coverage_restated's 8-tuples.  ids: None - a row's query is the
    read's id - or a function of the query (a class run's base + perm[query])."""
    q, s, sh, ks = [], [], [], []
    for query, members in T.tied_sets(rows, nseq, **cut):
        k = len(members)
        assert 1 <= k <= 500
        each = ONE // k
        ks.append(k)
        for j, (sub, _, _) in enumerate(members):
            q.append(int(query) if ids is None else int(ids(query)))
            s.append(int(sub))
            sh.append(each + (ONE - k * each if j == 0 else 0))
    return np.array(q, np.int64), np.array(s, np.int64), np.array(sh, np.uint64), ks


def shares(q, s, sh, nseq, B, seed):
    """cs[s][b]: uint64[nseq, B] (the layout of mc_tie_bootstrap's shares)"""
    out = np.zeros((nseq, B), np.uint64)
    if len(q):
        sh = np.asarray(sh, np.uint64)
        for b0 in range(0, B, 256):                                 # (blocks of replicates: the weight matrix stays small)
            bs = np.arange(b0, min(B, b0 + 256), dtype=np.uint64)
            w = br.weights(seed, bs[:, None], np.asarray(q, np.int64).astype(np.uint64)[None, :]).astype(np.uint64) * sh[None, :]      # [b, entry]
            for g in np.unique(s):
                out[g, b0:b0 + len(bs)] = w[:, s == g].sum(axis=1, dtype=np.uint64)
    return out


def scale32(scale):
    """s32[b] = scale[b] x 2^-32, one float64 multiplication"""
    with np.errstate(all="ignore"):
        return np.asarray(scale, np.float64) * np.float64(2.0 ** -32)


def stats(cs, scale):
    """float64[nseq, 6]: geneboot_restated's six doubles of the share matrix under scale x 2^-32.  (GR.gene_stats takes its counts
    through int64 to uint64: the bits of a uint64 share survive the view.)"""
    return GR.stats(np.asarray(cs, np.uint64).view(np.int64), scale32(scale))


def used(scale):
    return GR.used(scale32(scale))
