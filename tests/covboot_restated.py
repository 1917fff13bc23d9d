"""The statement of csrc/mc_covboot.h restated in plain Python and numpy - the yardstick of the coverage bootstrap's tests.

From rows alone: every assigned read - abundance_restated's best row (the four cut-offs, the highest bits, the first on a tie) with a subject
below nseq - is one ENTRY (q, gene, s, e): the best row's sstart and send, or the empty span (1, 0) where coverage_restated keeps the span out
of the depth (not 0 <= sstart <= send <= len - 1).  Read q is present in replicate b when boot_restated.weights(seed, b, q) > 0.  cov[g][b]
is the number of residues of gene g that lie in the span of at least one present entry of g: built as a depth per replicate and residue, with
no window and no bit masks - nothing the kernels do.  The six doubles of a gene are geneboot_restated's on cov under a scale of ones (every
replicate used), compared with the library's bit for bit; det[g] counts the replicates with cov >= need[g]."""
import numpy as np

import abundance_restated as R
import boot_restated as br
import geneboot_restated as GR
import order_cases as oc

WINDOW = oc.define("MC_CB_WINDOW", "mc_covboot.h")
MAXCAP = oc.define("MC_CB_MAXCAP", "mc_covboot.h")
assert MAXCAP == 2 ** 31 - 1 and WINDOW % 64 == 0
ENTRY = np.dtype([("q", "<u4"), ("gene", "<u4"), ("s", "<u2"), ("e", "<u2")])
assert ENTRY.itemsize == 12
EMPTY = (1, 0)


def entries(rows, lengths, ids=None, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """(q, gene, s, e) int64 arrays, one per assigned read, in the order the reads first appear.  rows: coverage_restated's 8-tuples.
    lengths: every gene's residues.  ids: None - a row's query is the read's id - or a function of the query (a class run's base + perm[query])."""
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge, a, b in rows:
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge, a, b))
    out = []
    for q, rs in by_read.items():
        best = None
        for s, nmatch, alnlen, bits, loge, a, b in rs:
            if not R.passes(nmatch, alnlen, bits, loge, min_ident, min_aln, min_bits, max_loge):
                continue
            if best is None or best[3] < bits:
                best = (s, a, b, bits)
        if best is None or not 0 <= best[0] < len(lengths):
            continue
        g, a, b = best[:3]
        if not 0 <= a <= b <= int(lengths[g]) - 1:
            a, b = EMPTY
        out.append((int(q) if ids is None else int(ids(q)), int(g), int(a), int(b)))
    cols = list(zip(*out)) if out else [[], [], [], []]
    return tuple(np.array(c, np.int64) for c in cols)


def present(seed, B, q):
    """bool[B, entries]: the weight of read q in replicate b is > 0"""
    return br.weights(seed, np.arange(B, dtype=np.uint64)[:, None], np.asarray(q, np.int64).astype(np.uint64)[None, :]) > 0


def cover(q, g, s, e, lengths, B, seed):
    """cov[g][b]: int64[nseq, B] (the layout of mc_coverage_bootstrap's covered)"""
    out = np.zeros((len(lengths), B), np.int64)
    if not len(q):
        return out
    pm = present(seed, B, q)
    for gene in np.unique(g):
        L = int(lengths[gene])
        depth = np.zeros((B, L), np.int32)
        for i in np.flatnonzero(g == gene):
            if s[i] <= e[i]:
                depth[pm[:, i], int(s[i]):int(e[i]) + 1] += 1
        out[gene] = (depth > 0).sum(axis=1)
    return out


def stats(cov):
    """float64[nseq, 6]: geneboot_restated's six doubles of the covered residues, every replicate used (a scale of ones)"""
    cov = np.asarray(cov, np.int64)
    return GR.stats(cov, np.ones(cov.shape[1], np.float64))


def detected(cov, need):
    """det[g]: the replicates with cov >= need[g]"""
    return (np.asarray(cov, np.int64) >= np.asarray(need, np.int64)[:, None]).sum(axis=1).astype(np.int64)


def need(lengths, F):
    """max(1, ceil(F x length)) in float64: the integer form of abundance.detect's comparison"""
    return np.maximum(1.0, np.ceil(np.float64(F) * np.asarray(lengths, np.float64))).astype(np.int64)
