"""The statement of csrc/mc_groupboot.h restated in plain Python and numpy, on top of tests/geneboot_restated.py - the yardstick of the
group bootstrap's tests.

c[s][b] are the gene bootstrap's replicate counts (geneboot_restated.counts).  A group's replicate count C[G][b] is the sum of its members'
counts.  Its replicate value y[G][b] of a used b starts at 0.0 and takes the members in ascending gene index: each adds
(float64(c[s][b]) * scale[b]) / gene_kb[s] - a multiplication, a division and an addition, three IEEE operations in numpy; of an unused b
it stays 0.0.  The six doubles of a group are geneboot_restated's of a gene, made from y instead of c * scale: the same 256 partials, the
same halving tree, the same indices of the order statistics.  Everything is compared with the library bit for bit."""
import numpy as np

import geneboot_restated as GR


def values(cmat, scale, group_of, ngroups, gene_kb, reverse=False):
    """(y float64[ngroups, B], C int64[ngroups, B]) of counts int64[nseq, B]; reverse: the members in DESCENDING gene index - not the rule,
    and there to show that the order is under test"""
    cmat = np.asarray(cmat, np.int64)
    scale, kb = np.asarray(scale, np.float64), np.asarray(gene_kb, np.float64)
    use = GR.used(scale)
    y, C = np.zeros((ngroups, cmat.shape[1]), np.float64), np.zeros((ngroups, cmat.shape[1]), np.int64)
    order = range(len(cmat) - 1, -1, -1) if reverse else range(len(cmat))
    with np.errstate(all="ignore"):
        for s in order:
            G = int(group_of[s])
            v = cmat[s].astype(np.uint64).astype(np.float64) * scale
            r = v / kb[s]
            y[G] = np.where(use, y[G] + r, y[G])
            C[G] += cmat[s]
    return y, C


def group_stats(y, scale):
    """the six doubles of one group: y float64[B], scale float64[B]"""
    scale = np.asarray(scale, np.float64)
    use = GR.used(scale)
    m = int(use.sum())
    if m == 0:
        return np.full(6, np.nan)
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        total = GR._ordered_sum(y, use)
        d = y - total / np.float64(m)
        m2 = GR._ordered_sum(d * d, use)
    x = np.sort(y[use])
    return np.array([total, m2] + [x[GR.index(m, k)] for k in (2, 3, 4, 5)], np.float64)


def stats(ymat, scale):
    """float64[ngroups, 6] of values float64[ngroups, B]; a group without reads is computed like any other (zeros, or NaN with m == 0)"""
    cache = {}
    out = np.zeros((len(ymat), 6), np.float64)
    for G, y in enumerate(np.asarray(ymat, np.float64)):
        key = y.tobytes()
        if key not in cache:
            cache[key] = group_stats(y, scale)
        out[G] = cache[key]
    return out


def plan(reads, group_of, ngroups, gene_kb):
    """mc_grb_plan: (gidx int32[ngroups], start uint32[ngrp + 1], member uint32, kb float64) - the groups with reads numbered ascending, and
    their members with reads as compact gene indices, group by group, ascending gene index within a group"""
    have = np.asarray(reads) > 0
    idx = np.where(have, np.cumsum(have) - 1, -1)
    live = sorted(set(int(group_of[s]) for s in np.flatnonzero(have)))
    gidx = np.full(ngroups, -1, np.int32)
    gidx[live] = np.arange(len(live))
    start, member, kb = [0], [], []
    for G in live:
        ms = [s for s in np.flatnonzero(have) if group_of[s] == G]
        member += [int(idx[s]) for s in ms]
        kb += [float(gene_kb[s]) for s in ms]
        start.append(len(member))
    return gidx, np.array(start, np.uint32), np.array(member, np.uint32), np.array(kb, np.float64)
