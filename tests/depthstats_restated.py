"""The statement of csrc/mc_depthstats.h in numpy, written from the statement alone: a prefix sum of a difference array (or of spans), np.sort,
slices.  The tests hold the header's functions (tests/emul/depthstats.cpp), the kernel (tests/emul/device_depthstats.hip) and the library
(Engine.depth_stats) to it."""
import numpy as np

FIGURES = ("median", "trimmed_sum", "low", "high")


def cut_lo_hi(length, keep):
    cut = length * (100 - keep) // 200
    return cut, cut, length - cut


def of_depth(d, keep):
    """(median, trimmed_sum, low, high) of one gene's depths, as Python integers"""
    x = np.sort(np.asarray(d).astype(np.uint64))
    _, lo, hi = cut_lo_hi(len(x), keep)
    return int(x[(len(x) - 1) // 2]), int(x[lo:hi].sum(dtype=np.uint64)), int(x[lo]), int(x[hi - 1])


def depth_stats(depth, lengths, has_reads, keep):
    """The four figures per gene from the depth of every residue, the genes one after the other (Engine.coverage_depth's layout).  has_reads: per
    gene, whether the table the read looks at first holds any - a gene without has four zeros (its depths are zeros anyway)."""
    out = {k: np.zeros(len(lengths), np.int64) for k in FIGURES}
    at = 0
    for s, n in enumerate(lengths):
        if has_reads[s]:
            for k, v in zip(FIGURES, of_depth(depth[at:at + n], keep)):
                out[k][s] = v
        at += n
    assert at == len(depth)
    out["keep"] = keep
    return out


def depth_of_diff(diff, lengths):
    """the depth of every residue from a difference array in k_coverage.h's layout: gene s owns len_s + 1 slots; wrapping 32-bit prefix sums"""
    parts, at = [], 0
    for n in lengths:
        parts.append(np.cumsum(np.asarray(diff[at:at + n], np.uint64)).astype(np.uint64) & np.uint64(0xFFFFFFFF))
        at += n + 1
    assert at == len(diff)
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)


def depth_of_spans(spans, lengths):
    """the depth of every residue from best rows (gene, sstart, send), 0-based and inclusive"""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    d = np.zeros(int(off[-1]) + 1, np.int64)
    for s, a, b in spans:
        d[off[s] + a] += 1
        d[off[s] + b + 1] -= 1
    depth = np.cumsum(d)[:-1]
    assert (depth >= 0).all()
    return depth.astype(np.uint32)


def invariants(st, spanned, max_depth):
    """the invariants of the statement that hold for every keep; [] when all do"""
    bad = []
    if not (st["low"] <= st["median"]).all() or not (st["median"] <= st["high"]).all():
        bad.append("low <= median <= high")
    if not (st["high"] <= np.asarray(max_depth)).all():
        bad.append("high <= max_depth")
    if not (st["trimmed_sum"] <= np.asarray(spanned)).all():
        bad.append("trimmed_sum <= spanned")
    if st["keep"] == 100 and not np.array_equal(st["trimmed_sum"], np.asarray(spanned)):
        bad.append("keep 100: trimmed_sum == spanned")
    return bad


def tad(trimmed_sum, lengths, keep):
    """trimmed_sum / (hi - lo) in float64"""
    kept = np.array([cut_lo_hi(int(n), keep)[2] - cut_lo_hi(int(n), keep)[1] for n in lengths], np.float64)
    return np.asarray(trimmed_sum, np.float64) / kept
