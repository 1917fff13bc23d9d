"""The identity statement of csrc/mc_identity.h, restated in plain Python - the yardstick of the identity tests.

Which row counts: a read's best row is the one tests/abundance_restated.py defines (the four cut-offs, the highest bits, the first on a
tie), under 0 <= subject < nseq.  What it adds: bin = 0 if alnlen < 1 else (100 * nmatch) // alnlen (0 .. 100); hist[subject][bin] += 1,
matched[subject] += nmatch, mismatched[subject] += mismatch, gap_opens[subject] += gapopen.  Per gene with n reads: ident_min / ident_max
the lowest / highest non-empty bin, ident_median the smallest bin whose cumulative count reaches (n - 1) // 2 + 1, ge[j] the reads in bins
>= level[j]; a gene without reads has -1 for the three bins.

The figures are taken from the sorted list of a gene's bins, one entry per read: no histogram walk, no prefix sum - nothing the kernels do."""
import gzip

import numpy as np

import abundance_restated as R

BINS = 101
NONE = -1


def rows_from_m8(text, names):
    """[(query, subject index, nmatch, alnlen, bits, loge, mismatch, gapopen)] of m8 text (str, or the path of a .m8 / .m8.gz file), in file
    order: what abundance_restated.rows_from_m8 parses, and columns 5 and 6 as they stand."""
    if "\n" not in text and "\t" not in text:
        with (gzip.open(text, "rt") if text.endswith(".gz") else open(text)) as f:
            text = f.read()
    more = []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        c = line.split("\t")
        more.append((int(c[4]), int(c[5])))
    base = R.rows_from_m8(text + "\n", names)                   # (text, never a path: the file has been read above)
    assert len(base) == len(more)
    return [b + m for b, m in zip(base, more)]


def rows_from_array(rows):
    """the same of an mc_row array (microbecensus_amd._native.ROW_DTYPE)"""
    return list(zip(*(rows[f].tolist() for f in ("query", "subject", "nmatch", "alnlen", "bits", "loge", "mismatch", "gapopen"))))


def bin_of(nmatch, alnlen):
    """the floor of the identity in percent; of a row no engine makes (nmatch outside 0 .. alnlen) the nearest of 0 and 100"""
    if alnlen < 1 or nmatch < 0:
        return 0
    return 100 if nmatch >= alnlen else (100 * nmatch) // alnlen


def best_rows(rows, nseq=None, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """[(subject, nmatch, alnlen, mismatch, gapopen)]: every read's best row, in the order the reads first appear; nseq: best rows whose
    subject does not lie in 0 .. nseq - 1 are left out"""
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge, mis, gap in rows:
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge, mis, gap))
    out = []
    for rs in by_read.values():
        best = None
        for s, nmatch, alnlen, bits, loge, mis, gap in rs:
            if not R.passes(nmatch, alnlen, bits, loge, min_ident, min_aln, min_bits, max_loge):
                continue
            if best is None or best[0] < bits:
                best = (bits, s, nmatch, alnlen, mis, gap)
        if best is not None and (nseq is None or 0 <= best[1] < nseq):
            out.append(best[1:])
    return out


def figures_of(bins, levels=()):
    """(ident_min, ident_median, ident_max, [ge per level]) of one gene's reads, given as the list of their bins"""
    b = sorted(int(x) for x in bins)
    if not b:
        return NONE, NONE, NONE, [0] * len(levels)
    return b[0], b[(len(b) - 1) // 2], b[-1], [sum(1 for x in b if x >= t) for t in levels]


def figures_of_hist(hist, levels=()):
    """the same of one histogram of 101 counts"""
    assert len(hist) == BINS
    return figures_of([b for b, c in enumerate(hist) for _ in range(int(c))], levels)


def identity(rows, nseq, levels=(), min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """{"hist": uint32[nseq, 101]; "matched", "mismatched", "gap_opens": int64[nseq]; "ident_min", "ident_median", "ident_max": int32[nseq];
    "ge": int64[nseq, len(levels)]; "best": the best rows} of rows as rows_from_m8 / rows_from_array give them"""
    best = best_rows(rows, nseq, min_ident, min_aln, min_bits, max_loge)
    per = [[] for _ in range(nseq)]
    out = {k: np.zeros(nseq, np.int64) for k in ("matched", "mismatched", "gap_opens")}
    hist = np.zeros((nseq, BINS), np.uint32)
    for s, nmatch, alnlen, mis, gap in best:
        b = bin_of(nmatch, alnlen)
        per[s].append(b)
        hist[s, b] += 1
        out["matched"][s] += nmatch
        out["mismatched"][s] += mis
        out["gap_opens"][s] += gap
    figs = [figures_of(p, levels) for p in per]
    for k, name in enumerate(("ident_min", "ident_median", "ident_max")):
        out[name] = np.array([f[k] for f in figs], np.int32)
    out["ge"] = np.array([f[3] for f in figs], np.int64).reshape(nseq, len(levels))
    out.update({"hist": hist, "best": best})
    return out


def invariants(idn, reads, aligned, levels=()):
    """the statement's invariants, as a list of those that do not hold; idn: identity()'s dict or Engine.identity()'s with "hist" added"""
    reads, aligned = np.asarray(reads, np.int64), np.asarray(aligned, np.int64)
    bad, has = [], reads > 0
    if not np.array_equal(idn["hist"].astype(np.int64).sum(axis=1), reads):
        bad.append("sum(hist) == reads")
    if not (idn["matched"] <= aligned).all():
        bad.append("matched_aa <= aligned_aa")
    lo, med, hi = (np.asarray(idn[k], np.int64) for k in ("ident_min", "ident_median", "ident_max"))
    if not ((lo[has] <= med[has]) & (med[has] <= hi[has])).all() or not ((lo[~has] == NONE) & (med[~has] == NONE) & (hi[~has] == NONE)).all():
        bad.append("ident_min <= ident_median <= ident_max, -1 without reads")
    m, a = idn["matched"][has], aligned[has]                     # ident_min <= 100 m / a < ident_max + 1, in integers
    if not ((lo[has] * a <= 100 * m) & (100 * m < (hi[has] + 1) * a)).all():
        bad.append("ident_min <= ident_mean < ident_max + 1")
    ge = np.asarray(idn["ge"], np.int64)
    if ge.shape[1] > 1 and not (ge[:, 1:] <= ge[:, :-1]).all():
        bad.append("ge is non-increasing in T")
    if len(levels) and levels[0] == 0 and not np.array_equal(ge[:, 0], reads):
        bad.append("ge at level 0 equals reads")
    return bad
