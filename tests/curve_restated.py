"""The curve statement of csrc/k_curve.h, restated in plain Python - the yardstick of the curve tests.

Points n_0 <= ... <= n_{K-1}, each >= 1, repeats allowed.  A read's global id q is its row's query (an int).  A read's best row is the one
tests/abundance_restated.py defines.  A read with a best row falls into bin b(q) = the number of k with n_k <= q (0 .. K; K: behind the
last point), adds 1 to bin_reads[b][subject] and alnlen to bin_aligned[b][subject], and - with coverage - lowers first[subject][p] to
min(first, q) for every p in sstart .. send (a span that does not lie inside its gene marks nothing).  At read time, per point k and gene
s: reads_k = the sum of bin_reads over b <= k, aligned_k the same of bin_aligned, covered_k = the number of p with first < n_k (a residue
never covered counts nowhere), assigned_k = the sum of reads_k over s, beyond = the sum of bin K over s.

Everything is built read by read and residue by residue in plain loops: no histogram, no scan, no binary search - nothing the kernels
do."""
import numpy as np

import abundance_restated as R


def bin_of(points, q):
    """the number of k with n_k <= q"""
    return sum(1 for n in points if n <= q)


def best_of_reads(rows, nseq, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """[(q, subject, alnlen, sstart, send)]: every read's best row with its id, in the order the reads first appear; rows as
    coverage_restated.rows_from_m8 / rows_from_array give them with an int query.  Best rows of a subject outside 0 .. nseq - 1 are left
    out (the kernels ignore them)."""
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge, a, b in rows:
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge, a, b))
    out = []
    for q, rs in by_read.items():
        best = None
        for s, nmatch, alnlen, bits, loge, a, b in rs:
            if not R.passes(nmatch, alnlen, bits, loge, min_ident, min_aln, min_bits, max_loge):
                continue
            if best is None or best[5] < bits:
                best = (q, s, alnlen, a, b, bits)
        if best is not None and 0 <= best[1] < nseq:
            out.append(best[:5])
    return out


def curve(rows, lengths, points, coverage=True, **cut):
    """{"bin_reads", "bin_aligned": int64[K + 1, nseq]; "first": a list per gene of ints or None (coverage) ; "reads", "aligned", "covered":
    int64[K, nseq] (covered all zero without coverage); "assigned": int64[K]; "beyond": int; "best": the best rows}"""
    lengths = [int(x) for x in lengths]
    points = [int(x) for x in points]
    K, nseq = len(points), len(lengths)
    assert K >= 1 and points[0] >= 1 and all(a <= b for a, b in zip(points, points[1:]))
    bin_reads = np.zeros((K + 1, nseq), np.int64)
    bin_aligned = np.zeros((K + 1, nseq), np.int64)
    first = [[None] * n for n in lengths]
    best = best_of_reads(rows, nseq, **cut)
    for q, s, alnlen, a, b in best:
        assert 0 <= q < 2 ** 31
        bq = bin_of(points, q)
        bin_reads[bq, s] += 1
        bin_aligned[bq, s] += alnlen
        if coverage and 0 <= a <= b <= lengths[s] - 1:
            f = first[s]
            for p in range(a, b + 1):
                if f[p] is None or q < f[p]:
                    f[p] = q
    reads = np.zeros((K, nseq), np.int64)
    aligned = np.zeros((K, nseq), np.int64)
    covered = np.zeros((K, nseq), np.int64)
    for k in range(K):
        for s in sorted({r[1] for r in best}):                        # (a gene without a best row keeps its zeros)
            reads[k, s] = sum(int(bin_reads[b, s]) for b in range(k + 1))
            aligned[k, s] = sum(int(bin_aligned[b, s]) for b in range(k + 1))
            covered[k, s] = sum(1 for f in first[s] if f is not None and f < points[k])
    return {"bin_reads": bin_reads, "bin_aligned": bin_aligned, "first": first, "reads": reads, "aligned": aligned, "covered": covered,
            "assigned": reads.sum(axis=1), "beyond": int(bin_reads[K].sum()), "best": best, "points": points}


def first_flat(cv):
    """first as the device keeps it: uint32, the genes one after the other, 0xFFFFFFFF where no read has covered"""
    return np.array([0xFFFFFFFF if f is None else f for g in cv["first"] for f in g], np.uint32)


def invariants(cv, ab_reads, ab_aligned, cov_covered=None, coverage=True):
    """the statement's invariants, as a list of those that do not hold.  ab_reads / ab_aligned: the count table of the same rows
    (abundance_restated); cov_covered: coverage_restated's covered of the same rows, compared when no read lies behind the last point."""
    bad = []
    if (np.diff(cv["reads"], axis=0) < 0).any() or (np.diff(cv["covered"], axis=0) < 0).any():
        bad.append("reads_k and covered_k do not decrease in k")
    if coverage and not np.array_equal(cv["covered"] > 0, cv["reads"] > 0):
        bad.append("covered_k > 0 iff reads_k > 0")
    if not (np.array_equal(cv["bin_reads"].sum(axis=0), ab_reads) and np.array_equal(cv["bin_aligned"].sum(axis=0), ab_aligned)):
        bad.append("the sum over all K + 1 bins is the count table")
    if all(q < cv["points"][-1] for q, *_ in cv["best"]):
        if cv["beyond"] != 0 or not (np.array_equal(cv["reads"][-1], ab_reads) and np.array_equal(cv["aligned"][-1], ab_aligned)):
            bad.append("beyond == 0 and the last row is the count table")
        if coverage and cov_covered is not None and not np.array_equal(cv["covered"][-1], cov_covered):
            bad.append("the last row's covered is the coverage's")
    elif cv["beyond"] == 0:
        bad.append("a read behind the last point and beyond == 0")
    return bad
