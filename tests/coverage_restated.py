"""The coverage statement of csrc/k_coverage.h, restated in plain Python - the yardstick of the coverage tests.

Which row counts: a read's best row is the one tests/abundance_restated.py defines (the four cut-offs, the highest bits, the first on a
tie).  What it adds: RAPsearch2's subject coordinates are 0-based and inclusive (mc_row.sstart / send; columns 9 and 10 of its m8); the
best row adds 1 to depth[subject][p] for every p in sstart .. send, both ends included.  (A span that does not lie inside its gene - no
row of the engine - adds nothing to the depth.)  Per gene: covered = the number of p with depth > 0, spanned = the sum of depth over p,
max_depth = the maximum of depth over p.

The depth is built residue by residue in a plain loop: no difference array, no prefix sum - nothing the kernels do."""
import gzip

import numpy as np

import abundance_restated as R


def rows_from_m8(text, names):
    """[(query, subject index, nmatch, alnlen, bits, loge, sstart, send)] of m8 text (str, or the path of a .m8 / .m8.gz file), in file
    order: what abundance_restated.rows_from_m8 parses, and columns 9 and 10 as they stand (0-based, inclusive)."""
    if "\n" not in text and "\t" not in text:
        with (gzip.open(text, "rt") if text.endswith(".gz") else open(text)) as f:
            text = f.read()
    spans = []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        c = line.split("\t")
        spans.append((int(c[8]), int(c[9])))
    base = R.rows_from_m8(text + "\n", names)                   # (text, never a path: the file has been read above)
    assert len(base) == len(spans)
    return [b + s for b, s in zip(base, spans)]


def rows_from_array(rows):
    """the same of an mc_row array (microbecensus_amd._native.ROW_DTYPE)"""
    return list(zip(*(rows[f].tolist() for f in ("query", "subject", "nmatch", "alnlen", "bits", "loge", "sstart", "send"))))


def best_rows(rows, nseq=None, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """[(subject, sstart, send)]: every read's best row, in the order the reads first appear.  nseq: best rows whose subject is not below
    it are left out (the counting kernel ignores them)."""
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge, a, b in rows:
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge, a, b))
    out = []
    for rs in by_read.values():
        best = None
        for s, nmatch, alnlen, bits, loge, a, b in rs:
            if not R.passes(nmatch, alnlen, bits, loge, min_ident, min_aln, min_bits, max_loge):
                continue
            if best is None or best[3] < bits:
                best = (s, a, b, bits)
        if best is not None and (nseq is None or 0 <= best[0] < nseq):
            out.append(best[:3])
    return out


def coverage(rows, lengths, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """{"covered", "spanned", "max_depth": int64[nseq]; "depth": uint32[sum(lengths)], the genes one after the other;
    "best": the best rows} of rows as rows_from_m8 / rows_from_array give them.  lengths: every gene's residues."""
    lengths = [int(x) for x in lengths]
    depth = [[0] * n for n in lengths]
    best = best_rows(rows, len(lengths), min_ident, min_aln, min_bits, max_loge)
    for s, a, b in best:
        if not 0 <= a <= b <= lengths[s] - 1:
            continue
        d = depth[s]
        for p in range(a, b + 1):
            d[p] += 1
    covered = np.array([sum(1 for v in d if v > 0) for d in depth], np.int64)
    spanned = np.array([sum(d) for d in depth], np.int64)
    max_depth = np.array([max(d) if d else 0 for d in depth], np.int64)
    flat = np.array([v & 0xFFFFFFFF for d in depth for v in d], np.uint32)
    return {"covered": covered, "spanned": spanned, "max_depth": max_depth, "depth": flat, "best": best}


def invariants(cov, reads, lengths):
    """the statement's invariants, as a list of those that do not hold"""
    lengths = np.asarray(lengths, np.int64)
    bad = []
    if not np.array_equal(cov["covered"] > 0, np.asarray(reads) > 0):
        bad.append("covered > 0 iff reads > 0")
    if not (cov["covered"] <= np.minimum(lengths, cov["spanned"])).all():
        bad.append("covered <= min(len, spanned)")
    if not (cov["max_depth"] <= np.asarray(reads)).all():
        bad.append("max_depth <= reads")
    if not int(cov["covered"].sum()) <= int(cov["spanned"].sum()):
        bad.append("sum(covered) <= sum(spanned)")
    return bad
