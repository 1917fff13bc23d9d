"""The abundance statement of csrc/k_abundance.h, restated in plain Python and numpy - the yardstick of the abundance tests.

A row of a read passes when all four of these hold, as exact integer or double comparisons:
    100 * nmatch >= min_ident * alnlen      alnlen >= min_aln      bits >= min_bits      loge <= max_loge
The read's best row is the passing row with the highest bits; on a tie the first in the file's order within the read (classify_reads'
`best < score`, strict).  The read adds 1 to reads[subject] and alnlen to aligned[subject] of its best row, and 1 to assigned.

Rows come from m8 text (rows_from_m8: the reference binary's goldens) or from an mc_row array (rows_from_array).  m8 text prints the
identity with %g (6 significant digits): nmatch = round(identity * alnlen / 100) is exact for alignments of a read (alnlen <= 170)."""
import gzip

import numpy as np


def rows_from_m8(text, names):
    """[(query, subject index, nmatch, alnlen, bits, loge)] of m8 text (str, or the path of a .m8 / .m8.gz file), in file order.
    query: the Query column as it stands (a string); '#' lines are skipped."""
    if "\n" not in text and "\t" not in text:
        with (gzip.open(text, "rt") if text.endswith(".gz") else open(text)) as f:
            text = f.read()
    index = {n: i for i, n in enumerate(names)}
    assert len(index) == len(names)
    out = []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        c = line.split("\t")
        alnlen = int(c[3])
        ident = float(c[2])
        nmatch = int(round(ident * alnlen / 100.0))
        assert abs(nmatch * 100.0 / alnlen - ident) < 1e-3 * max(1.0, ident), line
        out.append((c[0], index[c[1]], nmatch, alnlen, float(c[11]), float(c[10])))
    return out


def rows_from_array(rows):
    """the same of an mc_row array (microbecensus_amd._native.ROW_DTYPE)"""
    return list(zip(*(rows[f].tolist() for f in ("query", "subject", "nmatch", "alnlen", "bits", "loge"))))


def passes(nmatch, alnlen, bits, loge, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    return 100 * nmatch >= min_ident * alnlen and alnlen >= min_aln and bits >= min_bits and loge <= max_loge


def abundance(rows, nseq, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
    """{"reads": int64[nseq], "aligned": int64[nseq], "assigned": int} of rows as rows_from_m8 / rows_from_array give them."""
    assert isinstance(min_ident, int) and isinstance(min_aln, int)
    by_read = {}
    for q, s, nmatch, alnlen, bits, loge in rows:           # (dicts keep the order of first appearance: a read's rows stay in file order)
        by_read.setdefault(q, []).append((s, nmatch, alnlen, bits, loge))
    reads = np.zeros(nseq, np.int64)
    aligned = np.zeros(nseq, np.int64)
    assigned = 0
    for q, rs in by_read.items():
        best = None
        for s, nmatch, alnlen, bits, loge in rs:
            if not passes(nmatch, alnlen, bits, loge, min_ident, min_aln, min_bits, max_loge):
                continue
            if best is None or best[2] < bits:
                best = (s, alnlen, bits)
        if best is not None:
            reads[best[0]] += 1
            aligned[best[0]] += best[1]
            assigned += 1
    return {"reads": reads, "aligned": aligned, "assigned": assigned}


def cutoffs_clear_of_printed_values(rows, min_bits=0.0, max_loge=1.0, margin=1e-3):
    """m8 text prints bits and log(e) with %g: a cut-off is safe to compare against the printed values when none of them lies within
    `margin` of it (on the passing side they may - a printed value at least margin ABOVE min_bits ... - so: strictly, none within)."""
    bits = np.array([r[4] for r in rows])
    loge = np.array([r[5] for r in rows])
    return bool((np.abs(bits - min_bits) > margin).all()) and bool((np.abs(loge - max_loge) > margin).all())
