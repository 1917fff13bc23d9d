"""The synthetic cases of the tie accounting (csrc/k_ties.h), shared by the CPU run of the walk (tests/emul/ties.cpp, test_ties_host.py)
and the kernel's run on the device (tests/emul/device_ties.hip, test_gpu_ties_units.py): the smallest shapes at which the walk can go
wrong, each with what the statement says about it.  A case is a dict: lengths, rows (an mc_row array), group_of / ngroups (or None / 0),
cov (whether the any-depth is kept) and cut (the cut-offs).  expected() restates a case once and keeps the result."""
import numpy as np

import abundance_restated as R
import coverage_restated as V
import ties_restated as T
from microbecensus_amd._native import ROW_DTYPE

PARS = np.dtype([("min_ident", "<i4"), ("min_aln", "<i4"), ("min_bits", "<f8"), ("max_loge", "<f8")])   # McAbundPars
assert ROW_DTYPE.itemsize == 72 and PARS.itemsize == 24
ONE = 1 << 32
CUT = dict(min_ident=60, min_aln=25)


def rows_of(spec):
    """mc_row array of (query, subject, sstart, send[, bits[, nmatch, alnlen]]): bits 50, 27 of 30 identical by default"""
    arr = np.zeros(len(spec), ROW_DTYPE)
    for i, r in enumerate(spec):
        q, s, a, b = r[:4]
        bits = r[4] if len(r) > 4 else 50.0
        nmatch, alnlen = r[5:7] if len(r) > 5 else (27, 30)
        arr[i] = (q, s, nmatch * 100.0 / alnlen, alnlen, alnlen - nmatch, 0, 1, 90, a, b, -5.0, bits, 100, nmatch)
    return arr


def case(lengths, rows, group_of=None, ngroups=0, cov=True, cut=None):
    return {"lengths": [int(x) for x in lengths], "rows": rows if isinstance(rows, np.ndarray) else rows_of(rows),
            "group_of": None if group_of is None else np.asarray(group_of, np.int32), "ngroups": ngroups, "cov": cov, "cut": dict(cut or {})}


# ---- the small shapes, all in one database of eight genes in four groups ----------------------------------------------------------
B_LENGTHS = [30, 1, 40, 64, 65, 20, 50, 33]
B_GROUPS = [0, 0, 1, 1, 2, 2, 3, 3]
B_ROWS = [
    (0, 0, 0, 29, 60.0),                                                                       # one read, one row, a span ending at len - 1
    (1, 0, 5, 9, 60.0), (1, 2, 35, 39, 60.0),                                                  # k = 2, across two groups; both genes marked
    (2, 2, 0, 9, 55.0), (2, 3, 1, 63, 55.0), (2, 5, 2, 19, 55.0),                              # k = 3: the remainder 1 to gene 2
    (3, 0, 0, 5), (3, 2, 0, 5), (3, 3, 0, 5), (3, 4, 0, 64), (3, 5, 0, 5), (3, 6, 0, 5),       # k = 6
    (4, 7, 0, 5), (4, 0, 0, 5), (4, 2, 0, 5), (4, 3, 0, 5), (4, 4, 0, 5), (4, 5, 0, 5), (4, 6, 0, 5),   # k = 7; the first tied subject is gene 7
    (5, 0, 0, 4, 70.0), (5, 1, 0, 0, 70.0), (5, 0, 10, 20, 70.0),                              # s0, s1, s0: k = 2 inside one group; s0 by its first row; a gene of one residue
    (6, 3, 0, 9, 40.0), (6, 4, 0, 9, 45.0), (6, 5, 0, 9, 70.0), (6, 6, 0, 9, 50.0), (6, 3, 20, 29, 70.0),   # lower scores in front; the tied rows not adjacent
    (7, 2, 0, 9, 60.0), (7, 3, 0, 9, 60.0, 10, 30),                                            # a tied row that fails min_ident 60
    (8, 4, 0, 9, 90.0, 10, 30), (8, 5, 0, 9, 50.0), (8, 6, 0, 9, 50.0),                        # a higher-scoring row that fails it lowers T
    (9, 8, 0, 9, 80.0), (9, 0, 0, 9, 80.0),                                                    # the first-rule best row's subject is nseq: nothing anywhere
    (10, 1, 0, 0, 70.0), (10, 9, 0, 9, 70.0), (10, 32767, 0, 9, 70.0), (10, 0, 20, 29, 70.0),  # tied rows with subjects >= nseq behind an in-range first one
    (11, 6, 40, 49, 66.0), (11, 7, 30, 32, 66.0),                                              # k = 2 inside group 3; both spans end at len - 1
    (12, 0, 0, 9, 99.0, 5, 30),                                                                # no passing row under the cut-offs
    (13, 4, 3, 9, 52.0), (13, 5, 10, 25, 52.0),                                                # gene 5 has 20 residues: the span marks nothing, the read counts
]


def basics(groups=True, cov=True, cut=None):
    return case(B_LENGTHS, B_ROWS, B_GROUPS if groups else None, 4 if groups else 0, cov, cut)


def row_counts(nrows):
    """nrows rows in all (1, 256, 257): reads of two tied rows, and one read of one row at the end when nrows is odd"""
    spec = []
    for q in range(nrows // 2):
        spec += [(q, q % 3, q % 7, q % 7 + 20, 44.0), (q, 3 + q % 2, 0, 9, 44.0)]
    if nrows % 2:
        spec.append((nrows // 2, 2, 1, 5, 44.0))
    assert len(spec) == nrows
    return case([40, 40, 40, 30, 30], spec, [0, 0, 0, 1, 1], 2)


def boundaries():
    """rows 0 .. 249 one per read; a read of 12 rows over rows 250 .. 261 - across the 256-thread workgroup boundary - whose tied rows
    lie on both sides of it (rows 252, 255, 256, 260; row 256 repeats row 252's subject); reads of one row up to row 510; a read whose
    rows end exactly at nrows with its tied rows last; and a read that BEGINS at the last row"""
    spec = [(q, q % 4, q % 10, q % 10 + 15) for q in range(250)]
    tied = {252: 0, 255: 1, 256: 0, 260: 3}
    for r in range(250, 262):
        spec.append((250, tied[r], r - 250, r - 230, 80.0) if r in tied else (250, r % 4, 0, 9, 30.0 + r - 250))
    spec += [(q, q % 4, 1, 8) for q in range(251, 500)]
    spec += [(500, 2, 0, 9, 20.0), (500, 1, 0, 9, 61.0), (500, 3, 5, 39, 61.0)]
    spec += [(501, 3, 39, 39, 33.0)]
    c = case([40, 40, 40, 40], spec, [0, 1, 0, 1], 2)
    assert c["rows"]["query"][249] == 249 and c["rows"]["query"][250] == c["rows"]["query"][261] == 250 and c["rows"]["query"][-1] == 501 and c["rows"]["query"][-2] == 500
    return c


def long_span():
    """one read of 200 rows between two short reads: rows at the top at positions 3, 10, 63, 64, 65, 130 (the subject of position 3
    again) and 199 of the read, lower-scoring rows everywhere else, and at position 100 a row of a higher score that fails min_ident:
    the rows at the top lie far apart, with a repeated subject and rows that are not at the top between them"""
    top = {3: 0, 10: 1, 63: 2, 64: 3, 65: 4, 130: 0, 199: 5}
    spec = [(0, 6, 0, 9, 80.0), (0, 7, 0, 9, 80.0)]
    for p in range(200):
        if p in top:
            spec.append((1, top[p], p % 7, p % 7 + 10, 80.0))
        elif p == 100:
            spec.append((1, 6, 0, 9, 95.0, 10, 30))
        else:
            spec.append((1, p % 8, 0, 9, 30.0 + (p % 40)))
    spec += [(2, 7, 1, 5, 50.0)]
    return case([30] * 8, spec, [0, 0, 0, 1, 1, 1, 2, 2], 3, cut=CUT)


def wide(nreads, nsub):
    """nreads reads of 500 tied rows each over nsub subjects (500: every subject once; 250: every subject twice, the second round behind
    the first) - the walk's worst case"""
    one = rows_of([(0, k % nsub, k % 3, k % 3 + 4 + k // nsub, 77.0) for k in range(500)])
    rows = np.tile(one, nreads)
    rows["query"] = np.repeat(np.arange(nreads), 500)
    return case([12] * nsub, rows, [s % 5 for s in range(nsub)], 5)


def many(nreads=100_000):
    """nreads reads all tied on the same two subjects of one group: sums of 2^31 per read per subject"""
    rows = np.tile(rows_of([(0, 1, 2, 4, 50.0), (0, 2, 0, 2, 50.0)]), nreads)
    rows["query"] = np.repeat(np.arange(nreads), 2)
    return case([5, 5, 3], rows, [0, 1, 1], 2)


# ---- the files the two harnesses read and write ---------------------------------------------------------------------------------------
def sections_in(c):
    pars = np.zeros(1, PARS)
    cut = c["cut"]
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    off = np.zeros(len(c["lengths"]) + 1, np.uint32)
    off[1:] = np.cumsum(c["lengths"])
    group = np.zeros(0, np.int32) if c["group_of"] is None else c["group_of"]
    return [pars, off, c["rows"], group, np.array([c["ngroups"], int(c["cov"])], np.int32)]


_expected = {}


def expected(name, c):
    """(the restated ties, the restated counts, the restated coverage) of a case - computed once per name, shared, never changed"""
    if name not in _expected:
        nseq, rows = len(c["lengths"]), c["rows"]
        t = T.ties(V.rows_from_array(rows), c["lengths"], c["group_of"], c["ngroups"], **c["cut"])
        ab = R.abundance(R.rows_from_array(rows), max(nseq, int(rows["subject"].max()) + 1), **c["cut"])
        cv = V.coverage(V.rows_from_array(rows), c["lengths"], **c["cut"])
        _expected[name] = (t, ab, cv)
    return _expected[name]


def check_ties(c, want, tab, share, gu, depth_any=None):
    """what either harness wrote against the restatement, and the statement's invariants on it"""
    t, ab, cv = want
    nseq = len(c["lengths"])
    reads = ab["reads"][:nseq]
    assigned = int(reads.sum())
    got = {"candidates": tab[0:2 * nseq:2].astype(np.int64), "unique": tab[1:2 * nseq:2].astype(np.int64), "share": share, "group_unique": gu.astype(np.int64),
           "ambiguous": int(tab[2 * nseq]), "group_ambiguous": int(tab[2 * nseq + 1])}
    for k in T.COUNTERS + ("ambiguous", "group_ambiguous"):
        assert np.array_equal(got[k], t[k]), "%s: %s, the restatement %s" % (k, got[k], t[k])
    assert len(t["sets"]) == assigned
    if depth_any is not None:
        assert np.array_equal(depth_any, t["depth_any"] if c["cov"] else np.zeros_like(t["depth_any"])), "any-depth"
        got["depth_any"] = depth_any
    assert T.invariants(dict(got, k=t["k"]), reads, assigned, c["group_of"], cv["depth"] if c["cov"] and depth_any is not None else None) == []
    return got
