"""The statement of csrc/mc_fold.h restated in numpy - the yardstick of the tests of long genes.

A gene of `length` residues has one segment at offset 0 when length <= L, otherwise segments j = 0, 1, .. at offset j * S, S = L - V, each
of min(L, length - j * S) residues, up to the first that reaches the gene's end.  A span of at most V + 1 residues that starts at residue
a lies inside segment min(a // S, n - 1).  The fold of a row of segment s: subject -> gene[s], sstart and send + off[s], every other field
copied; a subject outside 0 .. nseq - 1 (nseq: the segments) is copied unchanged.  An edge row: sstart == 0 on a segment that is not its
gene's first, or send == the last residue of a segment that is not its gene's last."""
import numpy as np

import order_cases as oc
from microbecensus_amd._native import ROW_DTYPE as ROW

L = oc.define("MC_FOLD_SEG_LEN", "mc_fold.h")
V = oc.define("MC_FOLD_OVERLAP", "mc_fold.h")
MAX_GENE = oc.define("MC_FOLD_MAX_GENE", "mc_fold.h")
MAX_SEGS = oc.define("MC_FOLD_MAX_SEGS", "mc_fold.h")
SEG = np.dtype([("gene", "<i4"), ("off", "<i4"), ("lo", "<i4"), ("hi", "<i4")])     # McFoldSeg


def segments(length, seg_len=L, overlap=V):
    """[(offset, residues)] of a gene's segments"""
    if length <= seg_len:
        return [(0, length)]
    step, out, j = seg_len - overlap, [], 0
    while True:
        out.append((j * step, min(seg_len, length - j * step)))
        if j * step + seg_len >= length:
            return out
        j += 1


def seg_of(a, length, seg_len=L, overlap=V):
    return min(a // (seg_len - overlap), len(segments(length, seg_len, overlap)) - 1)


def records(gene_len, seg_len=L, overlap=V):
    """(McFoldSeg records, seg_gene, seg_off, the segments' residues) of genes of gene_len residues, gene after gene"""
    rec = []
    for g, n in enumerate(gene_len):
        sg = segments(int(n), seg_len, overlap)
        for j, (o, m) in enumerate(sg):
            rec.append((g, o, 0 if j > 0 else -1, m - 1 if j < len(sg) - 1 else -1, m))
    a = np.array([r[:4] for r in rec], np.int32).view(SEG).reshape(-1)
    return a, a["gene"].copy(), a["off"].copy(), np.array([r[4] for r in rec], np.int32)


def fold(rows, rec):
    """the rows folded (a copy), subjects outside the segments untouched"""
    out = rows.copy()
    s = rows["subject"]
    ok = (s >= 0) & (s < len(rec))
    r = rec[np.where(ok, s, 0)]
    out["subject"] = np.where(ok, r["gene"], s)
    out["sstart"] = rows["sstart"] + np.where(ok, r["off"], 0)
    out["send"] = rows["send"] + np.where(ok, r["off"], 0)
    return out


def edge_rows(rows, rec):
    s = rows["subject"]
    ok = (s >= 0) & (s < len(rec))
    r = rec[np.where(ok, s, 0)]
    return int((ok & (((r["lo"] >= 0) & (rows["sstart"] == r["lo"])) | ((r["hi"] >= 0) & (rows["send"] == r["hi"])))).sum())


def same_rows(a, b):
    """two mc_row arrays hold the same bits in every field (the four bytes of padding inside a row belong to no field)"""
    return a.shape == b.shape and all(np.array_equal(a[f].view("u8" if a.dtype[f].itemsize == 8 else "u4"), b[f].view("u8" if b.dtype[f].itemsize == 8 else "u4")) for f in a.dtype.names)


def random_rows(rng, n, nsegs, seg_res, low=0):
    """n mc_row rows of about n / 2 reads, ascending read id: subjects from `low` to three past the segments, spans inside their segments -
    a quarter start at residue 0, a quarter end on the segment's last residue (edge rows where the segment has that edge); rows of a
    subject outside the segments have bits 1, below every other row"""
    rows = np.zeros(n, ROW)
    rows["query"] = np.sort(rng.integers(0, max(1, n // 2), n))
    rows["subject"] = rng.integers(low, nsegs + 3, n)
    inside = (rows["subject"] >= 0) & (rows["subject"] < nsegs)
    m = np.where(inside, seg_res[np.clip(rows["subject"], 0, nsegs - 1)], 50)
    pick = rng.integers(0, 4, n)
    a = np.where(pick == 0, 0, rng.integers(0, 1 << 30, n) % m)
    b = np.where(pick == 1, m - 1, a + rng.integers(0, 1 << 30, n) % (m - a))
    rows["sstart"], rows["send"] = a, b
    rows["alnlen"], rows["nmatch"], rows["bits"], rows["loge"], rows["ident"] = 30, 27, rng.integers(40, 60, n), -5.0, 90.0
    rows["bits"] = np.where(inside, rows["bits"], 1.0)
    return rows
