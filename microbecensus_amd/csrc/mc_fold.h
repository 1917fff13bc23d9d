// mc_fold.h - genes longer than one database sequence of the engine (mc_set_gene_fold): how a long gene is cut into overlapping SEGMENTS,
// each an ordinary sequence of the index, and how a row found on a segment is FOLDED back onto its gene before any abundance kernel sees
// it.  Same conventions as mc_classes.h and mc_geneboot.h: host and device code alike, no HIP include of its own - k_fold.h runs it on the
// device, g++ compiles the very same text into tests/emul/fold.cpp, and tests/fold_restated.py restates it in numpy.
//
// ---- THE STATEMENT ----------------------------------------------------------------------------------------------------------------
// Constants: L = MC_FOLD_SEG_LEN, the longest segment; V = MC_FOLD_OVERLAP, what consecutive segments share; the step S = L - V.
// THE SEGMENTS of a gene of len residues (mc_fold_nsegs, mc_fold_seg_off, mc_fold_seg_len; every function takes L and V as arguments,
// the library passes the constants): len <= L: one segment at offset 0.  Otherwise segments j = 0, 1, .. at offset j * S, each of
// min(L, len - j * S) residues; the last one is the first that reaches len: n = 1 + ceil((len - L) / S) of them.  Consecutive segments
// share exactly V residues, every segment but the last has L residues, and the last has more than V (it reaches past its predecessor).
// THE SEGMENT ARGUMENT.  A span [a, b] of the gene, 0 <= a <= b <= len - 1, with b - a + 1 <= V + 1 residues lies wholly inside segment
// j = min(floor(a / S), n - 1) (mc_fold_seg_of):
//     j = floor(a / S) < n - 1:  j S <= a, and b <= a + V <= j S + (S - 1) + V = j S + L - 1, the segment's last residue (it has L).
//     otherwise j = n - 1:       (n - 1) S <= a by the floor, and b <= len - 1, the last segment's last residue.
// So whatever alignment the unsplit database holds with a subject span of at most V + 1 residues, one segment holds all of it.
// THE FOLD OF A ROW (mc_fold_row): with seg[s] = {gene, off, ..} the record of segment s (mc_fold_seg),
//     subject' = seg[subject].gene        sstart' = sstart + seg[subject].off        send' = send + seg[subject].off
// and every other field is copied.  A row whose subject lies outside 0 .. nseq - 1 (nseq: the SEGMENTS of the index) is copied unchanged:
// the counting kernels ignore it as they did.
// AN EDGE ROW (mc_fold_edge) is a row of a segment in 0 .. nseq - 1 whose span touches an INTERIOR edge: sstart == 0 on a segment that is
// not its gene's first, or send == the segment's last residue on a segment that is not its gene's last.  An alignment that stops there may
// have stopped because the segment did: the number of such rows (edge_rows) is the witness that V was wide enough for the reads at hand.
// It is no filter: the row is folded and counted like any other.
// GENE-SPACE LIMITS (mc_set_gene_fold checks them): at most 32,767 segments in all (the engine's), a gene has at most MC_FOLD_MAX_GENE =
// 65,535 residues, and the coverage offsets, the sum of len + 1 over the genes, stay below 2^32.
//
// ---- L: WHAT THE ENGINE TAKES -----------------------------------------------------------------------------------------------------
// The posting word holds 11 bits of position (MC_POST8, mc_core.h: 2,047 residues), but the engine opens no database with a sequence
// longer than the full-size workspace of its gapped stage: MC_GAP_W - 8 = 1,192 residues (k_gapped.h; open_impl, mc_hip.hip, refuses
// "marker longer than the gapped-extension workspace").  A segment is a sequence of the engine, so L is the smaller of the two, 1,192;
// mc_hip.hip holds the static_assert that ties L to MC_GAP_W, beside that check (this header has no HIP include and cannot see k_gapped.h).
//
// ---- V: WHAT CAN AND WHAT CANNOT BE DERIVED ------------------------------------------------------------------------------------------
// The subject span of an alignment is its substitution columns plus the subject residues opposite gaps in the query.  The longest read has
// 3 x MC_MAXAA = 510 bases: at most MC_MAXAA = 170 query residues, so at most 170 substitution columns.  What the gapped stage can insert:
//   * a flank is kept only with a gain > 0 (k_gap_emit), a substitution gains at most 11 (BLOSUM62, W / W), a flank has at most
//     MC_MAXAA - 1 = 169 query residues: the gap costs of a flank stay below 11 x 169 = 1,859;
//   * a gap run of g columns costs MC_GAP_OPEN + g x MC_GAP_EXT = 11 + g, and the right growth of a row (mc_align_gapped, mc_core.h) ends at
//     the first cell more than xdrop_gapped = 26.98 under the best: 11 + g <= 26 for a live cell, so g <= 15, plus the one cell that ends
//     the band: at most 16 columns for 27 score.
// So the scoring system allows up to floor(1,859 x 16 / 27) = 1,101 subject-only columns, a span of 1,271 residues - tryptophan runs
// bridged by gaps of 16 - which is MORE than a whole segment.  NO overlap below L bounds every alignment the engine can make; the bound
// the overlap was meant to be does not exist, and mc_align_gapped's own comment says so ("nothing bounds it below the subject length").
// V is therefore a choice, not a proof: V = 512, the read's 510 bases rounded up to a multiple of 64 - a span of up to V + 1 = 513
// residues is safe by the segment argument, i.e. every alignment with at most 513 - 170 = 343 subject-only columns, two per query residue.
// (The band of 150 bp reads reaches column 53 at most on real genomes, mc_core.h.)  An alignment beyond that is cut at a segment's edge,
// scores less there, and is an edge row: edge_rows counts it, and a run with edge_rows == 0 has met none.
#pragma once
#include "mc_core.h"

#define MC_FOLD_SEG_LEN 1192                                             // L
#define MC_FOLD_OVERLAP 512                                          // V
#define MC_FOLD_MAX_GENE 65535
#define MC_FOLD_MAX_SEGS 32767
static_assert(MC_FOLD_SEG_LEN <= 2047, "a segment is a sequence of the index: 11 bits of position in the posting word (MC_POST8)");
static_assert(MC_FOLD_OVERLAP == (3 * MC_MAXAA + 63) / 64 * 64 && MC_FOLD_OVERLAP + 1 >= 3 * MC_MAXAA, "V: the longest read's bases rounded up to a multiple of 64 - two subject-only columns per query residue");
static_assert(MC_FOLD_OVERLAP < MC_FOLD_SEG_LEN, "the step S = L - V is positive");
static_assert(MC_GAP_OPEN == 11 && MC_GAP_EXT == 1, "the derivation of what the gapped stage can insert reads these costs");

// the record of one segment on the device: its gene, its offset in the gene, and the two coordinates at which a row touches an interior
// edge: lo = 0 on a segment that is not its gene's first, hi = its last residue on one that is not its gene's last; -1: no such edge
struct McFoldSeg { int32_t gene, off, lo, hi; };

MC_HD int mc_fold_step(int L, int V) { return L - V; }
MC_HD int mc_fold_nsegs(int len, int L, int V) { return len <= L ? 1 : 1 + (len - L + (L - V) - 1) / (L - V); }
MC_HD int mc_fold_seg_off(int j, int L, int V) { return j * (L - V); }
MC_HD int mc_fold_seg_len(int len, int j, int L, int V) { const int rest = len - j * (L - V); return rest < L ? rest : L; }
// the segment that holds every span of at most V + 1 residues that starts at residue a of a gene of len residues
MC_HD int mc_fold_seg_of(int a, int len, int L, int V) { const int j = a / (L - V), n = mc_fold_nsegs(len, L, V); return j < n - 1 ? j : n - 1; }
// segment j of a gene of len residues cut with (L, V): gene g
MC_HD McFoldSeg mc_fold_seg(int g, int len, int j, int L, int V)
{
    McFoldSeg s; s.gene = g; s.off = mc_fold_seg_off(j, L, V);
    s.lo = j > 0 ? 0 : -1;
    s.hi = j < mc_fold_nsegs(len, L, V) - 1 ? mc_fold_seg_len(len, j, L, V) - 1 : -1;
    return s;
}

MC_HD bool mc_fold_edge(const McRow &r, int32_t nseq, const McFoldSeg *seg)
{
    if (r.subject < 0 || r.subject >= nseq) return false;
    const McFoldSeg s = seg[r.subject];
    return (s.lo >= 0 && r.sstart == s.lo) || (s.hi >= 0 && r.send == s.hi);
}
MC_HD McRow mc_fold_row(McRow r, int32_t nseq, const McFoldSeg *seg)
{
    if (r.subject < 0 || r.subject >= nseq) return r;
    const McFoldSeg s = seg[r.subject];
    r.subject = s.gene; r.sstart += s.off; r.send += s.off;
    return r;
}
