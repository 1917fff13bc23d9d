// mc_covboot.h - the bootstrap of the coverage columns (mc_set_coverage_bootstrap, mc_coverage_bootstrap): how much a gene's breadth, and
// its detection call, hang on single reads.  It extends mc_geneboot.h from the count of a gene's reads to the residues those reads cover.
// Same conventions as mc_geneboot.h and mc_tieboot.h: host and device code alike, no HIP include of its own - k_covboot.h runs it on the
// device, g++ compiles the very same text into tests/emul/covboot.cpp, and tests/covboot_restated.py restates it in numpy.
//
// ---- THE STATEMENT ----------------------------------------------------------------------------------------------------------------
// ENTRY.  Every assigned read is k_abundance.h's best row: the same four cut-offs, the highest bits, the first row on a tie; its subject
// must lie in 0 .. nseq - 1.  It leaves ONE entry (q, gene, s, e), 12 bytes: q the read's global id, 0 <= q < 2^31 - mc_row.query, and in a
// class run base + perm[query] (mc_cb_id; k_geneboot.h's McIdMap); s / e the best row's sstart / send, 0-based and inclusive, in gene space
// (behind k_fold under a gene fold: at most 65,534, 16 bits each).  A span that k_abundance_cov's guard keeps out of the depth (sstart < 0,
// sstart > send, send >= len) is stored as THE EMPTY SPAN s = 1, e = 0: the read still has its entry - the list's cursor always equals the
// count table's `assigned`, and the slices of the grouped list are the count table's `reads` - and it covers nothing.
// REPLICATE COVERAGE.  Read q is PRESENT in replicate b when mc_boot_weight(mc_boot_key(seed, b), q) > 0, which is the one comparison
// mc_mix64(key + q) >= MC_BOOT_THR[0] (mc_cb_present).  cov[b][g], b in 0 .. B - 1, 1 <= B <= MC_GB_MAXB, is the number of residues p of
// gene g with s <= p <= e for at least one present entry of g: an exact integer that does not depend on ranges, batches, launch geometry,
// the window below or the order of anything.  Replicate b under one seed is the same resample of the same reads as replicate b of
// mc_bootstrap and of mc_gene_bootstrap.
// SUMMARY.  The six doubles of mc_gb_gene on the values (double)cov[b][g] with every replicate used: scale 1.0 for all b, m = B, in
// mc_geneboot.h's addition order - device, g++ and numpy agree bit for bit.  A gene without reads gives zeros.  The figures are in
// residues; the host divides by the gene's length.
// DETECTION.  det[g] is the number of b with cov[b][g] >= need[g].  The caller passes need[g] = max(1, ceil(F x length)) computed in
// float64: for an integer c, c >= F x length holds exactly when c >= ceil(F x length), and need >= 1 makes "the replicate has a read of
// the gene" implied.  need[g] == 0 is refused: every replicate would detect every gene.
// INVARIANTS, all under one seed.  cov[b][g] <= covered[g] of k_coverage_scan (a replicate's present reads are some of the sample's).
// cov[b][g] > 0 implies c[b][g] > 0 of mc_gene_bootstrap; the converse holds for a gene all of whose spans are valid.  A gene with one
// read has cov[b] in {0, e - s + 1}.
// THE WINDOW.  The device keeps one 64-bit word per residue, bit b = replicate b of the tile covers it, for MC_CB_WINDOW residues at a
// time; a longer gene is covered window by window, every pass clipping the spans to its window (mc_cb_clip), and cov is the sum over the
// windows.  The serial form below (mc_cb_cover) walks the same windows with the same clip, so g++ runs that text too.
#pragma once
#include <cstddef>
#include "mc_geneboot.h"

#define MC_CB_WINDOW 2048                                           // residues per window: 16 KiB of LDS, and every gene of an unfolded database in one pass
#define MC_CB_MAXCAP 2147483647                                     // 2^31 - 1 entries: no more reads have an id

// an entry of the device list: one assigned read and the span of its best row.  In the collected list `gene` is the subject; in the
// grouped list the compact index of the gene among those with reads
struct McCbEntry { uint32_t q, gene; uint16_t s, e; };
static_assert(sizeof(McCbEntry) == 12, "an entry is 12 bytes");
// a gene with reads, as the cover kernel takes it: its slice of the grouped list, its residues and (0: no detection asked for) its need
struct McCbGene { uint32_t begin, n, len, need; };

// the global id of the read whose rows carry `query`: perm null: the id itself; else base + perm[query], below 2^31 (mc_search_classes)
MC_HD uint32_t mc_cb_id(const uint32_t *perm, int64_t base, int32_t query) { return perm ? (uint32_t)(base + (int64_t)perm[query]) : (uint32_t)query; }
// the entry of a read assigned to `gene` of len residues whose best row spans bs .. be: k_abundance_cov's guard, or the empty span
MC_HD McCbEntry mc_cb_entry(uint32_t q, int32_t gene, int32_t bs, int32_t be, uint32_t len)
{
    McCbEntry e; e.q = q; e.gene = (uint32_t)gene;
    const bool in = bs >= 0 && bs <= be && (uint32_t)be < len;        // (len <= 65,535, mc_fold.h: both ends fit 16 bits)
    e.s = in ? (uint16_t)bs : (uint16_t)1; e.e = in ? (uint16_t)be : (uint16_t)0;
    return e;
}
MC_HD bool mc_cb_present(uint64_t key, uint32_t q) { return mc_mix64(key + (uint64_t)q) >= MC_BOOT_THR[0]; }
// the part of an entry's span inside the window of wn residues from w0, as offsets a .. z into the window; false: none (the empty span too)
MC_HD bool mc_cb_clip(const McCbEntry &e, uint32_t w0, uint32_t wn, uint32_t *a, uint32_t *z)
{
    const uint32_t s = e.s, t = e.e;
    if (s > t || t < w0 || s >= w0 + wn) return false;
    *a = s > w0 ? s - w0 : 0u;
    *z = t < w0 + wn ? t - w0 : wn - 1u;
    return true;
}

// What ONE thread does for the read at row i, the read's first (k_covboot_collect; the emulation): k_abundance_cov's walk with the span
// kept.  passes: a row's four cut-offs; len_of(s): the residues of gene s.  Returns whether the read is assigned, and then its entry.
template <class Pass, class Len>
MC_HD bool mc_cb_read(const Pass &passes, const Len &len_of, const McRow *rows, uint32_t nrows, uint32_t i, int32_t nseq, uint32_t q, McCbEntry *out)
{
    const int query = rows[i].query;
    double bbits = 0.0; int bsub = -1, bs = 0, be = 0;
    for (uint32_t k = i; k < nrows && rows[k].query == query; k++) {
        const McRow r = rows[k];
        if (!passes(r)) continue;
        if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; bs = r.sstart; be = r.send; }
    }
    if (bsub < 0 || bsub >= nseq) return false;
    *out = mc_cb_entry(q, bsub, bs, be, len_of(bsub));
    return true;
}

// The replicate coverage of ONE gene and ONE replicate in serial form (k_covboot_cover does the same for 64 replicates at once: a bit
// each in a window's words).  e: the gene's n entries; mark: MC_CB_WINDOW bytes of scratch.
MC_HD uint32_t mc_cb_cover(const McCbEntry *e, size_t n, uint32_t len, uint64_t key, uint8_t *mark)
{
    uint32_t cov = 0;
    for (uint32_t w0 = 0; w0 < len; w0 += MC_CB_WINDOW) {
        const uint32_t wn = len - w0 < MC_CB_WINDOW ? len - w0 : MC_CB_WINDOW;
        for (uint32_t p = 0; p < wn; p++) mark[p] = 0;
        for (size_t i = 0; i < n; i++) {
            uint32_t a, z;
            if (!mc_cb_present(key, e[i].q) || !mc_cb_clip(e[i], w0, wn, &a, &z)) continue;
            for (uint32_t p = a; p <= z; p++) mark[p] = 1;
        }
        for (uint32_t p = 0; p < wn; p++) cov += mark[p];
    }
    return cov;
}
