// mc_identity.h - the alignment identity of the reads assigned to a gene (mc_set_identity): the bin of one best row, the layout of the
// per-gene tables, and the figures read off one gene's histogram.  Host and device code alike: k_identity.h runs it, mc_abund.h sizes
// its buffers by it, tests/emul/identity.cpp compiles it with g++, and tests/identity_restated.py restates it.  No HIP include here.
//
// ---- THE STATEMENT ---------------------------------------------------------------------------------------------------------------
// Which row counts: a read's best row is exactly the one k_abundance.h defines - the same four cut-offs, the highest bits, the first
// on a tie - and it counts under the same condition, 0 <= subject < nseq.  For that row (nmatch: the identical columns, mc_row.nmatch):
//     bin = alnlen < 1 ? 0 : (100 * nmatch) / alnlen          integer division: the floor of the identity in percent, 0 .. 100
//     hist[subject][bin] += 1          matched[subject] += nmatch          mismatched[subject] += mismatch          gap_opens[subject] += gapopen
// (Every row of the engine has 0 <= nmatch <= alnlen; of any other row the bin is the nearest of 0 and 100 - nothing is written outside a
// gene's bins - and the sums take the row's values as they are.)
// hist is 32-bit, MC_ID_BINS counters per gene; the three sums are 64-bit, one record per gene.  All counters are integers: the result is
// exact and does not depend on launch geometry, batches, ranges, classes or the order of the atomics.
// Per gene, with n = the sum of its bins (= reads[subject] of k_abundance.h):
//     ident_min, ident_max   the lowest and the highest non-empty bin
//     ident_median           the LOWER median: the smallest bin b whose cumulative count hist[0] + .. + hist[b] reaches (n - 1) / 2 + 1
//     ge[j]                  the reads in bins >= level[j]; up to MC_ID_LEVELS levels, integers in 0 .. 100, strictly ascending
// A gene with n == 0 has no min, median or max - MC_ID_NONE stands for them - and its ge are 0.
// Width: a bin counts to 2^32 - 1; a gene with 2^32 or more reads wraps n, and with it the median and ge.
//
// ---- Layout ----------------------------------------------------------------------------------------------------------------------
// hist: gene s owns MC_ID_STRIDE = 128 counters from MC_ID_STRIDE * s: bins 0 .. 100 and 27 that stay zero - 512 bytes, four lines of 128,
// so that a wave of k_identity_scan takes a gene as two aligned words per lane (lane l: bins l and 64 + l) without a bounds test.
// sums: one McIdSums per gene, 32 bytes and aligned to them: the three atomics of a read go to ONE line.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_ID_HD __host__ __device__ inline
#else
#define MC_ID_HD inline
#endif

#define MC_ID_BINS 101
#define MC_ID_LEVELS 8
#define MC_ID_STRIDE 128
#define MC_ID_NONE (-1)
#define MC_ID_NOUT (3 + MC_ID_LEVELS)            // the most values k_identity_scan writes per gene: min, median, max, ge[0 .. nlevels - 1]

struct alignas(32) McIdSums { unsigned long long matched, mismatched, gap_opens, unused; };

static inline size_t mc_id_hist_slots(size_t nseq) { return (size_t)MC_ID_STRIDE * nseq; }
static inline size_t mc_id_hist_at(size_t s, int bin) { return (size_t)MC_ID_STRIDE * s + (size_t)bin; }
static inline size_t mc_id_out_slots(size_t nseq) { return (size_t)MC_ID_NOUT * nseq; }

MC_ID_HD int mc_id_bin(int nmatch, int alnlen)
{
    if (alnlen < 1 || nmatch < 0) return 0;
    return nmatch >= alnlen ? 100 : (100 * nmatch) / alnlen;
}

// ---- the figures of ONE histogram of MC_ID_BINS counters, written once: the scan kernel computes the same values a wave at a time, and
// tests/test_gpu_identity_units.py holds it to these through tests/identity_restated.py
MC_ID_HD unsigned long long mc_id_total(const uint32_t *h)
{
    unsigned long long n = 0;
    for (int b = 0; b < MC_ID_BINS; b++) n += h[b];
    return n;
}
MC_ID_HD int mc_id_min(const uint32_t *h)
{
    for (int b = 0; b < MC_ID_BINS; b++) if (h[b]) return b;
    return MC_ID_NONE;
}
MC_ID_HD int mc_id_max(const uint32_t *h)
{
    for (int b = MC_ID_BINS - 1; b >= 0; b--) if (h[b]) return b;
    return MC_ID_NONE;
}
MC_ID_HD int mc_id_median(const uint32_t *h)
{
    const unsigned long long n = mc_id_total(h);
    if (n == 0) return MC_ID_NONE;
    const unsigned long long need = (n - 1) / 2 + 1;
    unsigned long long cum = 0;
    for (int b = 0; b < MC_ID_BINS; b++) { cum += h[b]; if (cum >= need) return b; }
    return MC_ID_NONE;                                             // (not reached: cum == n >= need at the last bin)
}
MC_ID_HD unsigned long long mc_id_ge(const uint32_t *h, int level)
{
    unsigned long long n = 0;
    for (int b = level < 0 ? 0 : level; b < MC_ID_BINS; b++) n += h[b];
    return n;
}
// the index of the first level that is out of 0 .. 100 or not above the one before it; -1: all n are good (n itself is the caller's to check)
MC_ID_HD int mc_id_bad_level(const int32_t *level, int n)
{
    for (int j = 0; j < n; j++)
        if (level[j] < 0 || level[j] > 100 || (j && level[j] <= level[j - 1])) return j;
    return -1;
}
