// mc_depthstats.h - order statistics of a gene's per-residue depth (mc_depth_stats): the lower median, and the sum of the central P percent
// of the sorted depths - the "truncated average depth", TAD80 at P = 80.  Host and device code alike: k_depthstats.h runs it,
// tests/emul/depthstats.cpp compiles it with g++, and tests/depthstats_restated.py restates it.  No HIP include here.
//
// ---- THE STATEMENT ---------------------------------------------------------------------------------------------------------------
// For gene s of len residues, d[0 .. len - 1] is the depth of k_coverage.h: the wrapping 32-bit prefix sums of the gene's slots of the
// difference array (of the depth, or with ties of the any-depth).  x[0] <= ... <= x[len - 1] are those depths sorted, zeros included.
// P is the percent kept, an integer in 1 .. 100.
//     cut = len * (100 - P) / 200         integer division: the ranks left out at EITHER end
//     lo = cut          hi = len - cut
//     median      = x[(len - 1) / 2]                      the LOWER median, as ident_median is (mc_identity.h)
//     low         = x[lo]          high = x[hi - 1]       the kept ranks' ends
//     trimmed_sum = the sum of x[i] for lo <= i < hi      64-bit: at most 65,535 values below 2^32, exact
// The truncated average depth is trimmed_sum / (hi - lo), made on the host in float64 (abundance.py).
// A gene without reads (tab[2 s] == 0: its slots are all zero) has four zeros and is not walked.
// All four are exact integers and do not depend on batches, ranges, launch geometry or the order of any atomics.
//
// hi - lo >= 1 for every len >= 1: 200 * cut <= len * (100 - P) <= 99 * len, so 2 * cut <= 0.99 * len < len and hi - lo = len - 2 * cut > 0.
// lo <= (len - 1) / 2 <= hi - 1 always: 2 * cut < len gives 2 * cut <= len - 1, so the integer cut is at most floor((len - 1) / 2); and
// hi - 1 = len - 1 - cut >= len - 1 - floor((len - 1) / 2) = ceil((len - 1) / 2).
// Invariants (tests/depthstats_restated.py: invariants):
//     P == 100:  cut == 0 and trimmed_sum == spanned of mc_coverage_read
//     low <= median <= high   for every P (the line above)
//     high <= max_depth       trimmed_sum <= spanned
// A pile of reads on one short domain moves neither the median nor, while the domain is shorter than cut residues, the trimmed sum; a gene
// covered over less than half of its length has a median of 0.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_DS_HD __host__ __device__ inline
#else
#define MC_DS_HD inline
#endif

#define MC_DS_NOUT 4                             // the values k_depth_select writes per gene: median, trimmed_sum, low, high
#define MC_DS_MEDIAN 0
#define MC_DS_SUM 1
#define MC_DS_LOW 2
#define MC_DS_HIGH 3

static inline size_t mc_ds_out_slots(size_t nseq) { return (size_t)MC_DS_NOUT * nseq; }

MC_DS_HD bool mc_ds_keep_ok(long long P) { return P >= 1 && P <= 100; }
// the ranks left out at either end (len up to 65,535: 32 bits hold the product)
MC_DS_HD uint32_t mc_ds_cut(uint32_t len, int32_t P) { return len * (uint32_t)(100 - P) / 200u; }
MC_DS_HD uint32_t mc_ds_lo(uint32_t len, int32_t P) { return mc_ds_cut(len, P); }
MC_DS_HD uint32_t mc_ds_hi(uint32_t len, int32_t P) { return len - mc_ds_cut(len, P); }
MC_DS_HD uint32_t mc_ds_median_rank(uint32_t len) { return (len - 1u) / 2u; }

// ---- the boundary arithmetic of a SELECTION: the sum over the ranks lo .. hi - 1 without sorting, from low = x[lo], high = x[hi - 1] and four
// exact counts over the gene's depths: n_lt_low and n_le_low, the depths below and at or below `low`; n_lt_high, those below `high`; between,
// the sum of the depths strictly between the two.  The depths equal to `low` hold the ranks n_lt_low .. n_le_low - 1, of which lo .. min(n_le_low,
// hi) - 1 are kept (n_lt_low <= lo < n_le_low: that is what x[lo] == low says - n_lt_low enters nowhere else); those equal to `high` hold the
// ranks from n_lt_high, of which max(n_lt_high, lo) .. hi - 1 are kept; every depth strictly between lies at a kept rank.
MC_DS_HD unsigned long long mc_ds_trimmed_sum(uint32_t low, uint32_t high, uint32_t lo, uint32_t hi, uint32_t n_lt_low, uint32_t n_le_low, uint32_t n_lt_high,
                                              unsigned long long between)
{
    (void)n_lt_low;
    if (low == high) return (unsigned long long)low * (hi - lo);
    const uint32_t top = n_le_low < hi ? n_le_low : hi, from = n_lt_high > lo ? n_lt_high : lo;
    return (unsigned long long)low * (top - lo) + between + (unsigned long long)high * (hi - from);
}
