// k_depthstats.h - the lower median and the truncated average depth of every gene on the device (mc_depth_stats): order statistics of the
// depths k_coverage.h keeps as a difference array, by a radix SELECTION - nothing is sorted, and no residue's depth leaves the device.
// mc_depthstats.h states the rule and holds the boundary arithmetic.
#pragma once
#include "k_coverage.h"
#include "mc_depthstats.h"

#ifndef MC_DS_LDS_LEN
#define MC_DS_LDS_LEN 4096                       // the residues of a gene whose depths are kept in LDS (16 KB): every unfolded gene (2,047 at most)
#endif
#define MC_DS_THREADS 256
#define MC_DS_RANKS 3                            // the ranks selected at once: (len - 1) / 2, lo and hi - 1

// what one workgroup keeps in LDS: the depths of a gene of up to MC_DS_LDS_LEN residues, one 256-bin histogram per rank, and per rank what the
// passes so far have fixed - the value's high digits, the depths below them, and (after a pass) the depths in the chosen bin
struct McDsShared {
    uint32_t dep[MC_DS_LDS_LEN];
    uint32_t hist[MC_DS_RANKS][256];
    uint32_t wsum[2][4];                         // the four waves' totals of a chunk of the scan, double-buffered: one barrier per chunk
    uint32_t wmax[4];
    unsigned long long wbetween[4];
    uint32_t prefix[MC_DS_RANKS], below[MC_DS_RANKS], equal[MC_DS_RANKS];
};

// f(p, d) for every residue p of the gene with its depth d, by all MC_DS_THREADS threads of the workgroup (every thread calls this).
// LDS: the depths are in sh.dep (a gene of up to MC_DS_LDS_LEN residues, behind the first walk).  Otherwise the difference array is scanned
// again: chunks of 256 slots, a wave scan (k_coverage.h) per wave, the waves' totals and the carry of the chunks before through LDS.
template <bool LDS, class F> __device__ __forceinline__ void mc_ds_walk(McDsShared &sh, const uint32_t *__restrict__ slots, uint32_t len, F f)
{
    const uint32_t tid = threadIdx.x;
    if (LDS) {
        for (uint32_t p = tid; p < len; p += MC_DS_THREADS) f(p, sh.dep[p]);
        return;
    }
    const int lane = mc_lane();
    const uint32_t w = tid >> 6;
    uint32_t carry = 0, buf = 0;
    for (uint32_t base = 0; base < len; base += MC_DS_THREADS, buf ^= 1u) {          // (uniform: every thread takes every chunk and its barrier)
        const uint32_t p = base + tid;
        uint32_t d = mc_wave_scan_u32(p < len ? slots[p] : 0u, lane);
        if (lane == 63) sh.wsum[buf][w] = d;
        __syncthreads();
        const uint32_t t0 = sh.wsum[buf][0], t1 = sh.wsum[buf][1], t2 = sh.wsum[buf][2], t3 = sh.wsum[buf][3];
        d += carry + (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
        carry += t0 + t1 + t2 + t3;
        if (p < len) f(p, d);
    }
}

// One pass of the selection at digit `shift` (24, 16, 8 or 0), 8 bits: every depth that agrees with rank k's value in the digits above adds 1 to
// bin (d >> shift) & 255 of k's histogram; then wave k finds the bin that holds rank k - lane l sums bins 4 l .. 4 l + 3, a wave scan gives the
// cumulative counts, a ballot the lane, that lane the bin - and fixes the digit: prefix |= bin << shift, below += the depths in the lower bins.
template <bool LDS> __device__ __forceinline__ void mc_ds_pass(McDsShared &sh, const uint32_t *__restrict__ slots, uint32_t len, int shift, const uint32_t (&rank)[MC_DS_RANKS])
{
    const uint32_t tid = threadIdx.x;
    for (int k = 0; k < MC_DS_RANKS; k++) sh.hist[k][tid] = 0u;
    __syncthreads();
    const uint32_t p0 = sh.prefix[0], p1 = sh.prefix[1], p2 = sh.prefix[2];
    mc_ds_walk<LDS>(sh, slots, len, [&](uint32_t, uint32_t d) {
        const uint32_t bin = (d >> shift) & 255u;                               // (the digits above `shift + 8`: two shifts, each below 32)
        if ((((d ^ p0) >> shift) >> 8) == 0u) atomicAdd(&sh.hist[0][bin], 1u);
        if ((((d ^ p1) >> shift) >> 8) == 0u) atomicAdd(&sh.hist[1][bin], 1u);
        if ((((d ^ p2) >> shift) >> 8) == 0u) atomicAdd(&sh.hist[2][bin], 1u);
    });
    __syncthreads();
    const uint32_t k = tid >> 6;
    if (k < MC_DS_RANKS) {                                                      // (wave-uniform)
        const int lane = mc_lane();
        const uint32_t c0 = sh.hist[k][4 * lane], c1 = sh.hist[k][4 * lane + 1], c2 = sh.hist[k][4 * lane + 2], c3 = sh.hist[k][4 * lane + 3];
        const uint32_t t = c0 + c1 + c2 + c3, incl = mc_wave_scan_u32(t, lane);
        const uint32_t rk = k == 0 ? rank[0] : k == 1 ? rank[1] : rank[2];
        const uint32_t need = rk - sh.below[k];                                 // the rank among the depths that agree so far: below their number
        const unsigned long long reach = __ballot(incl > need);
        if (reach && lane == __builtin_ctzll(reach)) {
            uint32_t rem = need - (incl - t), j = 0, cj = c0;
            if (rem >= cj) { rem -= cj; j = 1; cj = c1; }
            if (j == 1 && rem >= cj) { rem -= cj; j = 2; cj = c2; }
            if (j == 2 && rem >= cj) { rem -= cj; j = 3; cj = c3; }
            sh.prefix[k] |= (4u * (uint32_t)lane + j) << shift;
            sh.below[k] = rk - rem;
            sh.equal[k] = cj;
        }
    }
    __syncthreads();
}

template <bool LDS> __device__ __forceinline__ void mc_ds_gene(McDsShared &sh, const uint32_t *__restrict__ slots, uint32_t len, int32_t P, unsigned long long *o)
{
    const uint32_t tid = threadIdx.x;
    const int lane = mc_lane();
    // 1. the depths (into LDS where they fit) and their maximum
    uint32_t mx = 0;
    mc_ds_walk<false>(sh, slots, len, [&](uint32_t p, uint32_t d) { if (LDS) sh.dep[p] = d; mx = max(mx, d); });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    if (lane == 0) sh.wmax[tid >> 6] = mx;
    if (tid < MC_DS_RANKS) { sh.prefix[tid] = 0u; sh.below[tid] = 0u; sh.equal[tid] = len; }
    __syncthreads();
    mx = max(max(sh.wmax[0], sh.wmax[1]), max(sh.wmax[2], sh.wmax[3]));
    if (mx == 0u) {                                                             // (reads whose spans marked nothing: every depth is zero)
        if (tid < MC_DS_NOUT) o[tid] = 0ull;
        return;
    }
    // 2. the three ranks at once, most significant digit first; the digits above the maximum's highest set bit are zero in every depth
    const uint32_t lo = mc_ds_lo(len, P), hi = mc_ds_hi(len, P);
    const uint32_t rank[MC_DS_RANKS] = {mc_ds_median_rank(len), lo, hi - 1u};
    for (int shift = (31 - __clz(mx)) / 8 * 8; shift >= 0; shift -= 8) mc_ds_pass<LDS>(sh, slots, len, shift, rank);
    const uint32_t low = sh.prefix[1], high = sh.prefix[2];
    // 3. the sum of the depths strictly between low and high (none when they are equal or neighbours)
    unsigned long long between = 0;
    if (high > low + 1u) {                                                      // (uniform)
        mc_ds_walk<LDS>(sh, slots, len, [&](uint32_t, uint32_t d) { if (d > low && d < high) between += d; });
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) between += __shfl_xor(between, d, 64);
        if (lane == 0) sh.wbetween[tid >> 6] = between;
        __syncthreads();
        between = sh.wbetween[0] + sh.wbetween[1] + sh.wbetween[2] + sh.wbetween[3];
    }
    if (tid == 0) {
        o[MC_DS_MEDIAN] = sh.prefix[0];
        o[MC_DS_SUM] = mc_ds_trimmed_sum(low, high, lo, hi, sh.below[1], sh.below[1] + sh.equal[1], sh.below[2], between);
        o[MC_DS_LOW] = low;
        o[MC_DS_HIGH] = high;
    }
}

// The read: ONE WORKGROUP PER GENE.  It first reads tab[2 s] like k_coverage_scan - the gene's reads in the count table, or its candidates in the
// head of the tie table for the any-depth: a gene without any (on real data nearly all of them) writes four zeros and leaves.  Otherwise
//   1. a block-wide scan of the gene's slots gives the depths and their maximum;
//   2. a radix selection, most significant digit first, 8 bits a pass, finds the ranks (len - 1) / 2, lo and hi - 1 at once - the passes above
//      the maximum's highest set bit are skipped: a gene no deeper than 255 takes one pass;
//   3. one last walk sums the depths strictly between x[lo] and x[hi - 1]; the counts of mc_ds_trimmed_sum are what the selection ended with.
// The depths of a gene of up to MC_DS_LDS_LEN residues stay in LDS between the walks; a longer gene (gene space under a fold, up to 65,535) scans
// its slots again in every walk: no global scratch, nothing to allocate.  The result is the same whatever the path and the block's shape.
// out: MC_DS_NOUT values per gene from out[MC_DS_NOUT * s]: median, trimmed_sum, low, high.  diff is only read: ranges may go on marking after a
// read.  The only atomics are the histograms' in LDS.
__global__ void __launch_bounds__(MC_DS_THREADS) k_depth_select(const unsigned long long *__restrict__ tab, const uint32_t *__restrict__ off, const uint32_t *__restrict__ diff,
                                                                int32_t nseq, int32_t P, unsigned long long *out)
{
    __shared__ McDsShared sh;
    const int32_t s = (int32_t)blockIdx.x;
    if (s >= nseq) return;                                                      // (uniform)
    unsigned long long *o = out + (size_t)MC_DS_NOUT * (size_t)s;
    if (tab[2 * (size_t)s] == 0) {
        if (threadIdx.x < MC_DS_NOUT) o[threadIdx.x] = 0ull;
        return;
    }
    const uint32_t r0 = off[s], len = off[s + 1] - r0;
    const uint32_t *slots = diff + r0 + (uint32_t)s;                            // (the gene's first slot: k_coverage.h, "Layout")
    if (len <= MC_DS_LDS_LEN) mc_ds_gene<true>(sh, slots, len, P, o);
    else mc_ds_gene<false>(sh, slots, len, P, o);
}
