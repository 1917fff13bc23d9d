// k_groupboot.h - the bootstrap of the groups table behind the gene bootstrap's (mc_group_bootstrap): a group's replicate values are
// sums of its members' replicate RPKGs, whose errors are correlated, so its error bar is made from the members' replicate counts and
// not from their error bars.  mc_groupboot.h states the rule; the two kernels below follow it on `mat`, the genes-with-reads x B
// replicate counts k_geneboot_sums left on the device (k_geneboot.h).  No replicate count reaches the host.
#pragma once
#include "k_geneboot.h"
#include "mc_groupboot.h"

// The shape of k_geneboot_sums: a 2-D grid of groups with reads x replicate tiles of MC_GB_LANES, one wave per block, a lane per
// replicate.  The wave walks the group's members - start[G] .. start[G + 1] of `member`, the compact indices of the genes with reads in
// ascending gene index, kb their gene_kb (mc_grb_plan) - in that order: the addition order is part of the rule, so the walk is serial per
// lane.  The member and its kb are the same for the whole wave (a uniform address: scalar loads), and the next member's load flies under
// this member's arithmetic; the 64 lanes read 512 consecutive bytes of mat[g][.].  A lane keeps y and C in registers and writes
// val[G][b] and, with cnt not null, cnt[G][b]: plain stores, no atomics.  A lane with b >= B reads replicate B - 1 and writes nothing; a
// member not below ngenes (the plan has none) adds nothing.
__global__ void __launch_bounds__(MC_GB_LANES) k_groupboot_values(const unsigned long long *__restrict__ mat, uint32_t ngenes, int32_t B, const double *__restrict__ scale,
                                                                  const uint32_t *__restrict__ start, const uint32_t *__restrict__ member, const double *__restrict__ kb,
                                                                  double *val, unsigned long long *cnt)
{
    const int lane = (int)threadIdx.x;
    const long long b = (long long)blockIdx.y * MC_GB_LANES + lane;
    const size_t bb = (size_t)(b < B ? b : B - 1);
    const uint32_t lo = start[blockIdx.x], hi = start[blockIdx.x + 1];
    const double s = scale[bb];
    const bool use = mc_gb_used(s);
    double y = 0.0;
    unsigned long long C = 0ull;
    uint32_t gnext = lo < hi ? member[lo] : 0u;
    double knext = lo < hi ? kb[lo] : 1.0;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t g = gnext;
        const double k = knext;
        const uint32_t j = i + 1 < hi ? i + 1 : i;
        gnext = member[j]; knext = kb[j];
        if (g >= ngenes) continue;
        const unsigned long long c = mat[(size_t)g * (size_t)B + bb];
        C += c;
        if (use) y = mc_grb_add(y, c, s, k);
    }
    if (b >= B) return;
    const size_t at = (size_t)blockIdx.x * (size_t)B + bb;
    val[at] = y;
    if (cnt) cnt[at] = C;
}

// k_geneboot_summary on a row of val: one workgroup of MC_GB_THREADS per group with reads.  The used values go to LDS, an unused
// replicate as +inf, padded with +inf to the next power of two P; sum and m2 are added in the stated order (mc_grb_thread_sum, then the
// halving tree level by level with a barrier between the levels); a bitonic network sorts the P values ascending - the m used ones come
// first - and thread 0 writes the six doubles to out[6 G ..].  m: the number of used replicates, counted by the caller with mc_gb_used.
// The LDS is k_geneboot_summary's: MC_GB_MAXB + MC_GB_THREADS doubles.
__global__ void __launch_bounds__(MC_GB_THREADS) k_groupboot_summary(const double *__restrict__ val, const double *__restrict__ scale, int32_t B, int32_t m, double *out)
{
    __shared__ double x[MC_GB_MAXB];
    __shared__ double part[MC_GB_THREADS];
    const int t = (int)threadIdx.x;
    const double *y = val + (size_t)blockIdx.x * (size_t)B;
    double *o = out + (size_t)MC_GB_NOUT * blockIdx.x;
    if (m <= 0) { if (t < MC_GB_NOUT) o[t] = mc_gb_nan(); return; }
    int P = 1;
    while (P < B) P <<= 1;
    for (int b = t; b < P; b += MC_GB_THREADS) x[b] = b < B && mc_gb_used(scale[b]) ? y[b] : __builtin_inf();
    part[t] = mc_grb_thread_sum(y, scale, B, t, 0.0, false);
    __syncthreads();
    for (int h = MC_GB_THREADS / 2; h >= 1; h >>= 1) { if (t < h) part[t] += part[t + h]; __syncthreads(); }
    const double sum = part[0];
    __syncthreads();
    part[t] = mc_grb_thread_sum(y, scale, B, t, sum / (double)m, true);
    __syncthreads();
    for (int h = MC_GB_THREADS / 2; h >= 1; h >>= 1) { if (t < h) part[t] += part[t + h]; __syncthreads(); }
    const double m2 = part[0];
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += MC_GB_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const double a = x[i], z = x[l];
                    if ((i & k) == 0 ? a > z : a < z) { x[i] = z; x[l] = a; }
                }
            }
            __syncthreads();
        }
    if (t == 0) {
        o[MC_GB_SUM] = sum; o[MC_GB_M2] = m2;
        for (int k = MC_GB_LO; k <= MC_GB_HI1; k++) o[k] = x[mc_gb_index(m, k)];
    }
}
