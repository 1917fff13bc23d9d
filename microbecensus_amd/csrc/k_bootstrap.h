// k_bootstrap.h - the Poisson bootstrap of the per-family sums (mc_bootstrap): B replicates x every best hit, weights as mc_boot.h
// states them.
#pragma once
#include "mc_hip_common.h"
#include "mc_boot.h"

// A 2-D grid of hit tiles x replicate tiles, one wave per block.  A lane owns one replicate (its key in registers) and walks the
// tile's hits; the hit is the same for the whole wave (a uniform address: scalar loads), only u = mix(key + read) differs.  The
// sums live in the block's LDS as [family][lane] 8-byte words - the 64 lanes of an update touch 64 consecutive words, no bank
// conflict, and the wave is the array's only user, so plain read-modify-write does (no atomics, no barrier).  One word per family:
// aln_stat says whether it is an int64 (hits, aln) or a double (cov).  Row nfam holds W[b], the replicate's classified reads.
// Each block writes its partial sums to part[tile][row][b]; k_bootstrap_reduce adds the tiles in ascending order, so the integer
// sums are exact whatever the tiling and the cov sums are the same on every run with the same (n, B).
#define MC_BOOT_LANES 64
struct McBootPars { int32_t nfam, B; uint64_t stats, seed; };     // stats: two bits per family, its aln_stat
__host__ __device__ inline int mc_boot_stat(const McBootPars &P, int f) { return (int)((P.stats >> (2 * f)) & 3ull); }

__global__ void __launch_bounds__(MC_BOOT_LANES) k_bootstrap(McBootPars P, const mc_best_hit *__restrict__ hits, int64_t n, int64_t per_tile, unsigned long long *__restrict__ part)
{
    __shared__ unsigned long long acc[33 * MC_BOOT_LANES];
    const int lane = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.y * MC_BOOT_LANES + lane;
    for (int f = 0; f < P.nfam; f++) acc[f * MC_BOOT_LANES + lane] = 0ull;
    const uint64_t key = mc_boot_key(P.seed, (uint64_t)b);
    const int64_t lo = (int64_t)blockIdx.x * per_tile, hi = lo + per_tile < n ? lo + per_tile : n;
    unsigned long long wsum = 0ull;
    mc_best_hit next = hits[lo < n ? lo : 0];
    for (int64_t i = lo; i < hi; i++) {
        const mc_best_hit h = next;
        next = hits[i + 1 < hi ? i + 1 : i];                        // the next hit's scalar load flies under this hit's mixing
        const int w = mc_boot_weight(key, (uint64_t)(uint32_t)h.read);
        if (w == 0) continue;
        wsum += (unsigned long long)w;
        unsigned long long *a = &acc[h.family * MC_BOOT_LANES + lane];
        const int st = mc_boot_stat(P, h.family);
        if (st == MC_BOOT_COV) *a = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)*a) + (double)w * ((double)h.aln / (double)h.target_len));
        else *a += (unsigned long long)w * (unsigned long long)(st == MC_BOOT_ALN ? h.aln : 1);
    }
    if (b >= P.B) return;
    unsigned long long *out = part + (size_t)blockIdx.x * (size_t)(P.nfam + 1) * (size_t)P.B + (size_t)b;
    for (int f = 0; f < P.nfam; f++) out[(size_t)f * (size_t)P.B] = acc[f * MC_BOOT_LANES + lane];
    out[(size_t)P.nfam * (size_t)P.B] = wsum;
}

// one thread per (row, b): the tiles' partial sums added in ascending tile order; sums_i64 [B][nfam + 1], sums_f64 [B][nfam]
__global__ void __launch_bounds__(256) k_bootstrap_reduce(McBootPars P, int ntiles, const unsigned long long *__restrict__ part, long long *__restrict__ sums_i64, double *__restrict__ sums_f64)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t rows = P.nfam + 1;
    if (t >= rows * P.B) return;
    const int f = (int)(t / P.B);
    const int64_t b = t % P.B;
    const bool cov = f < P.nfam && mc_boot_stat(P, f) == MC_BOOT_COV;
    unsigned long long si = 0ull; double sd = 0.0;
    for (int k = 0; k < ntiles; k++) {
        const unsigned long long v = part[((size_t)k * (size_t)rows + (size_t)f) * (size_t)P.B + (size_t)b];
        if (cov) sd += __longlong_as_double((long long)v); else si += v;
    }
    sums_i64[b * rows + f] = cov ? 0ll : (long long)si;
    if (f < P.nfam) sums_f64[b * P.nfam + f] = cov ? sd : 0.0;
}
