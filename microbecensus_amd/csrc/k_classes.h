// k_classes.h - a batch of padded read rows sorted into its length classes on the device (mc_search_classes; the rule: mc_classes.h).
// The fixed-length pipeline then runs once per class, each class's reads back to back at that class's length.  k_varlen.h's scheme
// with at most MC_CL_BINS = 33 bins (the K classes and "no class"), which fit in LDS and registers, and a gather that trims.
//   k_cl_hist     per tile of MC_CL_TILE rows: the length of every row (P lanes per row, one aligned 16-byte load each, a min over the
//                 P lanes), its class (cls[row]; K = none), and how many rows of each class; counts[bin * ntiles + tile]
//   k_bin_scan    (k_varlen.h's, with nbins = K + 1) exclusive scan of counts in that (bin-major) order -> where each tile's rows of
//                 each class go; start[bin] = first sorted position of the class, start[nbins] = n
//   k_cl_scatter  perm[sorted position] = row index; stable: within a class the row indices ascend.  Ranks come from wave ballots
//                 (one round per class present in the wave), not from a scan over the workgroup's rows
//   k_cl_gather   the first class_len[k] bytes of every row of class k to that class's block of dst (16-byte aligned), a thread per
//                 16 bytes of DESTINATION: two aligned 16-byte loads, a funnel shift and one 16-byte store where the 16 bytes lie in one
//                 row (all but 16 / class_len of them), bytes otherwise; a block's last word is filled up with 0 bytes.  Rows without a
//                 class are not copied.
// The rows buffer is 16-byte aligned and has MC_CL_SLACK readable bytes behind its last row; dst has them behind its last block.
#pragma once
#include "mc_classes.h"
#include "k_varlen.h"                                                // (k_bin_scan)

#define MC_CL_BINS (MC_CLS_MAX + 1)
#define MC_CL_TILE 4096
#define MC_CL_BS 256
#define MC_CL_SLACK 64

// lanes per row: the power of two that holds the aligned 16-byte words a row can touch, (stride + 30) / 16 of them at most (<= 33)
static inline int mc_cl_lanes(int stride)
{
    int p = 1;
    while (p * 16 < stride + 30) p <<= 1;
    return p;
}

__global__ void __launch_bounds__(MC_CL_BS) k_cl_hist(const uint8_t *__restrict__ rows, int64_t n, int stride, McClasses C, int P, uint32_t ntiles,
                                                      uint8_t *__restrict__ cls, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t hist[MC_CL_BINS];
    if (threadIdx.x < MC_CL_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    const int sub = threadIdx.x & (P - 1), per = MC_CL_BS / P;         // this lane's word of the row; rows per round of the workgroup
    const int64_t base = (int64_t)blockIdx.x * MC_CL_TILE;
    for (int k = threadIdx.x / P; k < MC_CL_TILE; k += per) {           // (the P lanes of a row share k: the shuffles below are convergent)
        const int64_t i = base + k;
        int len = stride;
        if (i < n) {
            const int64_t s = i * stride;
            const int m = (int)(s & 15), j0 = sub * 16 - m;           // row-relative index of the word's first byte
            if (j0 < stride) {
                const uint4 w = *(const uint4 *)(rows + (s - m) + (int64_t)sub * 16);
                const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int b = 15; b >= 0; b--) {
                    const int j = j0 + b;
                    if (((d[b >> 2] >> (8 * (b & 3))) & 255u) == 0 && j >= 0 && j < stride) len = j;
                }
            }
        }
        for (int o = P >> 1; o; o >>= 1) len = min(len, __shfl_xor(len, o));
        if (sub == 0 && i < n) {
            const int c = mc_class_of(C, len);
            cls[i] = (uint8_t)c;
            atomicAdd(&hist[c], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x <= (unsigned)C.K) counts[(size_t)threadIdx.x * ntiles + blockIdx.x] = hist[threadIdx.x];
}

__global__ void __launch_bounds__(MC_CL_BS) k_cl_scatter(const uint8_t *__restrict__ cls, int64_t n, uint32_t ntiles, uint32_t nbins, const uint32_t *__restrict__ tile_off,
                                                         uint32_t *__restrict__ perm)
{
    __shared__ uint32_t cnt[MC_CL_BINS];                               // rows of each class in the rounds before
    __shared__ uint32_t wcnt[MC_CL_BS / 64][MC_CL_BINS];               // ... and in each wave of this round
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t < MC_CL_BINS) cnt[t] = 0;
    const int64_t base = (int64_t)blockIdx.x * MC_CL_TILE;
    for (int r = 0; r < MC_CL_TILE / MC_CL_BS; r++) {
        const int64_t i = base + r * MC_CL_BS + t;
        const int b = i < n ? (int)cls[i] : 255;
        for (int j = t; j < (MC_CL_BS / 64) * MC_CL_BINS; j += MC_CL_BS) (&wcnt[0][0])[j] = 0;
        __syncthreads();
        uint32_t rank = 0;
        unsigned long long todo = __ballot(b != 255);
        while (todo) {                                               // (wave-uniform: one round per class present)
            const int lead = __ffsll(todo) - 1;
            const int bb = __shfl(b, lead);
            const unsigned long long m = __ballot(b == bb);
            if (b == bb) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == lead) wcnt[wv][bb] = (uint32_t)__popcll(m);
            todo &= ~m;
        }
        __syncthreads();
        if (i < n) {
            uint32_t pre = cnt[b];
            for (int w = 0; w < wv; w++) pre += wcnt[w][b];
            perm[tile_off[(size_t)b * ntiles + blockIdx.x] + pre + rank] = (uint32_t)i;
        }
        __syncthreads();
        if (t < (int)nbins) { uint32_t a = 0; for (int w = 0; w < MC_CL_BS / 64; w++) a += wcnt[w][t]; cnt[t] += a; }
        __syncthreads();
    }
}

// what the gather needs of the host's view of the scan: per class its first sorted position, its rows, its first 16-byte word of dst
struct McClGather { int32_t K; uint32_t first[MC_CL_BINS], cnt[MC_CL_BINS]; int64_t word0[MC_CL_BINS + 1]; };

#define MC_CL_GATHER_BLOCKS 8192
__global__ void __launch_bounds__(MC_CL_BS) k_cl_gather(const uint8_t *__restrict__ rows, int stride, const uint32_t *__restrict__ perm, McClasses C, McClGather G,
                                                        uint8_t *__restrict__ dst)
{
    const int64_t W = G.word0[G.K], step = (int64_t)gridDim.x * MC_CL_BS;
    for (int64_t w = (int64_t)blockIdx.x * MC_CL_BS + threadIdx.x; w < W; w += step) {
        int k = 0;
        while (w >= G.word0[k + 1]) k++;
        const int L = C.len[k];
        const int64_t o = (w - G.word0[k]) * 16, total = (int64_t)G.cnt[k] * L;   // byte of the class's block; its size
        const int64_t r = o / L;
        const int c = (int)(o - r * L);
        uint8_t *d = dst + G.word0[k] * 16 + o;
        const uint32_t *pk = perm + G.first[k];
        if (c + 16 <= L) {                                             // (then o + 16 <= total too)
            const uint8_t *s = rows + (int64_t)pk[r] * stride + c;
            const int sh = (int)((uintptr_t)s & 15);
            const uint4 a = *(const uint4 *)(s - sh), b = *(const uint4 *)(s - sh + 16);
            const int q = sh >> 2, bs = (sh & 3) * 8;
            const uint32_t e0 = q == 0 ? a.x : q == 1 ? a.y : q == 2 ? a.z : a.w, e1 = q == 0 ? a.y : q == 1 ? a.z : q == 2 ? a.w : b.x,
                           e2 = q == 0 ? a.z : q == 1 ? a.w : q == 2 ? b.x : b.y, e3 = q == 0 ? a.w : q == 1 ? b.x : q == 2 ? b.y : b.z,
                           e4 = q == 0 ? b.x : q == 1 ? b.y : q == 2 ? b.z : b.w;
            uint4 v;
            v.x = (uint32_t)((((uint64_t)e1 << 32) | e0) >> bs); v.y = (uint32_t)((((uint64_t)e2 << 32) | e1) >> bs);
            v.z = (uint32_t)((((uint64_t)e3 << 32) | e2) >> bs); v.w = (uint32_t)((((uint64_t)e4 << 32) | e3) >> bs);
            *(uint4 *)d = v;
        } else {
            for (int b = 0; b < 16; b++) {                           // (the bytes behind a block's last read, up to its 16-byte end, are 0)
                const int cc = c + b;
                d[b] = o + b >= total ? (uint8_t)0 : cc < L ? rows[(int64_t)pk[r] * stride + cc] : rows[(int64_t)pk[r + 1] * stride + (cc - L)];
            }
        }
    }
}
