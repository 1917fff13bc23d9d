// k_community.h - the library of a mock community: M member genomes with a number of copies (cells) each, sequenced as one mixture.
#pragma once
#include "mc_hip_common.h"
#include "mc_simlib.h"                // mc_sim_place (the draw), mc_sim_walk (the read)
#include "k_simulate.h"               // McSimKind

// A read comes from member m with probability proportional to copies[m] x (valid starts of m); inside the member it is the read of
// k_simulate.h.  mc_simlib.h states the draw (cum, total, vstart per member; u = mix(key + frag) % universe); the kernels below are
// k_simulate and k_simulate_lib with that place in front: two binary searches per read (member, then the member's contigs)
// instead of one, and a second 64-bit remainder.  The bases of all members lie in one allocation with 64 bytes of slack behind it.
//
// cum[] of a community of up to MC_COMM_LDS_M members is staged in LDS by every block (the first search of every read runs on it);
// larger tables are searched where they lie (L2).
//
// Reads per member of a pass, as a by-product (never one device atomic per read): a block counts into an LDS histogram
// (one ds_add per read; lanes of a wave that drew the same member serialise there, which costs a few cycles per wave beside the
// copy of 64 reads) and flushes it with one device atomic per member it touched.  Without the LDS table (M > MC_COMM_LDS_M) a
// block writes its members to LDS and the first thread of every distinct member adds that member's count: again one device atomic
// per (block, member touched).  counts: int64, a mate counts as a read.
#define MC_COMM_LDS_M 1024

struct McCommTable {
    const uint64_t *cum;              // [M + 1]
    const int64_t *total;             // [M]
    const int32_t *mfirst;            // [M + 1]
    const int64_t *vstart;            // [ncontig], per member from 0
    const int64_t *off;               // [ncontig + 1]
    int M, lds;                       // lds: cum staged in LDS, histogram in LDS
};
static inline size_t comm_lds_bytes(int M) { return M <= MC_COMM_LDS_M ? (size_t)8 * (M + 1) + (size_t)4 * M : 0; }

// stage cum and clear the histogram (T.lds is the same in every thread: the barrier is uniform); returns the table to search
__device__ inline const uint64_t *comm_stage(const McCommTable &T, uint8_t *lds, uint32_t **hist)
{
    *hist = nullptr;
    if (!T.lds) return T.cum;
    uint64_t *s_cum = (uint64_t *)lds;
    uint32_t *s_hist = (uint32_t *)(lds + 8 * (size_t)(T.M + 1));
    for (int t = threadIdx.x; t <= T.M; t += blockDim.x) s_cum[t] = T.cum[t];
    for (int t = threadIdx.x; t < T.M; t += blockDim.x) s_hist[t] = 0;
    __syncthreads();
    *hist = s_hist;
    return s_cum;
}

// after the barrier behind the block's last count: its counts to the device, one atomic per member it touched
__device__ inline void comm_flush(const McCommTable &T, const uint32_t *s_hist, const int32_t *s_mem, int nvalid, unsigned long long *counts)
{
    if (T.lds) {
        for (int m = threadIdx.x; m < T.M; m += blockDim.x) { const uint32_t k = s_hist[m]; if (k) atomicAdd(&counts[m], (unsigned long long)k); }
    } else if ((int)threadIdx.x < nvalid) {
        const int32_t mine = s_mem[threadIdx.x];
        unsigned k = 0;
        bool first = true;
        for (int j = 0; j < nvalid; j++) { const bool eq = s_mem[j] == mine; k += eq; first = first && !(eq && j < (int)threadIdx.x); }
        if (first) atomicAdd(&counts[mine], (unsigned long long)k);
    }
}

// The default kind (single end, no errors): 256 threads per block, every thread places one read, then each wave copies the 64 reads
// of its lanes, a byte per lane (k_simulate's copy).  Dynamic LDS: comm_lds_bytes(M).
__global__ void __launch_bounds__(256) k_community(const uint8_t *__restrict__ bases, McCommTable T, int L, uint64_t key, int64_t first, int64_t n,
                                                   uint8_t *__restrict__ dst, unsigned long long *__restrict__ counts)
{
    __shared__ int64_t s_start[256];
    __shared__ int32_t s_mem[256];
    uint32_t *s_hist;
    const uint64_t *cum = comm_stage(T, mc_smem, &s_hist);
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    const int64_t k = r0 + threadIdx.x;
    if (k < n) {
        const McSimPlace p = mc_sim_place(cum, T.total, T.mfirst, T.vstart, T.off, T.M, mc_mix64(key + (uint64_t)(first + k)));
        s_start[threadIdx.x] = p.start;
        if (T.lds) atomicAdd(&s_hist[p.member], 1u); else s_mem[threadIdx.x] = p.member;
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = 0; j < 64; j++) {
        const int t = w * 64 + j;
        const int64_t r = r0 + t;
        if (r >= n) break;
        const uint8_t *src = bases + s_start[t];
        uint8_t *out = dst + r * (int64_t)L;
        for (int b = lane; b < L; b += 64) out[b] = src[b];
    }
    comm_flush(T, s_hist, s_mem, (int)(n - r0 < 256 ? n - r0 : 256), counts);
}

// Every other library kind (k_simulate_lib with the community's place): one wave per block, a lane walks its read into its LDS row,
// the rows leave as words.  Dynamic LDS: 64 x L bytes of rows, the thresholds, then comm_lds_bytes(M).
__global__ void __launch_bounds__(64) k_community_lib(const uint8_t *__restrict__ bases, McCommTable T, McSimKind kind, const uint64_t *__restrict__ thr,
                                                      uint64_t key, uint64_t ekey, int64_t first, int64_t n, uint8_t *__restrict__ dst,
                                                      unsigned long long *__restrict__ counts)
{
    __shared__ int32_t s_mem[64];
    const int L = kind.L;
    uint8_t *s_rows = mc_smem;
    uint64_t *s_thr = (uint64_t *)(mc_smem + 64 * L);                // (64 x L is a multiple of 8)
    if (kind.errors) for (int t = threadIdx.x; t < MC_SIM_NTHR; t += 64) s_thr[t] = thr[t];
    uint32_t *s_hist;
    const uint64_t *cum = comm_stage(T, mc_smem + 64 * L + 8 * MC_SIM_NTHR, &s_hist);
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int64_t k = r0 + threadIdx.x;
    if (k < n) {
        const int64_t i = first + k;
        const McSimPlace pl = mc_sim_place(cum, T.total, T.mfirst, T.vstart, T.off, T.M, mc_mix64(key + (uint64_t)(kind.paired ? i >> 1 : i)));
        if (T.lds) atomicAdd(&s_hist[pl.member], 1u); else s_mem[threadIdx.x] = pl.member;
        const int64_t cs = T.off[pl.contig], ce = T.off[pl.contig + 1], s = pl.start;
        const bool rev = kind.paired && (i & 1);
        const uint64_t *words = (const uint64_t *)bases;
        int64_t wi = -1;
        uint64_t word = 0;
        auto base = [&](int64_t p) -> uint8_t {
            if ((p >> 3) != wi) { wi = p >> 3; word = words[wi]; }
            return (uint8_t)(word >> (8 * (p & 7)));
        };
        uint8_t *row = s_rows + threadIdx.x * L;
        auto emit = [&](int o, uint8_t x) { row[o] = x; };
        McSimNoEvent ev;
        mc_sim_walk(base, emit, ev, cs, ce, rev ? s + kind.span - 1 : s, rev ? -1 : 1, L, mc_mix64(ekey + (uint64_t)i), s_thr, kind.errors != 0);
    }
    __syncthreads();
    const int nrows = (int)(n - r0 < 64 ? n - r0 : 64), nb = nrows * L;
    uint8_t *out = dst + r0 * L;
    for (int t = threadIdx.x; t < (nb >> 2); t += 64) ((uint32_t *)out)[t] = ((const uint32_t *)s_rows)[t];
    for (int t = (nb & ~3) + threadIdx.x; t < nb; t += 64) out[t] = s_rows[t];
    comm_flush(T, s_hist, s_mem, nrows, counts);
}
