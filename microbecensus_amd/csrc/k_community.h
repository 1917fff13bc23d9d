// k_community.h - the library of a mock community: M member genomes with a number of copies (cells) each, sequenced as one mixture.
#pragma once
#include "mc_hip_common.h"
#include "mc_simlib.h"                // mc_sim_place (the draw)
#include "k_simulate.h"               // McSimSpot, the kernels this placer is given to

// A read comes from member m with probability proportional to copies[m] x (valid starts of m); inside the member it is the read of
// k_simulate.h.  mc_simlib.h states the draw (cum, total, vstart per member; u = mix(key + frag) % universe); McCommPlacer below puts
// that place in front of k_simulate.h's kernels (k_sim_copy, k_sim_walk): two binary searches per read (member, then the member's
// contigs) instead of one, and a second 64-bit remainder.  The bases of all members lie in one allocation with 64 bytes of slack
// behind it.
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

struct McCommPlacer {
    const uint64_t *cum;              // [M + 1]
    const int64_t *total;             // [M]
    const int32_t *mfirst;            // [M + 1]
    const int64_t *vstart;            // [ncontig], per member from 0
    const int64_t *off;               // [ncontig + 1]
    int M, lds;                       // lds: cum staged in LDS, histogram in LDS
    unsigned long long *counts;       // [M]: reads per member of the pass
    const uint64_t *s_cum;            // the block's own, set by stage(): the table to search, the LDS histogram, the members of its threads
    uint32_t *s_hist;
    int32_t *s_mem;

    size_t lds_bytes() const { return M <= MC_COMM_LDS_M ? (size_t)8 * (M + 1) + (size_t)4 * M : 0; }

    // stage cum and clear the histogram (lds is the same in every thread: the barrier is uniform); NT: the threads of a block
    template <int NT> __device__ __forceinline__ void stage(uint8_t *smem)
    {
        __shared__ int32_t mem[NT];
        s_mem = mem; s_hist = nullptr; s_cum = cum;
        if (!lds) return;
        uint64_t *c = (uint64_t *)smem;
        s_hist = (uint32_t *)(smem + 8 * (size_t)(M + 1));
        for (int t = threadIdx.x; t <= M; t += NT) c[t] = cum[t];
        for (int t = threadIdx.x; t < M; t += NT) s_hist[t] = 0;
        __syncthreads();
        s_cum = c;
    }

    __device__ __forceinline__ McSimSpot at(uint64_t key, int64_t frag)
    {
        const McSimPlace p = mc_sim_place(s_cum, total, mfirst, vstart, off, M, mc_mix64(key + (uint64_t)frag));
        if (lds) atomicAdd(&s_hist[p.member], 1u); else s_mem[threadIdx.x] = p.member;
        return {p.contig, off[p.contig], off[p.contig + 1], p.start};
    }

    // after the barrier behind the block's last count: its counts to the device, one atomic per member it touched
    __device__ __forceinline__ void flush(int nvalid)
    {
        if (lds) {
            for (int m = threadIdx.x; m < M; m += blockDim.x) { const uint32_t k = s_hist[m]; if (k) atomicAdd(&counts[m], (unsigned long long)k); }
        } else if ((int)threadIdx.x < nvalid) {
            const int32_t mine = s_mem[threadIdx.x];
            unsigned k = 0;
            bool first = true;
            for (int j = 0; j < nvalid; j++) { const bool eq = s_mem[j] == mine; k += eq; first = first && !(eq && j < (int)threadIdx.x); }
            if (first) atomicAdd(&counts[mine], (unsigned long long)k);
        }
    }
};
