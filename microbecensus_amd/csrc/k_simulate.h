// k_simulate.h - the training workflow's library simulator (training/seq_sim.py as sim_reads.py calls it: single end, no errors, --cov).
#pragma once
#include "mc_hip_common.h"

// seq_sim.py picks a scaffold with probability proportional to its length, a start uniform in [0, len), and throws the fragment
// away when fewer than L bases follow: the reads it keeps are uniform over every (contig, start) with start + L <= len, genome-wide.
// Here that distribution is sampled directly.  vstart[c] = valid starts of contigs 0 .. c-1 (vstart[ncontig] = total > 0); read i of
// library `lib` under seed `seed` is
//     mix(z)  = splitmix64 finaliser of z + 0x9E3779B97F4A7C15 (shifts 30, 27, 31; multipliers 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)
//     key     = mix(seed ^ mix(lib))
//     u       = mix(key + i) % total                                           (all arithmetic modulo 2^64)
//     c       = the contig with vstart[c] <= u < vstart[c + 1]
//     read    = bases[off[c] + (u - vstart[c]) ...][0 .. L)                     (forward strand, bytes as in the FASTA)
// A read depends on (seed, lib, i) alone: how a library is cut into ranges, or which device makes it, never changes it.
__host__ __device__ inline uint64_t mc_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 256 threads per block: every thread places one read, then each wave copies the 64 reads of its lanes, a byte per lane, so that
// the loads and the stores of a read are contiguous.  dst row k = read first + k.
__global__ void __launch_bounds__(256) k_simulate(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int64_t *__restrict__ vstart,
                                                  int ncontig, int L, uint64_t key, int64_t first, int64_t n, uint8_t *__restrict__ dst)
{
    __shared__ int64_t s_start[256];
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) {
        const uint64_t total = (uint64_t)vstart[ncontig];
        const uint64_t u = mc_mix64(key + (uint64_t)(first + k)) % total;
        int lo = 0, hi = ncontig;                                    // the first contig whose vstart exceeds u, minus one
        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((uint64_t)vstart[mid] <= u) lo = mid + 1; else hi = mid; }
        const int c = lo - 1;
        s_start[threadIdx.x] = off[c] + (int64_t)(u - (uint64_t)vstart[c]);
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = 0; j < 64; j++) {
        const int t = w * 64 + j;
        const int64_t r = (int64_t)blockIdx.x * 256 + t;
        if (r >= n) break;
        const uint8_t *src = bases + s_start[t];
        uint8_t *out = dst + r * (int64_t)L;
        for (int b = lane; b < L; b += 64) out[b] = src[b];
    }
}
