// k_simulate.h - the training workflow's library simulator (training/seq_sim.py as sim_reads.py calls it: single end, no errors, --cov).
#pragma once
#include "mc_hip_common.h"
#include "mc_simlib.h"                // mc_mix64 (the formula below), and the generator of the other library kinds

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
// That is the default library (single end, no errors); the other kinds (mc_genome_set_library) are k_simulate_lib's below.
//
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

// Every other library kind: errors (uniform / illumina) and / or paired end.  mc_simlib.h states the formula (row i of the
// library; the starts of `span` = insert or L bases are vstart's).  One wave per block, a lane per read: the lane walks its read into
// its LDS row, fetching the genome through one aligned 8-byte word it keeps (a walk never leaves its contig, and the genome buffer
// has 64 bytes of slack behind it, so every word read lies inside the allocation).  Then the block's rows - one contiguous span of
// dst, starting at a multiple of 64 x L bytes - go out as 4-byte words.  Dynamic LDS: 64 x L bytes of rows, then the thresholds.
struct McSimKind { int L, paired, span, errors; };

__global__ void __launch_bounds__(64) k_simulate_lib(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int64_t *__restrict__ vstart,
                                                     int ncontig, McSimKind kind, const uint64_t *__restrict__ thr, uint64_t key, uint64_t ekey, int64_t first,
                                                     int64_t n, uint8_t *__restrict__ dst)
{
    const int L = kind.L;
    uint8_t *s_rows = mc_smem;
    uint64_t *s_thr = (uint64_t *)(mc_smem + 64 * L);                // (64 x L is a multiple of 8)
    if (kind.errors) for (int t = threadIdx.x; t < MC_SIM_NTHR; t += 64) s_thr[t] = thr[t];
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k < n) {
        const int64_t i = first + k;
        const uint64_t u = mc_mix64(key + (uint64_t)(kind.paired ? i >> 1 : i)) % (uint64_t)vstart[ncontig];
        const int c = mc_sim_contig(vstart, ncontig, u);
        const int64_t cs = off[c], ce = off[c + 1], s = cs + (int64_t)(u - (uint64_t)vstart[c]);
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
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int nb = (int)(n - r0 < 64 ? n - r0 : 64) * L;
    uint8_t *out = dst + r0 * L;
    for (int t = threadIdx.x; t < (nb >> 2); t += 64) ((uint32_t *)out)[t] = ((const uint32_t *)s_rows)[t];
    for (int t = (nb & ~3) + threadIdx.x; t < nb; t += 64) out[t] = s_rows[t];
}

// The reference read-length mode (mc_simlib.h, mc_sim_walk_ref): reads of L + insertions - deletions bases, back to back.  Two passes
// over the same pure function of (seed, library, row): lens != NULL writes each read's length; otherwise the read is written at
// dst + off[k] - off[0] (off: the exclusive scan of the lengths, k_sim_scan).  A lane per read.
__global__ void __launch_bounds__(64) k_simulate_var(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int64_t *__restrict__ vstart,
                                                     int ncontig, McSimKind kind, const uint64_t *__restrict__ thr, uint64_t key, uint64_t ekey, int64_t first,
                                                     int64_t n, uint32_t *__restrict__ lens, const int64_t *__restrict__ roff, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_thr[MC_SIM_NTHR];
    if (kind.errors) for (int t = threadIdx.x; t < MC_SIM_NTHR; t += 64) s_thr[t] = thr[t];
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int64_t i = first + k;
    const uint64_t u = mc_mix64(key + (uint64_t)(kind.paired ? i >> 1 : i)) % (uint64_t)vstart[ncontig];
    const int c = mc_sim_contig(vstart, ncontig, u);
    const int64_t s = off[c] + (int64_t)(u - (uint64_t)vstart[c]);
    const bool rev = kind.paired && (i & 1);
    const uint64_t *words = (const uint64_t *)bases;
    int64_t wi = -1;
    uint64_t word = 0;
    auto base = [&](int64_t p) -> uint8_t {
        if ((p >> 3) != wi) { wi = p >> 3; word = words[wi]; }
        return (uint8_t)(word >> (8 * (p & 7)));
    };
    const int64_t p0 = rev ? s + kind.span - 1 : s;
    const uint64_t r = mc_mix64(ekey + (uint64_t)i);
    if (lens) {
        auto count = [](int, uint8_t) {};
        lens[k] = (uint32_t)mc_sim_walk_ref(base, count, p0, rev ? -1 : 1, kind.L, r, thr ? s_thr : nullptr, kind.errors != 0);
    } else {
        uint8_t *row = dst + (roff[k] - roff[0]);
        auto emit = [&](int o, uint8_t x) { row[o] = x; };
        (void)mc_sim_walk_ref(base, emit, p0, rev ? -1 : 1, kind.L, r, thr ? s_thr : nullptr, kind.errors != 0);
    }
}

// exclusive scan of n read lengths into off[0 .. n] (one workgroup of 1024 threads; n <= a streaming batch)
__global__ void __launch_bounds__(1024) k_sim_scan(const uint32_t *__restrict__ lens, int64_t n, int64_t *__restrict__ off)
{
    __shared__ int64_t part[1024];
    const int64_t t = threadIdx.x, chunk = (n + 1023) / 1024;
    const int64_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    int64_t s = 0;
    for (int64_t i = lo; i < hi; i++) s += lens[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int64_t i = lo; i < hi; i++) { off[i] = run; run += lens[i]; }
    if (t == 1023) off[n] = part[1023];
}
