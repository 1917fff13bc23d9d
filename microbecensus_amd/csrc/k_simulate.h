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
// That is the default library (single end, no errors); the other kinds (mc_genome_set_library) are k_sim_walk's below.
//
// The kernels are written once and take a PLACER: a small device type that answers "where does fragment `frag` under `key` start"
// with a McSimSpot, and has two per-block hooks - stage(lds) in front of the block's reads (every thread calls it) and flush(nvalid)
// behind them (every thread calls it, after the barrier that follows the block's last at()).  Two placers: McGenomePlacer here (the
// draw above; no LDS, empty hooks) and McCommPlacer (k_community.h: a member first, then the draw above inside it).
struct McSimSpot { int contig; int64_t cs, ce, start; };            // the contig, its bounds [cs, ce) and the fragment's first base, all in `bases`

struct McGenomePlacer {
    const int64_t *off, *vstart;                                    // [ncontig + 1] each
    int ncontig;
    size_t lds_bytes() const { return 0; }
    template <int NT> __device__ __forceinline__ void stage(uint8_t *) {}
    __device__ __forceinline__ McSimSpot at(uint64_t key, int64_t frag)
    {
        const uint64_t u = mc_mix64(key + (uint64_t)frag) % (uint64_t)vstart[ncontig];
        const int c = mc_sim_contig(vstart, ncontig, u);
        return {c, off[c], off[c + 1], off[c] + (int64_t)(u - (uint64_t)vstart[c])};
    }
    __device__ __forceinline__ void flush(int) {}
};

// The default kind.  256 threads per block: every thread places one read, then each wave copies the 64 reads of its lanes, a byte
// per lane, so that the loads and the stores of a read are contiguous.  dst row k = read first + k.  Dynamic LDS: the placer's.
template <class P>
__global__ void __launch_bounds__(256) k_sim_copy(const uint8_t *__restrict__ bases, P place, int L, uint64_t key, int64_t first, int64_t n, uint8_t *__restrict__ dst)
{
    __shared__ int64_t s_start[256];
    place.template stage<256>(mc_smem);
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    const int64_t k = r0 + threadIdx.x;
    if (k < n) s_start[threadIdx.x] = place.at(key, first + k).start;
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
    place.flush((int)(n - r0 < 256 ? n - r0 : 256));
}

// Every other library kind: errors (uniform / illumina) and / or paired end.  mc_simlib.h states the formula (row i of the
// library; the starts of `span` = insert or L bases are the placer's).  One wave per block, a lane per read: the lane walks its read
// into its LDS row, fetching the genome through one aligned 8-byte word it keeps (a walk never leaves its contig, and the genome buffer
// has 64 bytes of slack behind it, so every word read lies inside the allocation).  Then the block's rows - one contiguous span of
// dst, starting at a multiple of 64 x L bytes - go out as 4-byte words.  Dynamic LDS: 64 x L bytes of rows, the thresholds, then
// the placer's.
struct McSimKind { int L, paired, span, errors; };

struct McSimFetch {                                                  // base(p): the byte at p of `bases`, through the word it keeps
    const uint64_t *words;
    int64_t wi = -1;
    uint64_t word = 0;
    __device__ __forceinline__ explicit McSimFetch(const uint8_t *bases) : words((const uint64_t *)bases) {}
    __device__ __forceinline__ uint8_t operator()(int64_t p)
    {
        if ((p >> 3) != wi) { wi = p >> 3; word = words[wi]; }
        return (uint8_t)(word >> (8 * (p & 7)));
    }
};

// row i of a library: where its walk begins, which way it goes, and the state of its error stream
struct McSimRow { McSimSpot spot; int64_t p0; int dir; uint64_t r; };
template <class P>
__device__ __forceinline__ McSimRow mc_sim_row(P &place, const McSimKind &kind, uint64_t key, uint64_t ekey, int64_t i)
{
    const McSimSpot sp = place.at(key, kind.paired ? i >> 1 : i);
    const bool rev = kind.paired && (i & 1);
    return {sp, rev ? sp.start + kind.span - 1 : sp.start, rev ? -1 : 1, mc_mix64(ekey + (uint64_t)i)};
}

// the first nb bytes of the block's LDS rows to out (4-byte aligned), as words and a tail of bytes
__device__ __forceinline__ void mc_sim_rows_out(const uint8_t *s_rows, int nb, uint8_t *out)
{
    for (int t = threadIdx.x; t < (nb >> 2); t += 64) ((uint32_t *)out)[t] = ((const uint32_t *)s_rows)[t];
    for (int t = (nb & ~3) + threadIdx.x; t < nb; t += 64) out[t] = s_rows[t];
}

template <class P>
__global__ void __launch_bounds__(64) k_sim_walk(const uint8_t *__restrict__ bases, P place, McSimKind kind, const uint64_t *__restrict__ thr, uint64_t key,
                                                 uint64_t ekey, int64_t first, int64_t n, uint8_t *__restrict__ dst)
{
    const int L = kind.L;
    uint8_t *s_rows = mc_smem;
    uint64_t *s_thr = (uint64_t *)(mc_smem + 64 * L);                // (64 x L is a multiple of 8)
    if (kind.errors) for (int t = threadIdx.x; t < MC_SIM_NTHR; t += 64) s_thr[t] = thr[t];
    place.template stage<64>(mc_smem + 64 * L + 8 * MC_SIM_NTHR);
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int64_t k = r0 + threadIdx.x;
    if (k < n) {
        const McSimRow w = mc_sim_row(place, kind, key, ekey, first + k);
        McSimFetch base(bases);
        uint8_t *row = s_rows + threadIdx.x * L;
        auto emit = [&](int o, uint8_t x) { row[o] = x; };
        McSimNoEvent ev;
        mc_sim_walk(base, emit, ev, w.spot.cs, w.spot.ce, w.p0, w.dir, L, w.r, s_thr, kind.errors != 0);
    }
    __syncthreads();
    const int nrows = (int)(n - r0 < 64 ? n - r0 : 64);
    mc_sim_rows_out(s_rows, nrows * L, dst + r0 * L);
    place.flush(nrows);
}

// The reference read-length mode (mc_simlib.h, mc_sim_walk_ref): reads of L + insertions - deletions bases, back to back.  Two passes
// over the same pure function of (seed, library, row): lens != NULL writes each read's length; otherwise the read is written at
// dst + off[k] - off[0] (off: the exclusive scan of the lengths, k_sim_scan).  A lane per read.  The genome's libraries only.
__global__ void __launch_bounds__(64) k_simulate_var(const uint8_t *__restrict__ bases, McGenomePlacer place, McSimKind kind, const uint64_t *__restrict__ thr,
                                                     uint64_t key, uint64_t ekey, int64_t first, int64_t n, uint32_t *__restrict__ lens,
                                                     const int64_t *__restrict__ roff, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_thr[MC_SIM_NTHR];
    if (kind.errors) for (int t = threadIdx.x; t < MC_SIM_NTHR; t += 64) s_thr[t] = thr[t];
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const McSimRow w = mc_sim_row(place, kind, key, ekey, first + k);
    McSimFetch base(bases);
    if (lens) {
        auto count = [](int, uint8_t) {};
        lens[k] = (uint32_t)mc_sim_walk_ref(base, count, w.p0, w.dir, kind.L, w.r, thr ? s_thr : nullptr, kind.errors != 0);
    } else {
        uint8_t *row = dst + (roff[k] - roff[0]);
        auto emit = [&](int o, uint8_t x) { row[o] = x; };
        (void)mc_sim_walk_ref(base, emit, w.p0, w.dir, kind.L, w.r, thr ? s_thr : nullptr, kind.errors != 0);
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
