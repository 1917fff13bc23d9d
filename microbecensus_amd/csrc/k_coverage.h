// k_coverage.h - per-gene coverage breadth and depth beside the read counts of k_abundance.h (mc_set_coverage): which residues of a
// gene the reads assigned to it cover, and how often.  A few hundred reads piled on one conserved domain give a high RPKG (the
// reference README's "Normalization") and say nothing about the gene being there; the covered fraction does.
#pragma once
#include "k_abundance.h"

// ---- THE STATEMENT (tests/coverage_restated.py restates it; the kernels below follow it) ------------------------------------------
// Which row counts: a read's best row is exactly the one k_abundance.h defines - the same four cut-offs, the highest bits, the first
// on a tie.
// What it adds: RAPsearch2's subject coordinates are 0-BASED AND INCLUSIVE (mc_row.sstart / send, columns 9 and 10 of its m8:
// 0 <= sstart <= send <= len - 1 in every row).  The best row adds 1 to depth[subject][p] for every p in sstart .. send, both ends
// included; subject residues opposite a gap in the query count too.  (A span that does not lie inside its gene - no row of the engine
// - adds nothing to the depth; the read counts as k_abundance.h says.)
// Per gene s of len residues:
//     covered[s]   = the number of p with depth > 0
//     spanned[s]   = the sum of depth over p      = the sum of send - sstart + 1 over the best rows of s
//     max_depth[s] = the maximum of depth over p
// All figures are exact integers and do not depend on batches, ranges, launch geometry or the order of the atomics.
// Width: depth is 32-bit - a residue covered by 2^32 or more reads wraps; spanned is 64-bit.
// Invariants: covered > 0 iff reads > 0; covered <= min(len, spanned); max_depth <= reads; sum(covered) <= sum(spanned).
//
// ---- Layout -------------------------------------------------------------------------------------------------------------------
// The depth is kept as a difference array of uint32_t: gene s owns len_s + 1 slots from covoff[s] = sum over t < s of (len_t + 1)
// = off[s] + s (off: the index's residue offsets, nseq + 1 of them, on the device anyway - covoff is computed, not stored; the array's
// size: mc_diff_slots, mc_abund.h).  At most
// 32,767 x 2,048 slots: 32 bits hold every offset.  The last slot of a gene is a sentinel: the -1 of a span that ends at len - 1
// lands there and not in the next gene.
// Mark (k_abundance_cov): the best row adds +1 at covoff[s] + sstart and -1 (wrapping) at covoff[s] + send + 1.  depth[p] is the
// wrapping prefix sum of the gene's slots up to p - whatever order the atomics came in.
//
// k_abundance_cov is k_abundance (k_abundance.h: the same walk, the same mc_abund_passes, the same tie rule, the same counters) with
// the best row's span kept and two 32-bit atomics issued beside the two 64-bit ones: the walk over a read's rows happens once, and
// mc_abund_launch (mc_abund.h) launches this kernel INSTEAD of k_abundance while coverage is on.  A kernel of its own, not an instantiation
// of a template both share: DESIGN.md 13.3 has why.  tests/test_gpu_coverage_units.py holds the counters of BOTH kernels to
// tests/abundance_restated.py, so the two walks cannot drift apart unseen.
__global__ void __launch_bounds__(256) k_abundance_cov(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, unsigned long long *tab,
                                                       const uint32_t *__restrict__ off, uint32_t *diff)
{
    __shared__ uint32_t wcnt[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < nrows) {
        const int q = rows[i].query;
        if (i == 0 || rows[i - 1].query != q) {                      // one thread per read: the one at its first row
            double bbits = 0.0; int bsub = -1, baln = 0, bs = 0, be = 0;
            for (uint32_t k = i; k < nrows && rows[k].query == q; k++) {
                const McRow r = rows[k];
                if (!mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge)) continue;   // (McRow::frame carries the identities)
                if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; baln = r.alnlen; bs = r.sstart; be = r.send; }
            }
            if (bsub >= 0 && bsub < nseq) {
                hit = true;
                atomicAdd(&tab[2 * (size_t)bsub], 1ull);
                atomicAdd(&tab[2 * (size_t)bsub + 1], (unsigned long long)baln);
                const uint32_t a = off[bsub] + (uint32_t)bsub, len = off[bsub + 1] - off[bsub];   // (the gene's first slot and its residues)
                if (bs >= 0 && bs <= be && (uint32_t)be < len) {         // (every row of the engine; the guard keeps any other span out of the array: it marks nothing)
                    atomicAdd(&diff[a + (uint32_t)bs], 1u);
                    atomicAdd(&diff[a + (uint32_t)be + 1u], 0xFFFFFFFFu);
                }
            }
        }
    }
    const unsigned long long m = __ballot(hit);
    if (mc_lane() == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (tot) atomicAdd(&tab[2 * (size_t)nseq], (unsigned long long)tot);
    }
}

// inclusive prefix sum over the 64 lanes of a wave (wrapping)
__device__ __forceinline__ uint32_t mc_wave_scan_u32(uint32_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

// Scan, at read time: one wave per gene, four genes per workgroup.  A wave first reads tab[2 s], the gene's read count: a gene without
// reads (on real data nearly all of them) writes three zeros and leaves - its slots are all zero.  Otherwise the gene is walked in
// chunks of 64 slots: the chunk's inclusive wave scan plus the carry of the chunks before it is the depth; covered from a ballot's
// popcount, spanned in a 64-bit lane accumulator, max_depth per lane, both reduced over the wave at the end.
// out: 3 x nseq (covered, spanned, max_depth of gene s at out[3 s ..]).  depth (or null): the depth of every residue, genes one
// after the other without the sentinels (gene s from off[s]); the caller has zeroed it - the genes without reads are not written.
// diff is only read: ranges may go on marking after a read.
__global__ void __launch_bounds__(256) k_coverage_scan(const unsigned long long *__restrict__ tab, const uint32_t *__restrict__ off, const uint32_t *__restrict__ diff,
                                                       int32_t nseq, unsigned long long *out, uint32_t *depth)
{
    const int lane = mc_lane();
    const int32_t s = (int32_t)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (s >= nseq) return;                                         // (wave-uniform)
    unsigned long long *o = out + 3 * (size_t)s;
    if (tab[2 * (size_t)s] == 0) {
        if (lane < 3) o[lane] = 0ull;
        return;
    }
    const uint32_t r0 = off[s], len = off[s + 1] - r0, a = r0 + (uint32_t)s;
    uint32_t carry = 0, covered = 0, mx = 0;
    unsigned long long sum = 0;
    for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t p = base + (uint32_t)lane;
        const bool in = p < len;
        const uint32_t d = mc_wave_scan_u32(in ? diff[a + p] : 0u, lane) + carry;
        carry = __shfl(d, 63, 64);
        covered += (uint32_t)__popcll(__ballot(in && d != 0));
        if (in) {
            sum += d; mx = max(mx, d);
            if (depth) depth[r0 + p] = d;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    }
    if (lane == 0) { o[0] = covered; o[1] = sum; o[2] = mx; }
}
