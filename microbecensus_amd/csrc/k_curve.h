// k_curve.h - a rarefaction curve beside the read counts of k_abundance.h and the coverage of k_coverage.h (mc_set_curve): every figure
// the gene table is built from, as the first n_k sampled reads alone would have given it, at K nested prefixes of the sample.  The
// sampler is a head-take, so point k is exactly what a run with -n n_k returns: whether the sample was sequenced deeply enough, or
// whether twice the reads would have found more genes, is read off one run instead of K.
#pragma once
#include "k_abundance.h"
#include "k_coverage.h"
#include "mc_curve.h"

// ---- THE STATEMENT (tests/curve_restated.py restates it; the kernels below follow it) ---------------------------------------------
// Points n_0 <= n_1 <= ... <= n_{K-1}, 1 <= K <= 64, are 64-bit and each >= 1; repeats are allowed.  They are given to the device
// BEFORE the first range (mc_set_curve zeroes everything below).
// A read's global id q is mc_row.query: first_read_id plus the read's index, 0 <= q < 2^31.
// Which row counts: a read's best row is exactly the one k_abundance.h defines - the same four cut-offs, the highest bits, the first
// on a tie.
// A read with a best row (of a subject in 0 .. nseq - 1) falls into bin b(q) = the number of k with n_k <= q, so b is in 0 .. K: a read
// of bin b belongs to the points k >= b, and bin K means "behind the last point".  The read adds 1 to bin_reads[b][subject] and alnlen
// to bin_aligned[b][subject].
// With coverage on the read also lowers first[subject][p] to min(first, q) for every p in sstart .. send - under k_abundance_cov's guard:
// a span that does not lie inside its gene marks nothing.  first starts at 0xFFFFFFFF, which no id reaches: a residue that holds it is
// covered at no point, however large the points.
// At read time, for every k < K and every gene s:
//     reads_k[s]   = the sum of bin_reads[b][s] over b <= k            aligned_k[s] = the same sum over bin_aligned
//     covered_k[s] = the number of p with first[s][p] != 0xFFFFFFFF and first[s][p] < n_k
//     assigned_k   = the sum of reads_k over s                         beyond = the sum over s of bin_reads[K][s]
// All counters are exact 64-bit integers; first is 32-bit.  Nothing depends on batches, ranges, launch geometry or the order of the
// atomics (sums and minima commute).
// Invariants: reads_k and covered_k do not decrease in k; covered_k > 0 iff reads_k > 0; the sum over all K + 1 bins is the count table
// of mc_abundance_read; with n_{K-1} above every id seen beyond == 0 and row K - 1 is mc_abundance_read's reads and aligned and
// mc_coverage_read's covered.
//
// ---- Layout (the sizes: mc_curve_bin_slots, mc_curve_out_slots in mc_abund.h) ---------------------------------------------------------
// bins: (K + 1) x nseq pairs of counters, bin b of subject s at 2 (b nseq + s): reads, aligned - one 16-byte pair, one line, as in
// k_abundance's table.  first: nres values, gene s from off[s] (no sentinels: nothing is written behind a span).
// The scan's output: K x nseq triples (reads_k, aligned_k, covered_k of gene s at 3 (k nseq + s)), then K + 1 totals: assigned_k, beyond.

// The shape of k_abundance, and a walk of its own over a read's rows (a third copy of k_abundance's walk: whoever edits one edits all;
// DESIGN.md 13.3 has why the walks are separate kernels - and this way the counting kernels are the same instructions with the curve
// on or off).  Launched behind the counting kernel (and k_ties) on the same rows (mc_abund_launch, mc_abund.h).
// The K points are copied into LDS once per workgroup; a read's bin is a binary search there.  Two 64-bit atomics per read into its
// bin's pair.  With coverage (first != null) every residue of the span takes an atomicMin - issued only when a plain load shows a value
// above q: first only ever falls, so a stale load costs a redundant atomic and never a wrong result, and since ranges arrive in
// ascending id order most residues of a well-covered gene are loads only.
__global__ void __launch_bounds__(256) k_curve(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, const unsigned long long *__restrict__ pts, int32_t K,
                                               unsigned long long *bins, const uint32_t *__restrict__ off, uint32_t *first)
{
    __shared__ unsigned long long n[MC_CURVE_MAXK];
    if ((int32_t)threadIdx.x < K) n[threadIdx.x] = pts[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nrows) return;
    const int q = rows[i].query;
    if (i != 0 && rows[i - 1].query == q) return;                   // one thread per read: the one at its first row
    double bbits = 0.0; int bsub = -1, baln = 0, bs = 0, be = 0;
    for (uint32_t k = i; k < nrows && rows[k].query == q; k++) {
        const McRow r = rows[k];
        if (!mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge)) continue;   // (McRow::frame carries the identities)
        if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; baln = r.alnlen; bs = r.sstart; be = r.send; }
    }
    if (bsub < 0 || bsub >= nseq) return;
    const uint32_t uq = (uint32_t)q;
    const size_t slot = 2 * ((size_t)mc_curve_bin(n, K, (unsigned long long)uq) * (size_t)nseq + (size_t)bsub);
    atomicAdd(&bins[slot], 1ull);
    atomicAdd(&bins[slot + 1], (unsigned long long)baln);
    if (!first) return;
    const uint32_t a = off[bsub], len = off[bsub + 1] - a;            // (the gene's first residue and its residues)
    if (bs >= 0 && bs <= be && (uint32_t)be < len) {                 // (k_abundance_cov's guard: any other span marks nothing)
        uint32_t *f = first + a;
        for (uint32_t p = (uint32_t)bs; p <= (uint32_t)be; p++)
            if (f[p] > uq) atomicMin(&f[p], uq);
    }
}

// inclusive prefix sum over the 64 lanes of a wave, 64-bit
__device__ __forceinline__ unsigned long long mc_wave_scan_u64(unsigned long long x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

// Scan, at read time, in the shape of k_coverage_scan: one wave per gene, four genes per workgroup.  A wave first reads tab[2 s], the
// gene's read count in the count table: a gene without reads writes its zeros and leaves.  Otherwise lane k holds point k and bin k of
// the gene: the inclusive wave scans over the bins are reads_k and aligned_k.  With coverage the gene's residues are taken in chunks of
// 64: every lane finds its residue's bin (mc_curve_first_bin, the points in the wave's own LDS copy) and counts it in a per-wave LDS
// histogram; the inclusive wave scan over the histogram is covered_k.  Lane k < K adds reads_k to tot[k] (assigned_k), lane 0 the
// gene's bin K to tot[K] (beyond): the caller has zeroed tot.  first: null with coverage off - covered_k is then written as 0.
// bins and first are only read: ranges may go on counting after a read.
__global__ void __launch_bounds__(256) k_curve_scan(const unsigned long long *__restrict__ tab, const unsigned long long *__restrict__ bins, const unsigned long long *__restrict__ pts,
                                                    int32_t K, const uint32_t *__restrict__ off, const uint32_t *__restrict__ first, int32_t nseq, unsigned long long *out,
                                                    unsigned long long *tot)
{
    __shared__ unsigned long long n[4][MC_CURVE_MAXK];
    __shared__ uint32_t hist[4][MC_CURVE_MAXK + 1];
    const int lane = mc_lane(), w = (int)(threadIdx.x >> 6);
    const int32_t s = (int32_t)(blockIdx.x * 4u + (uint32_t)w);
    if (s >= nseq) return;                                         // (wave-uniform; nothing below synchronises wider than a wave)
    const bool mine = lane < K;
    unsigned long long *o = out + 3 * ((size_t)lane * (size_t)nseq + (size_t)s);
    if (tab[2 * (size_t)s] == 0) {
        if (mine) { o[0] = 0ull; o[1] = 0ull; o[2] = 0ull; }
        return;
    }
    const unsigned long long *b = bins + 2 * ((size_t)lane * (size_t)nseq + (size_t)s);
    const unsigned long long reads_k = mc_wave_scan_u64(mine ? b[0] : 0ull, lane), aligned_k = mc_wave_scan_u64(mine ? b[1] : 0ull, lane);
    uint32_t covered_k = 0;
    if (first) {
        n[w][lane] = mine ? pts[lane] : ~0ull;
        hist[w][lane] = 0;
        if (lane == 0) hist[w][MC_CURVE_MAXK] = 0;
        mc_wave_sync();
        const uint32_t r0 = off[s], len = off[s + 1] - r0;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t p = base + (uint32_t)lane;
            if (p < len) atomicAdd(&hist[w][mc_curve_first_bin(n[w], K, first[r0 + p])], 1u);
        }
        mc_wave_sync();
        covered_k = mc_wave_scan_u32(mine ? hist[w][lane] : 0u, lane);
    }
    if (mine) {
        o[0] = reads_k; o[1] = aligned_k; o[2] = covered_k;
        if (reads_k) atomicAdd(&tot[lane], reads_k);
    }
    if (lane == 0) {
        const unsigned long long beyond = bins[2 * ((size_t)K * (size_t)nseq + (size_t)s)];
        if (beyond) atomicAdd(&tot[K], beyond);
    }
}
