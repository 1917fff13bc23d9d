// k_identity.h - how similar the reads assigned to a gene are to the database's sequence (mc_set_identity): a histogram of the best rows'
// identities per gene and the sums of their matched, mismatched and gap-opening columns, on the rows of a range; the per-gene figures
// (min, lower median, max, the reads at or above up to eight levels) by a scan at read time.  mc_identity.h states the rule and the layout.
#pragma once
#include "k_abundance.h"
#include "mc_identity.h"

// A THIRD walk behind k_abundance / k_abundance_cov (k_abundance.h, k_coverage.h: the same loop, the same mc_abund_passes, the same tie
// rule, the same 0 <= subject < nseq - whoever edits one edits all), a kernel of its own so that those two keep their instructions
// (walks under one kernel compiled to other code and measured slower).  The thread at a read's first row walks the read's
// rows and issues one 32-bit atomic into hist[subject][bin] and three 64-bit atomics into sums[subject] - one 32-byte record, one line.
// tests/test_gpu_identity_units.py holds sum(hist[s]) to the count table of the counting kernel on the same rows.
// rows: the nrows final rows of a completed range, ascending read id.  hist: nseq x MC_ID_STRIDE counters; sums: nseq records.
__global__ void __launch_bounds__(256) k_identity(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, uint32_t *hist, McIdSums *sums)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nrows) return;
    const int q = rows[i].query;
    if (i != 0 && rows[i - 1].query == q) return;                    // one thread per read: the one at its first row
    double bbits = 0.0; int bsub = -1, baln = 0, bnm = 0, bmis = 0, bgap = 0;
    for (uint32_t k = i; k < nrows && rows[k].query == q; k++) {
        const McRow r = rows[k];
        if (!mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge)) continue;   // (McRow::frame carries the identities)
        if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; baln = r.alnlen; bnm = r.frame; bmis = r.mismatch; bgap = r.gapopen; }
    }
    if (bsub < 0 || bsub >= nseq) return;
    atomicAdd(&hist[(size_t)MC_ID_STRIDE * (size_t)bsub + (size_t)mc_id_bin(bnm, baln)], 1u);   // (mc_id_bin: 0 .. 100 whatever the row holds)
    McIdSums *g = sums + bsub;
    atomicAdd(&g->matched, (unsigned long long)(long long)bnm);
    atomicAdd(&g->mismatched, (unsigned long long)(long long)bmis);
    atomicAdd(&g->gap_opens, (unsigned long long)(long long)bgap);
}

// inclusive prefix sum over the 64 lanes of a wave (wrapping), without LDS: k_coverage.h's form
__device__ __forceinline__ uint32_t mc_id_wave_scan(uint32_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

// Scan, at read time: one wave per gene, four genes per workgroup.  Lane l holds the gene's bins l and 64 + l (two coalesced words; the 27
// slots behind bin 100 are zero and inside the gene's stride).  Two wave prefix sums give every bin's cumulative count: c0 of bin l, c1 of
// bin 64 + l; n = c1 of lane 63.  min and max from the ballots of the non-empty bins; the lower median is the first bin whose cumulative
// count reaches (n - 1) / 2 + 1, the lowest set bit of a ballot; ge[j] = n - the cumulative count of bin level[j] - 1, fetched by a shuffle.
// out: nout = 3 + nlevels values per gene (min, median, max, ge[0 ..]) from out[nout * s]; a gene without reads writes MC_ID_NONE three times
// and zeros.  level: nlevels (0 .. MC_ID_LEVELS) checked levels on the device.  hist is only read: ranges may go on counting after a read.
__global__ void __launch_bounds__(256) k_identity_scan(const uint32_t *__restrict__ hist, int32_t nseq, const int32_t *__restrict__ level, int32_t nlevels, long long *out)
{
    const int lane = mc_lane();
    const int32_t s = (int32_t)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (s >= nseq) return;                                           // (wave-uniform)
    const uint32_t *h = hist + (size_t)MC_ID_STRIDE * (size_t)s;
    const uint32_t h0 = h[lane], h1 = h[64 + lane];
    const uint32_t c0 = mc_id_wave_scan(h0, lane);
    const uint32_t c1 = mc_id_wave_scan(h1, lane) + (uint32_t)__shfl((int)c0, 63, 64);
    const uint32_t n = (uint32_t)__shfl((int)c1, 63, 64);
    const unsigned long long m0 = __ballot(h0 != 0), m1 = __ballot(h1 != 0);
    const uint32_t need = n ? (n - 1) / 2 + 1 : 1;
    const unsigned long long r0 = __ballot(c0 >= need), r1 = __ballot(c1 >= need);
    // the level of lane j < nlevels; below: the cumulative count of the bin under it (every lane shuffles, lanes without a level read lane 0)
    const int lv = lane < nlevels ? level[lane] : 0;
    const int src = lv > 0 ? lv - 1 : 0;
    const uint32_t b0 = (uint32_t)__shfl((int)c0, src & 63, 64), b1 = (uint32_t)__shfl((int)c1, src & 63, 64);
    const uint32_t below = lv > 0 ? (src < 64 ? b0 : b1) : 0u;
    long long *o = out + (size_t)(3 + nlevels) * (size_t)s;
    if (lane == 0) {
        o[0] = m0 ? (long long)__builtin_ctzll(m0) : m1 ? 64ll + __builtin_ctzll(m1) : (long long)MC_ID_NONE;
        o[1] = !n ? (long long)MC_ID_NONE : r0 ? (long long)__builtin_ctzll(r0) : 64ll + __builtin_ctzll(r1);
        o[2] = m1 ? 127ll - __builtin_clzll(m1) : m0 ? 63ll - __builtin_clzll(m0) : (long long)MC_ID_NONE;
    }
    if (lane < nlevels) o[3 + lane] = (long long)(n - below);
}
