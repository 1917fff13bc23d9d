// k_covboot.h - the bootstrap of the coverage columns beside the depth of k_coverage.h and the gene bootstrap of k_geneboot.h
// (mc_set_coverage_bootstrap, mc_coverage_bootstrap): how much a breadth, and a detection call, hang on single reads.  mc_covboot.h states
// the rule and the entry; the kernels below follow it.  The difference array of k_coverage.h holds the whole sample's depth and not which
// read marked what, so k_covboot_collect keeps what a replicate needs of every assigned read - read id, gene, span: 12 bytes - in a device
// list; at read time the list is grouped by gene (k_covboot_scatter, into slices the count table's `reads` size), every replicate's covered
// residues are counted per gene (k_covboot_cover) and k_geneboot_summary makes the six doubles of that matrix.  No row reaches the host.
#pragma once
#include "k_ties.h"
#include "k_geneboot.h"
#include "mc_covboot.h"

struct McCbLen {                                                    // the residues of a gene, from the index's (or the fold's) offsets
    const uint32_t *off;
    __device__ __forceinline__ uint32_t operator()(int32_t s) const { return off[s + 1] - off[s]; }
};

// The shape of k_geneboot_collect: one thread per read, the one at its first row, walks the read's rows (mc_cb_read: k_abundance_cov's
// walk with the span kept, a further copy of it - whoever edits one edits all) and puts the read's entry into the list (mc_boot_put,
// k_geneboot.h).  map: the ids of a class run's batch, or a null perm: the row's query is the id (one kernel for both: it is new, no
// fixed-length run's instructions change with it).
// Launched behind the tie bootstrap's kernel on the same rows where they lie (mc_abund_launch, mc_abund.h) - behind the fold, in gene space.
__global__ void __launch_bounds__(256) k_covboot_collect(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, const uint32_t *__restrict__ off,
                                                         McCbEntry *list, unsigned long long capacity, unsigned long long *cur, McIdMap map)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    McCbEntry mine = {0u, 0u, 1, 0};
    if (i < nrows && (i == 0 || rows[i - 1].query != rows[i].query)) {   // one thread per read: the one at its first row
        McTiesPass pass; pass.A = A;
        const McCbLen len = {off};
        hit = mc_cb_read(pass, len, rows, nrows, i, nseq, mc_cb_id(map.perm, map.base, rows[i].query), &mine);
    }
    mc_boot_put(hit, mine, list, capacity, cur);
}

// Grouping by gene (mc_boot_scatter, k_geneboot.h), into slices the count table's `reads` size
__global__ void __launch_bounds__(256) k_covboot_scatter(const McCbEntry *__restrict__ list, long long n, int32_t nseq, uint32_t *cursor, const int32_t *__restrict__ idx,
                                                         McCbEntry *sorted)
{
    mc_boot_scatter(list, n, nseq, cursor, idx, sorted);
}

// The hot kernel.  A 2-D grid of (genes with reads) x (replicate tiles of MC_GB_LANES), one wave per block; a lane owns one replicate (its
// key in registers), as in k_bootstrap and k_geneboot_sums.  The wave walks the gene's slice of the grouped list: the entry is the same
// for the whole wave (a uniform address), and the next entry's load flies under this entry's mixing.  Every lane tests "present", and ONE
// ballot is the 64 replicates' presence mask M of the entry.  The lanes then OR M into the words s .. e of an LDS array - one 64-bit word
// per residue of the window, bit j = the tile's replicate j covers it; lane j takes the words s + j, s + j + 64, ..: consecutive 8-byte
// words, no two lanes of a half-wave on one bank - with an LDS atomic OR: no value comes back, and ORs commute.  At the window's end lane j
// counts the words whose bit j is set, over the touched range lo .. hi only: every lane reads the same word, a broadcast.  A gene longer
// than MC_CB_WINDOW residues is covered window by window, every pass clipping the spans (mc_cb_clip).  mat[g][b] is written as a 64-bit
// counter, so that k_geneboot_summary runs on it unchanged; det[g] (or null), zeroed by the caller, gets the popcount of a ballot of
// cov >= need per tile.  An entry whose gene is not this block's (a slot the scatter left out) covers nothing; mc_cb_clip keeps every
// word inside the window whatever an entry holds.
__global__ void __launch_bounds__(MC_GB_LANES) k_covboot_cover(const McCbEntry *__restrict__ sorted, const McCbGene *__restrict__ genes, int32_t B, uint64_t seed,
                                                               unsigned long long *mat, unsigned long long *det)
{
    __shared__ unsigned long long word[MC_CB_WINDOW];
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    const McCbGene G = genes[g];
    const long long b = (long long)blockIdx.y * MC_GB_LANES + lane;
    const uint64_t key = mc_boot_key(seed, (uint64_t)b);
    uint32_t cov = 0;
    for (uint32_t w0 = 0; w0 < G.len; w0 += MC_CB_WINDOW) {
        const uint32_t wn = G.len - w0 < MC_CB_WINDOW ? G.len - w0 : MC_CB_WINDOW;
        for (uint32_t p = lane; p < wn; p += MC_GB_LANES) word[p] = 0ull;
        __syncthreads();
        uint32_t lo = wn, hi = 0;                                   // the touched words: wave-uniform
        McCbEntry next = sorted[G.begin];
        for (uint32_t i = 0; i < G.n; i++) {
            const McCbEntry e = next;
            next = sorted[G.begin + (i + 1 < G.n ? i + 1 : i)];
            const unsigned long long M = __ballot(b < B && mc_cb_present(key, e.q));
            uint32_t a, z;
            if (!M || e.gene != g || !mc_cb_clip(e, w0, wn, &a, &z)) continue;   // (wave-uniform)
            for (uint32_t p = a + lane; p <= z; p += MC_GB_LANES) atomicOr(&word[p], M);
            lo = a < lo ? a : lo; hi = z + 1 > hi ? z + 1 : hi;
        }
        __syncthreads();
        for (uint32_t p = lo; p < hi; p++) cov += (uint32_t)((word[p] >> lane) & 1ull);
        __syncthreads();
    }
    if (b < B) mat[(size_t)g * (size_t)B + (size_t)b] = (unsigned long long)cov;
    if (det && G.need) {
        const unsigned long long D = __ballot(b < B && cov >= G.need);
        if (lane == 0 && D) atomicAdd(&det[g], (unsigned long long)__popcll(D));
    }
}
