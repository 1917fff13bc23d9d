// k_geneboot.h - the bootstrap of the per-gene read counts beside the counts of k_abundance.h (mc_set_gene_bootstrap, mc_gene_bootstrap):
// how sure an RPKG is.  mc_geneboot.h states the rule; the kernels below follow it.  The counts stream range by range and keep no row, so
// k_geneboot_collect keeps the one thing a replicate needs of an assigned read - (read id, gene), 8 bytes - in a device list; at read time
// the list is grouped by gene (k_geneboot_scatter, into slices the count table's `reads` size), every replicate's weights are summed per
// gene (k_geneboot_sums) and every gene's B values are sorted and summed up (k_geneboot_summary).  No row reaches the host.
#pragma once
#include "k_abundance.h"
#include "mc_geneboot.h"

// Slot reservation at the end of a collect kernel of 256 threads, k_abundance's `assigned` idiom: ballot, per-wave popcount, ONE atomic on
// the cursor per workgroup that has any hit; a lane writes `mine` at the workgroup's base + its rank among the workgroup's hits.  cur[0]:
// the cursor - it counts every hit, fitting or not; cur[1]: dropped.  A hit whose slot is not below capacity adds 1 to dropped and writes
// nothing: nothing is ever written behind the list.  Every thread of the workgroup calls it (two barriers).  The entry goes by value: by
// reference the kernels come out longer.
template <class E> __device__ __forceinline__ void mc_boot_put(bool hit, const E mine, E *list, unsigned long long capacity, unsigned long long *cur)
{
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long base;
    const unsigned long long m = __ballot(hit);
    const int lane = mc_lane(), w = (int)(threadIdx.x >> 6);
    if (lane == 0) wcnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        base = tot ? atomicAdd(&cur[0], (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    if (!hit) return;
    uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; k++) rank += wcnt[k];
    const unsigned long long slot = base + rank;
    if (slot < capacity) list[slot] = mine;
    else atomicAdd(&cur[1], 1ull);
}

// The shape of k_abundance, and a walk of its own over a read's rows (a fourth copy of k_abundance's walk: whoever edits one edits all;
// DESIGN.md 13.3 has why the walks are separate kernels - and this way the counting kernels are the same instructions with the switch on
// or off), and the read's entry into the list (mc_boot_put).  Launched behind the counting kernel, k_ties and k_curve on the same rows
// (mc_abund_launch, mc_abund.h).
__global__ void __launch_bounds__(256) k_geneboot_collect(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, McGbEntry *list, unsigned long long capacity,
                                                          unsigned long long *cur)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    McGbEntry mine = {0u, 0u};
    if (i < nrows) {
        const int q = rows[i].query;
        if (i == 0 || rows[i - 1].query != q) {                      // one thread per read: the one at its first row
            double bbits = 0.0; int bsub = -1;
            for (uint32_t k = i; k < nrows && rows[k].query == q; k++) {
                const McRow r = rows[k];
                if (!mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge)) continue;   // (McRow::frame carries the identities)
                if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; }
            }
            if (bsub >= 0 && bsub < nseq) { hit = true; mine.q = (uint32_t)q; mine.gene = (uint32_t)bsub; }
        }
    }
    mc_boot_put(hit, mine, list, capacity, cur);
}

// The id of a read whose rows carry a position `query` of a sorted batch and not the read's id (a class run, mc_set_abundance_classes):
// base + perm[query], perm the row index of every sorted position (the class prologue's), base the batch's first read id.  The sum
// is taken in 64 bits and lies below 2^31 (mc_search_classes).
struct McIdMap { const uint32_t *perm; int64_t base; };

// k_geneboot_collect for the pieces of a class run: launched INSTEAD of it while the owner holds an id map (mc_abund_launch), the same
// walk, the same slots, and the entry's id taken through `map`.  A second kernel and not a parameter of the first (a fifth copy of the
// walk: whoever edits one edits all): the kernel of the fixed-length runs stays the instructions it was - and no body shared by the two
// came out as the instructions they are (DESIGN.md 13.13 has the forms tried).
__global__ void __launch_bounds__(256) k_geneboot_collect_mapped(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, McGbEntry *list, unsigned long long capacity,
                                                                 unsigned long long *cur, McIdMap map)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    McGbEntry mine = {0u, 0u};
    if (i < nrows) {
        const int q = rows[i].query;
        if (i == 0 || rows[i - 1].query != q) {                      // one thread per read: the one at its first row
            double bbits = 0.0; int bsub = -1;
            for (uint32_t k = i; k < nrows && rows[k].query == q; k++) {
                const McRow r = rows[k];
                if (!mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge)) continue;   // (McRow::frame carries the identities)
                if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; }
            }
            if (bsub >= 0 && bsub < nseq) { hit = true; mine.q = (uint32_t)(map.base + (int64_t)map.perm[q]); mine.gene = (uint32_t)bsub; }
        }
    }
    mc_boot_put(hit, mine, list, capacity, cur);
}

// Grouping by gene, for every entry type (q, gene, ..): cursor[s] starts at the first slot of gene s in the grouped list - the exclusive
// scan of the pair table's first column (the count table's `reads`, the tie table's `candidates`) - and idx[s] is the gene's compact index
// among the genes with entries.  One thread per entry takes the next slot of its gene; the order within a gene is whatever the atomics
// give, and free: the sums are integers, covering is an OR.  n entries in both lists; a slot not below n, or a gene the table has no
// entry of (the table and the list disagree - the caller has checked that they do not), is not written.
template <class E> __device__ __forceinline__ void mc_boot_scatter(const E *__restrict__ list, long long n, int32_t nseq, uint32_t *cursor, const int32_t *__restrict__ idx, E *sorted)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const E e = list[i];
    if (e.gene >= (uint32_t)nseq || idx[e.gene] < 0) return;
    const uint32_t pos = atomicAdd(&cursor[e.gene], 1u);
    if ((long long)pos < n) { E o = e; o.gene = (uint32_t)idx[e.gene]; sorted[pos] = o; }
}
__global__ void __launch_bounds__(256) k_geneboot_scatter(const McGbEntry *__restrict__ list, long long n, int32_t nseq, uint32_t *cursor, const int32_t *__restrict__ idx,
                                                          McGbEntry *sorted)
{
    mc_boot_scatter(list, n, nseq, cursor, idx, sorted);
}

// The shape of k_bootstrap: a 2-D grid of entry tiles x replicate tiles of MC_GB_LANES, one wave per block.  A lane owns one replicate
// (its key in registers) and walks the tile, per_tile consecutive entries of the grouped list (mc_gb_per_tile: a function of (n, B)
// alone); the entry is the same for the whole wave (a uniform address: scalar loads), and the next entry's load flies under this entry's
// mixing.  The lane keeps its sum in a register and flushes it with one 64-bit atomicAdd into mat[gene][b] whenever the tile's gene
// changes, and at the tile's end - the 64 lanes of a flush touch 512 consecutive bytes.  A gene that holds every read is spread over all
// the tiles.  mat: ngenes x B counters, zeroed by the caller; an entry whose gene is not below ngenes (a slot the scatter left out) adds
// nothing.
// (k_tieboot_sums is this text on the other entry with one factor more: no body shared by the two came out as the instructions they
// are - DESIGN.md 13.13 has the forms tried - so whoever edits one edits both.)
__global__ void __launch_bounds__(MC_GB_LANES) k_geneboot_sums(const McGbEntry *__restrict__ sorted, long long n, long long per_tile, int32_t B, uint64_t seed, uint32_t ngenes, unsigned long long *mat)
{
    const int lane = (int)threadIdx.x;
    const long long b = (long long)blockIdx.y * MC_GB_LANES + lane;
    const long long lo = (long long)blockIdx.x * per_tile, hi = lo + per_tile < n ? lo + per_tile : n;
    if (lo >= hi) return;
    const uint64_t key = mc_boot_key(seed, (uint64_t)b);
    McGbEntry next = sorted[lo];
    uint32_t g = next.gene;
    unsigned long long acc = 0ull;
    for (long long i = lo; i < hi; i++) {
        const McGbEntry e = next;
        next = sorted[i + 1 < hi ? i + 1 : i];
        if (e.gene != g) {
            if (b < B && acc && g < ngenes) atomicAdd(&mat[(size_t)g * (size_t)B + (size_t)b], acc);
            acc = 0ull; g = e.gene;
        }
        acc += (unsigned long long)mc_boot_weight(key, (uint64_t)e.q);
    }
    if (b < B && acc && g < ngenes) atomicAdd(&mat[(size_t)g * (size_t)B + (size_t)b], acc);
}

// One workgroup per gene with reads: row g of mat, the gene's B replicate counts.  The values v[b] go to LDS, an unused replicate as
// +inf, padded with +inf to the next power of two P; sum and m2 are added in the stated order (mc_gb_thread_sum, then the halving tree
// level by level with a barrier between the levels); a bitonic network sorts the P values ascending - the m used ones come first - and
// thread 0 writes the six doubles to out[6 g ..].  m: the number of used replicates, counted by the caller with mc_gb_used.
__global__ void __launch_bounds__(MC_GB_THREADS) k_geneboot_summary(const unsigned long long *__restrict__ mat, const double *__restrict__ scale, int32_t B, int32_t m, double *out)
{
    __shared__ double x[MC_GB_MAXB];
    __shared__ double part[MC_GB_THREADS];
    const int t = (int)threadIdx.x;
    const unsigned long long *c = mat + (size_t)blockIdx.x * (size_t)B;
    double *o = out + (size_t)MC_GB_NOUT * blockIdx.x;
    if (m <= 0) { if (t < MC_GB_NOUT) o[t] = mc_gb_nan(); return; }
    int P = 1;
    while (P < B) P <<= 1;
    for (int b = t; b < P; b += MC_GB_THREADS) x[b] = b < B && mc_gb_used(scale[b]) ? mc_gb_value(c[b], scale[b]) : __builtin_inf();
    part[t] = mc_gb_thread_sum(c, scale, B, t, 0.0, false);
    __syncthreads();
    for (int h = MC_GB_THREADS / 2; h >= 1; h >>= 1) { if (t < h) part[t] += part[t + h]; __syncthreads(); }
    const double sum = part[0];
    __syncthreads();
    part[t] = mc_gb_thread_sum(c, scale, B, t, sum / (double)m, true);
    __syncthreads();
    for (int h = MC_GB_THREADS / 2; h >= 1; h >>= 1) { if (t < h) part[t] += part[t + h]; __syncthreads(); }
    const double m2 = part[0];
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += MC_GB_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const double a = x[i], z = x[l];
                    if ((i & k) == 0 ? a > z : a < z) { x[i] = z; x[l] = a; }
                }
            }
            __syncthreads();
        }
    if (t == 0) {
        o[MC_GB_SUM] = sum; o[MC_GB_M2] = m2;
        for (int k = MC_GB_LO; k <= MC_GB_HI1; k++) o[k] = x[mc_gb_index(m, k)];
    }
}
