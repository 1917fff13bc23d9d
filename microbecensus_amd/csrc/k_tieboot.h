// k_tieboot.h - the bootstrap of the tie shares beside the tie accounting of k_ties.h and the gene bootstrap of k_geneboot.h
// (mc_set_tie_bootstrap, mc_tie_bootstrap): how sure an rpkg_shared is.  mc_tieboot.h states the rule and the entry; the kernels below
// follow it.  The tied sets exist only in the rows of a range while it is on the device, so k_tieboot_collect keeps what a replicate needs
// of every (read, tied subject) - read id, gene, share: 12 bytes - in a device list; at read time the list is grouped by gene
// (k_tieboot_scatter, into slices the tie table's `candidates` size), every replicate's weighted shares are summed per gene
// (k_tieboot_sums) and k_geneboot_summary makes the six doubles of that matrix.  No row reaches the host.
#pragma once
#include "k_ties.h"
#include "k_geneboot.h"
#include "mc_tieboot.h"

// The shape of k_ties: one thread per read, the one at the read's first row, and TWO calls of mc_ties_read (mc_tieboot.h: mc_tb_count,
// mc_tb_write) with the slot reservation between them: the first learns k, the read's entries; the ks of the workgroup's 256 threads are
// scanned in LDS (Hillis-Steele over two buffers, a barrier per step: 8 steps; k <= 500, so a workgroup's total is below 2^17); ONE atomic
// on the cursor per workgroup that has any entry reserves them all, and the second call writes the read's entries at the workgroup's
// base + the exclusive scan of its k.  cur[0]: the cursor - it counts every entry, fitting or not; cur[1]: dropped.  An entry whose slot
// is not below capacity adds 1 to dropped and writes nothing: nothing is ever written behind the list.  map: the ids of a class run's
// batch, or a null perm: the row's query is the id (one kernel for both: it is new, no fixed-length run's instructions change with it).
// Launched behind k_geneboot_collect on the same rows where they lie (mc_abund_launch, mc_abund.h) - behind the fold, in gene space.
__global__ void __launch_bounds__(256) k_tieboot_collect(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, McTbEntry *list, unsigned long long capacity,
                                                         unsigned long long *cur, McIdMap map)
{
    __shared__ uint32_t scan[2][256];
    __shared__ unsigned long long base;
    const uint32_t t = threadIdx.x, i = blockIdx.x * 256u + t;
    const bool head = i < nrows && (i == 0 || rows[i - 1].query != rows[i].query);   // one thread per read: the one at its first row
    McTiesPass pass; pass.A = A;
    const uint32_t k = head ? mc_tb_count(pass, rows, nrows, i, nseq) : 0u;
    scan[0][t] = k;
    __syncthreads();
    int from = 0;
    for (uint32_t d = 1; d < 256u; d <<= 1) {                        // inclusive scan: after the step of distance d, [t] holds the sum of the 2 d values ending at t
        scan[from ^ 1][t] = scan[from][t] + (t >= d ? scan[from][t - d] : 0u);
        from ^= 1;
        __syncthreads();
    }
    if (t == 255) { const uint32_t tot = scan[from][255]; base = tot ? atomicAdd(&cur[0], (unsigned long long)tot) : 0ull; }
    __syncthreads();
    if (!k) return;
    const unsigned long long slot = base + (unsigned long long)(scan[from][t] - k);
    const uint32_t dropped = mc_tb_write(pass, rows, nrows, i, nseq, mc_tb_id(map.perm, map.base, rows[i].query), list, capacity, slot);
    if (dropped) atomicAdd(&cur[1], (unsigned long long)dropped);
}

// Grouping by gene (mc_boot_scatter, k_geneboot.h), into slices the tie table's `candidates` size
__global__ void __launch_bounds__(256) k_tieboot_scatter(const McTbEntry *__restrict__ list, long long n, int32_t nseq, uint32_t *cursor, const int32_t *__restrict__ idx,
                                                         McTbEntry *sorted)
{
    mc_boot_scatter(list, n, nseq, cursor, idx, sorted);
}

// k_geneboot_sums on the other entry (its text with one factor more: whoever edits one edits both - no body shared by the two came out as
// the instructions they are): the same 2-D grid of entry tiles x replicate tiles of MC_GB_LANES, one wave per block,
// per_tile = mc_gb_per_tile of the ENTRY count; a lane owns one replicate and adds weight x share of every entry of the tile into a
// register, flushed with one 64-bit atomicAdd into mat[gene][b] whenever the tile's gene changes, and at the tile's end.  mat: ngenes x B
// counters in units of 2^-32, zeroed by the caller; an entry whose gene is not below ngenes (a slot the scatter left out) adds nothing.
// No sum can wrap (mc_tieboot.h).
__global__ void __launch_bounds__(MC_GB_LANES) k_tieboot_sums(const McTbEntry *__restrict__ sorted, long long n, long long per_tile, int32_t B, uint64_t seed, uint32_t ngenes, unsigned long long *mat)
{
    const int lane = (int)threadIdx.x;
    const long long b = (long long)blockIdx.y * MC_GB_LANES + lane;
    const long long lo = (long long)blockIdx.x * per_tile, hi = lo + per_tile < n ? lo + per_tile : n;
    if (lo >= hi) return;
    const uint64_t key = mc_boot_key(seed, (uint64_t)b);
    McTbEntry next = sorted[lo];
    uint32_t g = next.gene;
    unsigned long long acc = 0ull;
    for (long long i = lo; i < hi; i++) {
        const McTbEntry e = next;
        next = sorted[i + 1 < hi ? i + 1 : i];
        if (e.gene != g) {
            if (b < B && acc && g < ngenes) atomicAdd(&mat[(size_t)g * (size_t)B + (size_t)b], acc);
            acc = 0ull; g = e.gene;
        }
        acc += (unsigned long long)mc_boot_weight(key, (uint64_t)e.q) * mc_tb_share(e);
    }
    if (b < B && acc && g < ngenes) atomicAdd(&mat[(size_t)g * (size_t)B + (size_t)b], acc);
}
