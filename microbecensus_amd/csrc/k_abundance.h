// k_abundance.h - per-gene read counts for RPKG (the reference README's "Normalization" section: RPKG = reads mapped to gene /
// gene length in kb / genome equivalents), summed on the device over the m8 rows of a range (mc_set_abundance).
#pragma once
#include "mc_hip_common.h"

// ---- THE STATEMENT (tests/abundance_restated.py restates it; the kernel below follows it) ---------------------------------------
// Cut-offs: min_ident (an integer percent, 0 .. 100), min_aln (residues, >= 0), min_bits, max_loge (doubles, not NaN).
// A row of a read PASSES when all four of these hold, as exact integer or double comparisons:
//     100 * nmatch >= min_ident * alnlen        alnlen >= min_aln        bits >= min_bits        loge <= max_loge
// (nmatch: the identical columns of the alignment, mc_row.nmatch; identity in percent is 100 * nmatch / alnlen).
// The read's BEST ROW is the passing row with the highest bits; on a tie the first in RAPsearch2's order within the read - the rule
// of classify_reads (microbe_census.py:450: `best < score`, strict) and of k_grid_classify.
// A read with a best row adds 1 to reads[subject], alnlen to aligned[subject] (the best row's subject and alignment length) and 1
// to the scalar `assigned`.  The scalar `searched` counts every read of a range that completed, with or without rows.
// All counters are 64-bit integers: the result is exact and does not depend on launch geometry, batches, ranges or the order of
// the atomics.
struct McAbundPars { int32_t min_ident, min_aln; double min_bits, max_loge; };

MC_HD bool mc_abund_passes(const McAbundPars &A, int nmatch, int alnlen, double bits, double loge)
{
    return 100 * nmatch >= A.min_ident * alnlen && alnlen >= A.min_aln && bits >= A.min_bits && loge <= A.max_loge;
}

// The shape of k_grid_classify: the thread at a read's first row walks the read's rows (at most 500, 1.9 on shotgun reads) and issues
// two 64-bit atomics into tab[subject][0 .. 1] (one 16-byte pair: one line); the reads it assigned are summed over the workgroup
// first, one atomic on tab[nseq][0] per workgroup that assigned any - a device-scope atomic on ONE address runs at the memory
// side (mc_block_alloc).  32,767 x 16 bytes does not fit an LDS histogram; the hits of a range are spread over the subjects.
// rows: the nrows final rows of a completed range (c.d_rows), ascending read id.  tab: (nseq + 1) x 2 counters.
// (k_coverage.h holds a SECOND COPY of this walk, k_abundance_cov, which also marks the best row's span: whoever edits one edits both.
// One walk under both kernels compiled to other code and measured about 1 % slower on five of six legs: DESIGN.md 13.3.  Both are
// launched by mc_abund_launch, mc_abund.h, which also owns the table.)
__global__ void __launch_bounds__(256) k_abundance(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, unsigned long long *tab)
{
    __shared__ uint32_t wcnt[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < nrows) {
        const int q = rows[i].query;
        if (i == 0 || rows[i - 1].query != q) {                      // one thread per read: the one at its first row
            double bbits = 0.0; int bsub = -1, baln = 0;
            for (uint32_t k = i; k < nrows && rows[k].query == q; k++) {
                const McRow r = rows[k];
                if (!mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge)) continue;   // (McRow::frame carries the identities)
                if (bsub < 0 || bbits < r.bits) { bbits = r.bits; bsub = r.subject; baln = r.alnlen; }
            }
            if (bsub >= 0 && bsub < nseq) {
                hit = true;
                atomicAdd(&tab[2 * (size_t)bsub], 1ull);
                atomicAdd(&tab[2 * (size_t)bsub + 1], (unsigned long long)baln);
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
