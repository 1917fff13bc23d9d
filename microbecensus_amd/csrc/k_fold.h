// k_fold.h - the fold of a range's rows from the segments of long genes onto the genes (mc_set_gene_fold; mc_fold.h states the rule and
// holds the per-row functions this kernel runs).  Launched by McAbundance::launch (mc_abund.h) in front of mc_abund_launch, so the
// counting, coverage, tie, curve, bootstrap and class kernels behind it see gene space and stay the instructions they were.
#pragma once
#include "mc_hip_common.h"
#include "mc_fold.h"

// One thread per row: the row in (72 bytes, the compiler's wide loads), one 16-byte record of its segment (seg: nseq records, read-only -
// a lane's subject is its own, so the record comes through the vector path; the table of at most 512 KiB stays in L2), the row out into
// `out`, a buffer of the owner's - never in place: the rows of a range go to the host as the engine made them (m8, keep_rows), in a copy
// that runs beside this kernel.  The edge rows (mc_fold_edge) are summed over the workgroup first, k_abundance's idiom: a ballot per wave,
// one 64-bit atomic on edge[0] per workgroup that met any.  Memory-bound: 144 bytes per row, 0.3 GB per 1 M reads of two rows each.
__global__ void __launch_bounds__(256) k_fold(const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, const McFoldSeg *__restrict__ seg, McRow *__restrict__ out, unsigned long long *edge)
{
    __shared__ uint32_t wcnt[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool touch = false;
    if (i < nrows) {
        const McRow r = rows[i];
        touch = mc_fold_edge(r, nseq, seg);
        out[i] = mc_fold_row(r, nseq, seg);
    }
    const unsigned long long m = __ballot(touch);
    if (mc_lane() == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (tot) atomicAdd(edge, (unsigned long long)tot);
    }
}
