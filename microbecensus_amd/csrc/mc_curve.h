// mc_curve.h - the two rules of the rarefaction curve (k_curve.h states them) that need no GPU: which bin a read id or a residue's first
// id falls into, and what the scan makes of one gene's bins.  Same conventions as mc_core.h and mc_ties.h: MC_HD code, no HIP include
// of its own, so that g++ compiles the very same text into tests/emul/curve.cpp and runs it on the CPU against tests/curve_restated.py.
#pragma once
#include "mc_core.h"

#define MC_CURVE_MAXK 64                                            // one wave: lane k holds point k (k_curve_scan)
#define MC_CURVE_NEVER 0xFFFFFFFFu                                  // first[] of a residue no read has covered: no id reaches it (ids are int32)

// b(q): the number of k with n[k] <= q, in 0 .. K.  n ascends (repeats allowed); K == 0 gives 0.  A binary search: the first k with
// n[k] > q.
MC_HD int mc_curve_bin(const unsigned long long *n, int K, unsigned long long q)
{
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (n[mid] <= q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the bin of a residue whose lowest covering id is f: it is covered at point k iff f < n[k] iff this bin is <= k.  A residue that was
// never covered is covered at NO point, however large the points: bin K.
MC_HD int mc_curve_first_bin(const unsigned long long *n, int K, uint32_t f)
{
    return f == MC_CURVE_NEVER ? K : mc_curve_bin(n, K, (unsigned long long)f);
}

// The scan's rule for ONE gene, in serial form (k_curve_scan does the same with a wave: lane k holds point k, the histogram lies in LDS,
// the running sums are wave scans).  bin_reads / bin_aligned: the gene's K + 1 bins; first: its len residues, or null with coverage off;
// hist: K + 1 counters of scratch.  Out: reads_k, aligned_k and (with first) covered_k, K values each.
MC_HD void mc_curve_gene(const unsigned long long *n, int K, const unsigned long long *bin_reads, const unsigned long long *bin_aligned, const uint32_t *first, uint32_t len,
                         uint32_t *hist, unsigned long long *reads_k, unsigned long long *aligned_k, unsigned long long *covered_k)
{
    for (int b = 0; b <= K; b++) hist[b] = 0;
    for (uint32_t p = 0; first && p < len; p++) hist[mc_curve_first_bin(n, K, first[p])]++;
    unsigned long long r = 0, a = 0, c = 0;
    for (int k = 0; k < K; k++) {
        r += bin_reads[k]; a += bin_aligned[k]; c += hist[k];
        reads_k[k] = r; aligned_k[k] = a;
        if (covered_k) covered_k[k] = first ? c : 0ull;
    }
}
