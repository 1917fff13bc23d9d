// k_ties.h - a tie accounting beside the read counts of k_abundance.h (mc_set_ties): k_abundance.h gives a read to the FIRST of the
// rows that share its highest bit score, and among near-identical sequences (alleles, variants, families) most reads tie - in the
// reference binary's own m8 of the example reads 57 of 251, across up to 6 subjects.  These counters say, per gene, how many of its
// reads were its alone, how many it could have had, and what an even split gives it.
#pragma once
#include "k_abundance.h"
#include "mc_ties.h"

// ---- THE STATEMENT (tests/ties_restated.py restates it; mc_ties.h walks it; the kernel below launches the walk) --------------------
// Which reads count: passing rows are as mc_abund_passes defines them, under the cut-offs of mc_set_abundance.  T is the highest bits
// among a read's passing rows.  A read that k_abundance.h does not assign adds nothing here either: a read with no passing row, and a
// read whose first-rule best row (the first passing row with bits == T) has a subject outside 0 .. nseq - 1.
// The tied set of a read: the DISTINCT subjects in 0 .. nseq - 1 that have a passing row with bits == T - exact double equality on the
// row's own field; row order does not matter, the tied rows need not be adjacent, and a subject that ties twice is in the set once.
// k is the size of the tied set, 1 <= k <= 500.  A tied subject's REPRESENTATIVE ROW is its first passing row with bits == T in the
// read's row order; the FIRST TIED SUBJECT is that of the first passing row with bits == T - the subject k_abundance assigns the read to.
// Counters, all 64-bit integers, exact and independent of batches, ranges, launch geometry and the order of the atomics:
//     candidates[s]     reads whose tied set contains s
//     unique[s]         reads whose tied set is {s}
//     share[s]          fixed point in units of 2^-32: a read adds floor(2^32 / k) to every tied subject, and the remainder
//                       2^32 - k * floor(2^32 / k) to the first tied subject as well
//     ambiguous         reads with k > 1
//     group_ambiguous   reads whose tied set spans more than one group           (only with a group map group_of[nseq])
//     group_unique[g]   reads whose whole tied set lies in group g               (only with a group map)
// Depth, with coverage on: a second difference array, laid out as k_coverage.h lays out the first.  The representative row of EVERY
// tied subject marks its span sstart .. send, under the same guard against spans outside the gene.  covered_any, spanned_any and
// max_depth_any per gene are what k_coverage_scan makes of that array; the scan reads tab[2 s] as "this gene has reads", and the table
// below holds candidates[s] in that slot.
// Invariants (reads, assigned: the counters of k_abundance.h over the same reads):
//     sum(share) = assigned x 2^32                  sum(unique) + ambiguous = assigned
//     unique[s] <= reads[s] <= candidates[s]        sum(candidates) = the sum of k over the reads
//     sum(group_unique) + group_ambiguous = assigned        group_unique[g] >= the sum of unique[s] over the s in g
//     depth <= any-depth at every residue
//
// ---- Layout -------------------------------------------------------------------------------------------------------------------
// tab: (nseq + 1) x 2 counters, the shape of k_abundance's table: [s] = candidates, unique of subject s; [nseq] = ambiguous,
// group_ambiguous.  share: nseq counters.  group_unique: ngroups counters.  diff_any: nres + nseq slots (k_coverage.h, "Layout"), or
// null while coverage is off.  The three counter arrays are ONE buffer; where each begins and how large it is: mc_tie_share_at,
// mc_tie_group_at, mc_tie_slots in mc_abund.h - the only other place that knows these numbers.

// the device's sink of mc_ties_read: plain vector atomics
struct McTiesDev {
    unsigned long long *tab, *shr, *gu;
    const uint32_t *off; uint32_t *diff;
    __device__ __forceinline__ bool marks() const { return diff != nullptr; }
    __device__ __forceinline__ void cand(int32_t s) { atomicAdd(&tab[2 * (size_t)s], 1ull); }
    __device__ __forceinline__ void uniq(int32_t s) { atomicAdd(&tab[2 * (size_t)s + 1], 1ull); }
    __device__ __forceinline__ void share(int32_t s, unsigned long long v) { atomicAdd(&shr[s], v); }
    __device__ __forceinline__ void group_uniq(int32_t g) { atomicAdd(&gu[g], 1ull); }
    __device__ __forceinline__ void mark(int32_t s, int32_t a, int32_t b)
    {
        const uint32_t base = off[s] + (uint32_t)s, len = off[s + 1] - off[s];   // (the gene's first slot and its residues)
        if (a >= 0 && a <= b && (uint32_t)b < len) {                  // (k_abundance_cov's guard: any other span marks nothing)
            atomicAdd(&diff[base + (uint32_t)a], 1u);
            atomicAdd(&diff[base + (uint32_t)b + 1u], 0xFFFFFFFFu);
        }
    }
};

struct McTiesPass {
    McAbundPars A;
    __device__ __forceinline__ bool operator()(const McRow &r) const { return mc_abund_passes(A, r.frame, r.alnlen, r.bits, r.loge); }   // (McRow::frame carries the identities)
};

// The shape of k_abundance: the thread at a read's first row walks the read's rows (mc_ties_read: up to three walks, and a duplicate
// check among the tied rows only); ambiguous and group_ambiguous are summed over the workgroup first, one atomic each per workgroup
// that has any.  Launched behind the counting kernel on the same rows (mc_abund_launch, mc_abund.h), it reads them where they lie.
// group_of / group_unique: null without a group map.  off / diff_any: null while coverage is off.
__global__ void __launch_bounds__(256) k_ties(McAbundPars A, const McRow *__restrict__ rows, uint32_t nrows, int32_t nseq, unsigned long long *tab, unsigned long long *share,
                                              const int32_t *__restrict__ group_of, unsigned long long *group_unique, const uint32_t *__restrict__ off, uint32_t *diff_any)
{
    __shared__ uint32_t wcnt[2][4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool amb = false, across = false;
    if (i < nrows && (i == 0 || rows[i - 1].query != rows[i].query)) {   // one thread per read: the one at its first row
        McTiesPass pass; pass.A = A;
        McTiesDev sink; sink.tab = tab; sink.shr = share; sink.gu = group_unique; sink.off = off; sink.diff = diff_any;
        const McTieRead t = mc_ties_read(pass, rows, nrows, i, nseq, group_of, sink);
        amb = t.k > 1; across = t.across;
    }
    const unsigned long long ma = __ballot(amb), mg = __ballot(across);
    if (mc_lane() == 0) { wcnt[0][threadIdx.x >> 6] = (uint32_t)__popcll(ma); wcnt[1][threadIdx.x >> 6] = (uint32_t)__popcll(mg); }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t tot = wcnt[threadIdx.x][0] + wcnt[threadIdx.x][1] + wcnt[threadIdx.x][2] + wcnt[threadIdx.x][3];
        if (tot) atomicAdd(&tab[2 * (size_t)nseq + threadIdx.x], (unsigned long long)tot);
    }
}
