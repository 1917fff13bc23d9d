// mc_geneboot.h - the bootstrap of the per-gene read counts (mc_set_gene_bootstrap, mc_gene_bootstrap): what a replicate counts, what is
// made of a gene's B replicate values, and in which order the floating-point sums are added.  Same conventions as mc_boot.h and
// mc_curve.h: host and device code alike, no HIP include of its own - k_geneboot.h runs it on the device, g++ compiles the very same text
// into tests/emul/geneboot.cpp, and tests/geneboot_restated.py restates it in numpy.
//
// ---- THE STATEMENT ----------------------------------------------------------------------------------------------------------------
// A read's ASSIGNMENT is exactly k_abundance.h's best row: the same four cut-offs, the highest bits, the first row on a tie; its subject
// must lie in 0 .. nseq - 1.  A read's global id q is mc_row.query, 0 <= q < 2^31.
// The REPLICATE COUNT c[b][s], b in 0 .. B - 1, 1 <= B <= MC_GB_MAXB, is the sum of mc_boot_weight(mc_boot_key(seed, b), q) over the reads
// q assigned to gene s (mc_boot.h): an exact 64-bit integer that does not depend on ranges, batches, launch geometry or the order of the
// atomics.  Replicate b under one seed is the same resample of the same reads as replicate b of mc_bootstrap.
// scale[b] is a double per replicate; replicate b is USED when scale[b] is finite and > 0 (mc_gb_used); m is the number of used ones.
// For a used b the gene's value is v[b] = (double)c[b][s] * scale[b], one rounding (mc_gb_value).
// The six doubles of a gene (MC_GB_SUM .. MC_GB_HI1):
//     sum = the sum of v[b] over the used b            m2 = the sum of (v[b] - sum / m)^2 over the used b
//     x[lo], x[lo + 1], x[hi], x[hi + 1] of the ascending-sorted used values x, lo = floor((m - 1) * 0.025), hi = floor((m - 1) * 0.975),
//     the + 1 index clamped to m - 1 (mc_gb_index)
// With m == 0 all six are NaN.  A gene without reads has c == 0 in every replicate: sum = m2 = 0 and zeros for the four (m > 0).
// THE ADDITION ORDER of sum and m2 is a function of B alone (mc_gb_thread_sum, mc_gb_tree): "thread" t of MC_GB_THREADS adds its
// b = t, t + MC_GB_THREADS, ... ascending, skipping the unused ones, into a partial that starts at 0.0; then a halving tree adds the
// partials: for h = MC_GB_THREADS / 2, .., 1: part[t] += part[t + h] for every t < h.  m2 squares d = v[b] - mean as d * d and adds it:
// a multiplication and an addition, never fused (the library, the harnesses and the emulation are built with -ffp-contract=off).  The
// kernel, the g++ emulation and the numpy restatement follow this order, so the results are compared bit for bit.
#pragma once
#include "mc_core.h"
#include "mc_boot.h"

#define MC_GB_MAXB 4096                                             // one gene's values fit a workgroup's LDS for the sort: 32 KiB
#define MC_GB_THREADS 256
#define MC_GB_LANES 64                                              // replicates per tile of k_geneboot_sums: a lane each
#define MC_GB_TILES 2048                                            // entry tiles x replicate tiles aimed at (mc_gb_per_tile)
enum { MC_GB_SUM = 0, MC_GB_M2, MC_GB_LO, MC_GB_LO1, MC_GB_HI, MC_GB_HI1, MC_GB_NOUT };

// an entry of the device list: one assigned read.  In the collected list `gene` is the subject; in the grouped list the compact index
// of the gene among those with reads
struct McGbEntry { uint32_t q, gene; };

MC_HD bool mc_gb_used(double s) { return s > 0.0 && s <= 1.7976931348623157e308; }   // (finite and > 0; NaN compares false)
MC_HD double mc_gb_value(unsigned long long c, double s) { return (double)c * s; }
MC_HD double mc_gb_nan() { return __builtin_nan(""); }

// The index of an order statistic among m >= 1 sorted values: which: MC_GB_LO .. MC_GB_HI1
MC_HD int mc_gb_index(int m, int which)
{
    const int at = (int)((double)(m - 1) * (which == MC_GB_LO || which == MC_GB_LO1 ? 0.025 : 0.975));   // (>= 0: the cast is the floor)
    const int i = at + (which == MC_GB_LO1 || which == MC_GB_HI1 ? 1 : 0);
    return i < m - 1 ? i : m - 1;
}

// what thread t adds: the values of its used replicates (squares false), or their squared distances from mean (squares true)
MC_HD double mc_gb_thread_sum(const unsigned long long *c, const double *scale, int B, int t, double mean, bool squares)
{
    double p = 0.0;
    for (int b = t; b < B; b += MC_GB_THREADS) {
        if (!mc_gb_used(scale[b])) continue;
        const double v = mc_gb_value(c[b], scale[b]);
        if (squares) { const double d = v - mean; p += d * d; }
        else p += v;
    }
    return p;
}

// the halving tree in serial form (the kernel runs level h with the threads t < h and a barrier between the levels); the sum ends in part[0]
MC_HD void mc_gb_tree(double *part)
{
    for (int h = MC_GB_THREADS / 2; h >= 1; h >>= 1)
        for (int t = 0; t < h; t++) part[t] += part[t + h];
}

// The whole rule for ONE gene in serial form (k_geneboot_summary does the same with a workgroup: the sort is a bitonic network in LDS,
// which gives the same sorted values as any sort).  c: the gene's B replicate counts; x: B doubles of scratch; part: MC_GB_THREADS.
MC_HD void mc_gb_gene(const unsigned long long *c, const double *scale, int B, double *x, double *part, double *out)
{
    int m = 0;
    for (int b = 0; b < B; b++) if (mc_gb_used(scale[b])) x[m++] = mc_gb_value(c[b], scale[b]);
    if (m == 0) { for (int k = 0; k < MC_GB_NOUT; k++) out[k] = mc_gb_nan(); return; }
    for (int t = 0; t < MC_GB_THREADS; t++) part[t] = mc_gb_thread_sum(c, scale, B, t, 0.0, false);
    mc_gb_tree(part);
    out[MC_GB_SUM] = part[0];
    const double mean = out[MC_GB_SUM] / (double)m;
    for (int t = 0; t < MC_GB_THREADS; t++) part[t] = mc_gb_thread_sum(c, scale, B, t, mean, true);
    mc_gb_tree(part);
    out[MC_GB_M2] = part[0];
    for (int i = 1; i < m; i++) {                                   // (insertion sort: m <= 4096, and only the emulation runs this)
        const double v = x[i]; int j = i;
        while (j > 0 && x[j - 1] > v) { x[j] = x[j - 1]; j--; }
        x[j] = v;
    }
    for (int k = MC_GB_LO; k <= MC_GB_HI1; k++) out[k] = x[mc_gb_index(m, k)];
}

// The tiling of k_geneboot_sums, a function of (entries, B) alone: how many consecutive entries of the grouped list one wave walks.
// About MC_GB_TILES waves in all, never fewer than 64 entries per tile; a gene that holds every read is spread over all the tiles.
MC_HD long long mc_gb_per_tile(long long n, int B)
{
    const long long nbt = (B + MC_GB_LANES - 1) / MC_GB_LANES, want = MC_GB_TILES / nbt > 0 ? MC_GB_TILES / nbt : 1;
    const long long per = (n + want - 1) / want;
    return per < 64 ? 64 : per;
}
