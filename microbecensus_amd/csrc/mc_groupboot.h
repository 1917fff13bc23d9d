// mc_groupboot.h - the bootstrap of the GROUPS table (mc_group_bootstrap): what a replicate of a group is, what is made of a group's B
// replicate values, and in which order the floating-point sums are added.  Same conventions as mc_geneboot.h, on whose statement it
// stands: host and device code alike, no HIP include of its own - k_groupboot.h runs it on the device, g++ compiles the very same text
// into tests/emul/groupboot.cpp, and tests/groupboot_restated.py restates it in numpy.
//
// ---- THE STATEMENT ----------------------------------------------------------------------------------------------------------------
// c[b][s] are the gene bootstrap's replicate counts (mc_geneboot.h), group_of[s] in 0 .. ngroups - 1 the group of every gene s,
// gene_kb[s] a finite double > 0 (the front end passes 3 x length_aa / 1000), scale[b] a double per replicate, USED or not by
// mc_gb_used; m is the number of used replicates.
// The GROUP REPLICATE COUNT C[b][G] is the sum of c[b][s] over the members s of G: an exact 64-bit integer, of every b.
// The GROUP REPLICATE VALUE y[b][G] of a used b starts at 0.0, and the members are taken in ASCENDING GENE INDEX s; each adds
//     mc_gb_value(c[b][s], scale[b]) / gene_kb[s]
// (mc_grb_add): one multiplication, one division and one addition per member, never fused.  The division comes BEFORE the addition: a
// group's value is a sum of RPKGs, and no function of the group's count.  A member without reads has c == 0 in every replicate and adds
// +0.0 / gene_kb = +0.0 to a y that is never -0.0 (it starts at +0.0 and only non-negative terms are added): skipping such a member
// changes no bit.  The kernel only sees the genes with reads and skips the others; the serial form and the restatement may add them.
// Of an UNUSED b y[b][G] is 0.0 - nothing is added - and nothing below reads it.
// The six doubles of a group (MC_GB_SUM .. MC_GB_HI1) are made from its used y[b][G] exactly as mc_geneboot.h makes a gene's from its
// v[b]: the same partition of b over MC_GB_THREADS partials, the same halving tree (mc_gb_tree), d * d unfused, the same mc_gb_index.
// With m == 0 all six are NaN; a group without reads has y == 0 in every replicate: zeros for all six with m > 0.
// The host (abundance.group_boot_columns) makes rpkg_boot_se = sqrt(m2 / (m - 1)) and the interval from the order statistics; there is
// no division by a length there: it is inside y.
#pragma once
#include <cstddef>
#include "mc_geneboot.h"

// one member's step of the walk: y + (double)c * s / kb, three roundings
MC_HD double mc_grb_add(double y, unsigned long long c, double s, double kb)
{
    const double v = mc_gb_value(c, s);
    const double r = v / kb;
    return y + r;
}

// mc_gb_thread_sum on an array of values: what thread t adds of y[b], b = t, t + MC_GB_THREADS, ... ascending, the unused ones skipped
MC_HD double mc_grb_thread_sum(const double *y, const double *scale, int B, int t, double mean, bool squares)
{
    double p = 0.0;
    for (int b = t; b < B; b += MC_GB_THREADS) {
        if (!mc_gb_used(scale[b])) continue;
        const double v = y[b];
        if (squares) { const double d = v - mean; p += d * d; }
        else p += v;
    }
    return p;
}

// The replicate values and counts of ONE group in serial form (k_groupboot_values gives a lane to every b).  c: the replicate counts
// of all genes at [s * B + b]; member: the group's n members, ascending; y: B doubles; C: B counts, or null
MC_HD void mc_grb_values(const unsigned long long *c, const int *member, int n, const double *gene_kb, const double *scale, int B, double *y, unsigned long long *C)
{
    for (int b = 0; b < B; b++) {
        double v = 0.0; unsigned long long tot = 0ull;
        const bool use = mc_gb_used(scale[b]);
        for (int k = 0; k < n; k++) {
            const unsigned long long cb = c[(size_t)member[k] * (size_t)B + (size_t)b];
            tot += cb;
            if (use) v = mc_grb_add(v, cb, scale[b], gene_kb[member[k]]);
        }
        y[b] = v;
        if (C) C[b] = tot;
    }
}

// mc_gb_gene on an array of values: the whole rule for ONE group in serial form (k_groupboot_summary does the same with a workgroup).
// y: the group's B replicate values; x: B doubles of scratch; part: MC_GB_THREADS
MC_HD void mc_grb_group(const double *y, const double *scale, int B, double *x, double *part, double *out)
{
    int m = 0;
    for (int b = 0; b < B; b++) if (mc_gb_used(scale[b])) x[m++] = y[b];
    if (m == 0) { for (int k = 0; k < MC_GB_NOUT; k++) out[k] = mc_gb_nan(); return; }
    for (int t = 0; t < MC_GB_THREADS; t++) part[t] = mc_grb_thread_sum(y, scale, B, t, 0.0, false);
    mc_gb_tree(part);
    out[MC_GB_SUM] = part[0];
    const double mean = out[MC_GB_SUM] / (double)m;
    for (int t = 0; t < MC_GB_THREADS; t++) part[t] = mc_grb_thread_sum(y, scale, B, t, mean, true);
    mc_gb_tree(part);
    out[MC_GB_M2] = part[0];
    for (int i = 1; i < m; i++) {                                   // (insertion sort: m <= 4096, and only the emulation runs this)
        const double v = x[i]; int j = i;
        while (j > 0 && x[j - 1] > v) { x[j] = x[j - 1]; j--; }
        x[j] = v;
    }
    for (int k = MC_GB_LO; k <= MC_GB_HI1; k++) out[k] = x[mc_gb_index(m, k)];
}

// The host plan of a read, beside mc_gb_plan and from the same compact indices idx[s] (>= 0: a gene with reads): gidx[G]: the compact
// index of a group with reads - ascending with G - or -1; start: the CSR of the groups with reads over `member`, ngrp + 1 offsets;
// member: the compact indices of the genes with reads, group by group and ascending gene index within a group; kb: their gene_kb.
// start holds up to ngroups + 1 values, member and kb as many as genes have reads.  Returns ngrp, the groups with reads.
static inline int mc_grb_plan(const int *idx, int nseq, const int *group_of, int ngroups, const double *gene_kb, int *gidx, unsigned *start, unsigned *member, double *kb)
{
    for (int G = 0; G < ngroups; G++) gidx[G] = 0;
    for (int s = 0; s < nseq; s++) if (idx[s] >= 0) gidx[group_of[s]]++;              // (members with reads, for now)
    int ngrp = 0; unsigned at = 0;
    for (int G = 0; G < ngroups; G++) {
        const int n = gidx[G];
        if (!n) { gidx[G] = -1; continue; }
        gidx[G] = ngrp; start[ngrp++] = at; at += (unsigned)n;
    }
    start[ngrp] = at;
    for (int s = 0; s < nseq; s++) {                                                  // ascending s: every group's slice fills in gene order
        if (idx[s] < 0) continue;
        const unsigned slot = start[gidx[group_of[s]]]++;
        member[slot] = (unsigned)idx[s]; kb[slot] = gene_kb[s];
    }
    for (int g = ngrp; g > 0; g--) start[g] = start[g - 1];                           // (every start has moved to its group's end)
    start[0] = 0;
    return ngrp;
}
