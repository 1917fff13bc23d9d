// tests/emul/groupboot.cpp - the rules of the group bootstrap that need no GPU (csrc/mc_groupboot.h: mc_grb_add, mc_grb_thread_sum - the
// very text the kernels of k_groupboot.h run -, mc_grb_values and mc_grb_group, the rule in serial form, and mc_grb_plan, the host plan)
// compiled by g++ and run on the CPU: a stand-alone program that includes the library's header and copies none of it.
//   groupboot run IN OUT      (files of sections: order_io.h; tests/test_groupboot_host.py writes IN and reads OUT)
// IN:  three int32 (nseq, B, ngroups), the genes' replicate counts (uint64, [s * B + b]), scale (B doubles), group_of (int32 per gene),
//      gene_kb (double per gene) and the genes' reads (uint64 per gene: what the count table holds).
// OUT: y (ngroups x B doubles), C (ngroups x B uint64), the six doubles of every group (ngroups x 6); then the plan: ngrp (int32), gidx
//      (int32 per group), start (uint32, ngrp + 1), member (uint32) and kb (double) of the genes with reads.
// Every array lives in a std::vector of its exact size: -fsanitize=address sees an access behind any of them.
#include "../../microbecensus_amd/csrc/mc_groupboot.h"

#include "order_io.h"

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: groupboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t nmeta, nc, nsc, ngo, nkb, nrd;
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const unsigned long long *c = in.take<unsigned long long>(&nc);
    const double *sc = in.take<double>(&nsc);
    const int32_t *gof = in.take<int32_t>(&ngo);
    const double *gkb = in.take<double>(&nkb);
    const unsigned long long *rd = in.take<unsigned long long>(&nrd);
    if (nmeta != 3 || meta[0] < 1 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 1 || meta[2] > meta[0] || nc != (size_t)meta[0] * (size_t)meta[1] || nsc != (size_t)meta[1] ||
        ngo != (size_t)meta[0] || nkb != ngo || nrd != ngo) { fprintf(stderr, "input: malformed\n"); return 2; }
    const int nseq = meta[0], B = meta[1], ngroups = meta[2];
    for (int s = 0; s < nseq; s++)
        if (gof[s] < 0 || gof[s] >= ngroups || !(gkb[s] > 0.0 && gkb[s] <= 1.7976931348623157e308)) { fprintf(stderr, "input: gene %d: its group or its gene_kb\n", s); return 2; }
    const std::vector<unsigned long long> counts(c, c + nc);
    const std::vector<double> scale(sc, sc + B), kb(gkb, gkb + nseq);
    const std::vector<int> group_of(gof, gof + nseq);
    std::vector<double> y, stats;
    std::vector<unsigned long long> C;
    for (int G = 0; G < ngroups; G++) {
        std::vector<int> member;
        for (int s = 0; s < nseq; s++) if (group_of[(size_t)s] == G) member.push_back(s);
        std::vector<double> yG((size_t)B), x((size_t)B), part(MC_GB_THREADS), o(MC_GB_NOUT);
        std::vector<unsigned long long> CG((size_t)B);
        mc_grb_values(counts.data(), member.data(), (int)member.size(), kb.data(), scale.data(), B, yG.data(), CG.data());
        mc_grb_group(yG.data(), scale.data(), B, x.data(), part.data(), o.data());
        y.insert(y.end(), yG.begin(), yG.end()); C.insert(C.end(), CG.begin(), CG.end()); stats.insert(stats.end(), o.begin(), o.end());
    }
    out.put(y); out.put(C); out.put(stats);
    // the plan, from the compact indices mc_gb_plan would give: every array of exactly the size the header promises to stay within
    std::vector<int> idx((size_t)nseq), gidx((size_t)ngroups);
    int ng = 0;
    for (int s = 0; s < nseq; s++) idx[(size_t)s] = rd[s] ? ng++ : -1;
    int live = 0;
    for (int G = 0; G < ngroups; G++) { bool any = false; for (int s = 0; s < nseq; s++) any = any || (group_of[(size_t)s] == G && rd[s]); live += any ? 1 : 0; }
    std::vector<unsigned> start((size_t)ngroups + 1), member((size_t)ng);
    std::vector<double> mkb((size_t)ng);
    const int32_t ngrp = mc_grb_plan(idx.data(), nseq, group_of.data(), ngroups, kb.data(), gidx.data(), start.data(), member.data(), mkb.data());
    if (ngrp != live) { fprintf(stderr, "mc_grb_plan: %d groups with reads, %d counted\n", ngrp, live); return 1; }
    start.resize((size_t)ngrp + 1);
    out.put(&ngrp, 1); out.put(gidx); out.put(start); out.put(member); out.put(mkb);
    sections_write(argv[3], out);
    return 0;
}
