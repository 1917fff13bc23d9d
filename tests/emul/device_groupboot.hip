// tests/emul/device_groupboot.hip - the group bootstrap's kernels (csrc/k_groupboot.h: k_groupboot_values and k_groupboot_summary, behind
// the gene bootstrap's read on the replicate counts it left on the device) on synthetic rows and group maps built to reach their edges: a
// stand-alone program that includes the library's headers - it compiles the text the library compiles and copies none of it - and links
// neither the library nor the reader.
//   device_groupboot run IN OUT      (files of sections: order_io.h; tests/test_gpu_groupboot_units.py writes IN and reads OUT)
// IN:  device_geneboot.hip's six sections - the cut-offs (McAbundPars), four int32 (nseq, B, capacity, launch: must be 1), the rows (McRow),
//      the launches (uint32), scale (B doubles), the seed (uint64) - then group_of (int32 per gene), two int32 (ngroups, counts_first:
//      whether the owner's first call asks for the counts) and gene_kb (double per gene).
// OUT: 0 status (int32: genes with reads, groups with reads, m, then the owner's three return values: the group read, the gene read, the
//      group read behind it); raw buffers on mc_geneboot_launch's mat: 1 val, 2 cnt (groups with reads x B), 3 the six doubles of the
//      groups with reads, 4 val and 5 the six doubles of a second launch that asks for NO counts; 6 - 13 the 16 elements of padding behind
//      val, cnt, the output, the CSR's offsets, its members, their gene_kb, mat and the scales; then McAbundance's own answers on the same
//      launches: 14 stats and 15 counts of its first call (ngroups x 6, ngroups x B or empty), 16 stats and 17 counts of the call behind a
//      gene bootstrap (which asks for the counts when the first did not), 18 three floats (the group reads' ms behind the first call and
//      behind the second, the gene reads' ms), 19 its error message.
// Every launch goes through mc_abund_launch, mc_geneboot_launch and mc_groupboot_launch (csrc/mc_abund.h), the functions the library
// launches through.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an error is printed
// and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_groupboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nrows, ncuts, nscale, nseed, ngo, nmeta2, nkb;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const double *scale = in.take<double>(&nscale);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    const int32_t *group_of = in.take<int32_t>(&ngo);
    const int32_t *meta2 = in.take<int32_t>(&nmeta2);
    const double *gene_kb = in.take<double>(&nkb);
    // the input is a legal state: a database within the engine's limits, B and a capacity as the ABI takes them, rows by ascending read id,
    // a map and lengths as mc_group_bootstrap takes them
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[0] > 32767 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 1 || meta[2] > (1 << 24) || meta[3] != 1 || nscale != (size_t)meta[1] || nseed != 1) {
        fprintf(stderr, "input: cut-offs, sizes, scale or seed malformed\n"); return 2;
    }
    if (nrows > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows) { fprintf(stderr, "input: %zu rows, %zu launches\n", nrows, ncuts); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++)
            if (rows[i].query < 0 || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a negative read id, or read ids descend within a launch\n", i); return 2; }
    }
    const int32_t nseq = meta[0], B = meta[1];
    if (nmeta2 != 2 || meta2[0] < 1 || meta2[0] > nseq || ngo != (size_t)nseq || nkb != (size_t)nseq) { fprintf(stderr, "input: the map, ngroups or gene_kb malformed\n"); return 2; }
    const int32_t ngroups = meta2[0];
    const bool counts_first = meta2[1] != 0;
    for (int32_t s = 0; s < nseq; s++)
        if (group_of[s] < 0 || group_of[s] >= ngroups || !(gene_kb[s] > 0.0 && gene_kb[s] <= 1.7976931348623157e308)) { fprintf(stderr, "input: gene %d: its group or its gene_kb\n", s); return 2; }
    const size_t ns = (size_t)nseq, cap = (size_t)meta[2], ngr = (size_t)ngroups;

    // the rows through the counting kernel and k_geneboot_collect, then mat through the gene bootstrap's read: device_geneboot.hip's path
    Dev<McRow> d_rows(rows, nrows);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_cur(2);
    Dev<McGbEntry> d_list(cap, 0xEE);
    McEvent own[9];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs Bf = {nseq, nullptr, d_tab, nullptr, nullptr, nullptr, nullptr};
    const McGeneBootBufs G = {d_list, (unsigned long long)cap, d_cur, own[3]};
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (mc_abund_launch(*A, Bf, d_rows + at, (uint32_t)(cuts[c] - at), nullptr, ev, nullptr, &G)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    const std::vector<unsigned long long> tab = d_tab.host(), cur = d_cur.host();
    std::vector<uint32_t> gstart(ns); std::vector<int32_t> idx(ns);
    unsigned long long total = 0;
    const int32_t ng = mc_gb_plan(tab.data(), nseq, gstart.data(), idx.data(), &total);
    if (cur[1] != 0 || cur[0] != total || cur[0] > cap) { fprintf(stderr, "input: %llu entries of %llu assigned reads fit the list of %zu\n", cur[0], total, cap); return 2; }
    const size_t n = (size_t)cur[0], gneed = (size_t)ng * (size_t)B;
    int32_t m = 0;
    for (int32_t b = 0; b < B; b++) m += mc_gb_used(scale[b]) ? 1 : 0;
    Dev<uint32_t> d_cursor(gstart.data(), ns);
    Dev<int32_t> d_idx(idx.data(), ns);
    Dev<McGbEntry> d_sorted(n, 0xEE);
    Dev<unsigned long long> d_mat(gneed);
    Dev<double> d_scale(scale, (size_t)B), d_gout((size_t)MC_GB_NOUT * (size_t)ng, 0xFF);
    const McGeneBootRead GR = {nseq, ng, (long long)n, d_list, d_cursor, d_idx, d_sorted, d_mat, d_scale, B, m, seed[0], d_gout};
    const hipEvent_t rev[2] = {own[4], own[5]};
    if (mc_geneboot_launch(GR, nullptr, rev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();

    // the group read on raw buffers, each of its exact size with padding behind it: with the counts, then without
    std::vector<int32_t> gidx(ngr); std::vector<uint32_t> start(ngr + 1), member((size_t)ng); std::vector<double> kb((size_t)ng);
    const int32_t ngrp = mc_grb_plan(idx.data(), nseq, group_of, ngroups, gene_kb, gidx.data(), start.data(), member.data(), kb.data());
    const size_t need = (size_t)ngrp * (size_t)B;
    Dev<uint32_t> d_start(start.data(), (size_t)ngrp + 1), d_member(member.data(), (size_t)ng);
    Dev<double> d_kb(kb.data(), (size_t)ng), d_val(need, 0xFF), d_val2(need, 0xFF), d_out((size_t)MC_GB_NOUT * (size_t)ngrp, 0xFF), d_out2((size_t)MC_GB_NOUT * (size_t)ngrp, 0xFF);
    Dev<unsigned long long> d_cnt(need, 0xEE);
    const hipEvent_t gev[3] = {own[6], own[7], own[8]};
    const McGroupBootRead R1 = {ng, ngrp, d_mat, d_start, d_member, d_kb, d_val, d_cnt, d_scale, B, m, d_out};
    if (mc_groupboot_launch(R1, nullptr, gev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    const McGroupBootRead R2 = {ng, ngrp, d_mat, d_start, d_member, d_kb, d_val2, nullptr, d_scale, B, m, d_out2};
    if (mc_groupboot_launch(R2, nullptr, gev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    int32_t status[6] = {ng, ngrp, m, 0, 0, 0};
    Sections body;
    body.put(d_val.host()); body.put(d_cnt.host()); body.put(d_out.host()); body.put(d_val2.host()); body.put(d_out2.host());
    body.put(d_val.pad()); body.put(d_cnt.pad()); body.put(d_out.pad()); body.put(d_start.pad()); body.put(d_member.pad()); body.put(d_kb.pad()); body.put(d_mat.pad()); body.put(d_scale.pad());

    // the owner's own path on the same launches: a group read that has to make mat, a gene read, a group read that may take mat over
    McAbundance ab;
    ab.bind(nseq, 0, nullptr);
    if (ab.set_counts(true, *A) || ab.set_gene_bootstrap((int64_t)cap)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (ab.launch(d_rows + at, (uint32_t)(cuts[c] - at), nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
        ab.range_done(0);
    }
    std::vector<int64_t> c1(counts_first ? ngr * (size_t)B : 0, -1), c2(counts_first ? 0 : ngr * (size_t)B, -1), dropped(1, -1);
    std::vector<double> s1(ngr * MC_GB_NOUT, -1.0), s2(ngr * MC_GB_NOUT, -1.0), gs(ns * MC_GB_NOUT, -1.0);
    float ms[3] = {0.f, 0.f, 0.f};
    g_err.clear();
    status[3] = ab.read_group_bootstrap(B, seed[0], scale, group_of, ngroups, gene_kb, counts_first ? c1.data() : nullptr, s1.data(), dropped.data());
    CK(hipDeviceSynchronize());
    ms[0] = ab.grp_ms;
    status[4] = ab.read_gene_bootstrap(B, seed[0], scale, nullptr, gs.data(), dropped.data());
    CK(hipDeviceSynchronize());
    status[5] = ab.read_group_bootstrap(B, seed[0], scale, group_of, ngroups, gene_kb, counts_first ? nullptr : c2.data(), s2.data(), dropped.data());
    CK(hipDeviceSynchronize());
    ms[1] = ab.grp_ms; ms[2] = ab.gread_ms;
    body.put(s1); body.put(c1); body.put(s2); body.put(c2); body.put(ms, 3); body.put(g_err.data(), g_err.size());
    out.put(status, 6);
    for (const std::vector<uint8_t> &b : body.s) out.put(b);
    sections_write(argv[3], out);
    return 0;
}
