// tests/emul/device_geneboot.hip - the gene bootstrap's kernels (csrc/k_geneboot.h: k_geneboot_collect, behind the counting kernel on a
// range's rows, and at read time k_geneboot_scatter, k_geneboot_sums and k_geneboot_summary) on synthetic rows built to reach their edges:
// a stand-alone program that includes the library's headers - it compiles the text the library compiles and copies none of it - and links
// neither the library nor the reader.
//   device_geneboot run IN OUT      (files of sections: order_io.h; tests/test_gpu_geneboot_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), four int32 (nseq, B, capacity, launch: 0 hands the launches NO list), the rows (McRow), the launches
//      (uint32: the row index behind each launch's last row, ascending, the last one == the number of rows; rows ascend by read id WITHIN
//      a launch), scale (B doubles) and the seed (uint64).
// OUT: 0 status (int32: launch, the owner's return value, genes with reads, whether the read ran); 1 tab ((nseq + 1) x 2 counters of the
//      counting kernel); 2 the list (capacity entries, 0xEE bytes where nothing was written); 3 the cursor and dropped; 4 - 6 the 16
//      elements of padding behind those three; then, when the read ran (the list was handed over and nothing was dropped): 7 the grouped
//      list, 8 mat (genes with reads x B), 9 the six doubles of the genes with reads, 10 - 15 the padding behind the grouped list, mat, the
//      output, the genes' cursors, their compact indices and the scales; then McAbundance's own answer on the same launches: 16 dropped,
//      17 counts (nseq x B), 18 stats (nseq x 6), 19 its error message.
// Every launch goes through mc_abund_launch and the read through mc_geneboot_launch (csrc/mc_abund.h), the functions the library launches
// through.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an error is printed and ends
// the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_geneboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nrows, ncuts, nscale, nseed;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const double *scale = in.take<double>(&nscale);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    // the input is a legal state: a database within the engine's limits, B and a capacity as the ABI takes them, rows by ascending read id
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[0] > 32767 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 1 || meta[2] > (1 << 24) || nscale != (size_t)meta[1] || nseed != 1) {
        fprintf(stderr, "input: cut-offs, sizes, scale or seed malformed\n"); return 2;
    }
    if (nrows > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows) { fprintf(stderr, "input: %zu rows, %zu launches\n", nrows, ncuts); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++)
            if (rows[i].query < 0 || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a negative read id, or read ids descend within a launch\n", i); return 2; }
    }
    const int32_t nseq = meta[0], B = meta[1];
    const size_t ns = (size_t)nseq, cap = (size_t)meta[2];
    const bool launch = meta[3] != 0;

    Dev<McRow> d_rows(rows, nrows);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_cur(2);
    Dev<McGbEntry> d_list(cap, 0xEE);
    McEvent own[6];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs Bf = {nseq, nullptr, d_tab, nullptr, nullptr, nullptr, nullptr};
    const McGeneBootBufs G = {d_list, (unsigned long long)cap, d_cur, own[3]};
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (mc_abund_launch(*A, Bf, d_rows + at, (uint32_t)(cuts[c] - at), nullptr, ev, nullptr, launch ? &G : nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    const std::vector<unsigned long long> tab = d_tab.host(), cur = d_cur.host();
    std::vector<uint32_t> start(ns); std::vector<int32_t> idx(ns);
    unsigned long long total = 0;
    const int32_t ng = mc_gb_plan(tab.data(), nseq, start.data(), idx.data(), &total);
    const bool read = launch && cur[1] == 0 && cur[0] == total && cur[0] <= cap;       // (what McAbundance::read_gene_bootstrap asks before it reads)
    int32_t status[4] = {launch ? 1 : 0, 0, ng, read ? 1 : 0};
    Sections body;
    body.put(tab); body.put(d_list.host()); body.put(cur);
    body.put(d_tab.pad()); body.put(d_list.pad()); body.put(d_cur.pad());
    if (read) {
        const size_t n = (size_t)cur[0], need = (size_t)ng * (size_t)B;
        int32_t m = 0;
        for (int32_t b = 0; b < B; b++) m += mc_gb_used(scale[b]) ? 1 : 0;
        Dev<uint32_t> d_cursor(start.data(), ns);
        Dev<int32_t> d_idx(idx.data(), ns);
        Dev<McGbEntry> d_sorted(n, 0xEE);
        Dev<unsigned long long> d_mat(need);
        Dev<double> d_scale(scale, (size_t)B), d_out((size_t)MC_GB_NOUT * (size_t)ng, 0xFF);
        const McGeneBootRead R = {nseq, ng, (long long)n, d_list, d_cursor, d_idx, d_sorted, d_mat, d_scale, B, m, seed[0], d_out};
        const hipEvent_t rev[2] = {own[4], own[5]};
        if (mc_geneboot_launch(R, nullptr, rev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
        body.put(d_sorted.host()); body.put(d_mat.host()); body.put(d_out.host());
        body.put(d_sorted.pad()); body.put(d_mat.pad()); body.put(d_out.pad()); body.put(d_cursor.pad()); body.put(d_idx.pad()); body.put(d_scale.pad());
    }
    if (launch) {
        // the owner's own path on the same launches: the switches, the launch, the read and its refusal
        McAbundance ab;
        ab.bind(nseq, 0, nullptr);
        if (ab.set_counts(true, *A) || ab.set_gene_bootstrap((int64_t)cap)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
            if (ab.launch(d_rows + at, (uint32_t)(cuts[c] - at), nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
            CK_LAUNCH();
            ab.range_done(0);
        }
        std::vector<int64_t> counts(ns * (size_t)B, -1), dropped(1, -1);
        std::vector<double> stats(ns * MC_GB_NOUT, -1.0);
        g_err.clear();
        status[1] = ab.read_gene_bootstrap(B, seed[0], scale, counts.data(), stats.data(), dropped.data());
        CK(hipDeviceSynchronize());
        if (!read) { body.put(dropped.data(), 0); for (int k = 0; k < 8; k++) body.put(dropped.data(), 0); }   // (sections 7 - 15 stay empty)
        body.put(dropped); body.put(counts); body.put(stats); body.put(g_err.data(), g_err.size());
    }
    out.put(status, 4);
    for (const std::vector<uint8_t> &b : body.s) out.put(b);
    sections_write(argv[3], out);
    return 0;
}
