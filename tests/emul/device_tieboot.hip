// tests/emul/device_tieboot.hip - the tie bootstrap's kernels (csrc/k_tieboot.h: k_tieboot_collect, behind the counting kernel, k_ties and
// k_geneboot_collect on a range's rows, and at read time k_tieboot_scatter, k_tieboot_sums and the gene bootstrap's k_geneboot_summary) on
// synthetic rows built to reach their edges: a stand-alone program that includes the library's headers - it compiles the text the library
// compiles and copies none of it - and links neither the library nor the reader.
//   device_tieboot run IN OUT      (files of sections: order_io.h; tests/test_gpu_tieboot_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), four int32 (nseq, B, capacity - 0 .. 2^24 -, launch: 0 hands the launches NO tie list), the rows (McRow),
//      the launches (uint32: the row index behind each launch's last row, ascending, the last one == the number of rows; rows ascend by
//      read id WITHIN a launch), scale (B doubles), the seed (uint64), perm (uint32; none: a row's query is the read's id; else every
//      query is an index into it) and base (int64).
// OUT: 0 status (int32: launch, the owner's return value, genes with candidates, whether the read ran); 1 the count table ((nseq + 1) x 2);
//      2 the tie table (mc_tie_slots(nseq, 0) counters: candidates and unique, ambiguous, the shares); 3 the list (capacity entries, 0xEE
//      bytes where nothing was written); 4 the cursor and dropped; 5 - 8 the 16 elements of padding behind those four; 9 - 17: when the read
//      ran (the list was handed over and nothing was dropped; empty otherwise) 9 the grouped list, 10 mat (genes with candidates x B), 11 the
//      six doubles of those genes, 12 - 17 the padding behind the grouped list, mat, the output, the genes' cursors, their compact indices and
//      the scales; then, when a list was handed over and the capacity is not 0, McAbundance's own answer on the same launches: 18 dropped,
//      19 shares (nseq x B), 20 stats (nseq x 6), 21 its error message.
// Every launch goes through mc_abund_launch and the read through mc_tieboot_launch (csrc/mc_abund.h), the functions the library launches
// through.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an error is printed and ends
// the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_tieboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nrows, ncuts, nscale, nseed, nperm, nbase;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const double *scale = in.take<double>(&nscale);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    const uint32_t *perm = in.take<uint32_t>(&nperm);
    const int64_t *base = in.take<int64_t>(&nbase);
    // the input is a legal state: a database within the engine's limits, B and a capacity as the ABI takes them, rows by ascending read id,
    // every id below 2^31
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[0] > 32767 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 0 || meta[2] > (1 << 24) || nscale != (size_t)meta[1] || nseed != 1 ||
        nbase != 1 || base[0] < 0) {
        fprintf(stderr, "input: cut-offs, sizes, scale, seed or base malformed\n"); return 2;
    }
    if (nrows < 1 || nrows > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows) { fprintf(stderr, "input: %zu rows, %zu launches\n", nrows, ncuts); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++) {
            if (rows[i].query < 0 || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a negative read id, or read ids descend within a launch\n", i); return 2; }
            if (nperm && ((size_t)rows[i].query >= nperm || base[0] + (int64_t)perm[rows[i].query] > 0x7fffffffll)) { fprintf(stderr, "input: row %zu: no id in the map\n", i); return 2; }
        }
    }
    const int32_t nseq = meta[0], B = meta[1];
    const size_t ns = (size_t)nseq, cap = (size_t)meta[2];
    const bool launch = meta[3] != 0;

    Dev<McRow> d_rows(rows, nrows);
    Dev<uint32_t> d_perm(perm, nperm);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_ties(mc_tie_slots(ns, 0)), d_cur(2);
    Dev<McTbEntry> d_list(cap, 0xEE);
    McEvent own[8];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs Bf = {nseq, nullptr, d_tab, nullptr, d_ties, nullptr, nullptr};
    const McTieBootBufs T = {d_list, (unsigned long long)cap, d_cur, own[3]};
    Dev<unsigned long long> d_cls(MC_AC_SLOTS);
    const McIdMap map = {d_perm, base[0]};
    const McClassRide R = {map, d_cls, 1, 0, 0ull, own[4]};          // (a ride of one class: the id map of the launches, as a class run hands it over)
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (mc_abund_launch(*A, Bf, d_rows + at, (uint32_t)(cuts[c] - at), nullptr, ev, nullptr, nullptr, nperm ? &R : nullptr, launch ? &T : nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    const std::vector<unsigned long long> tab = d_tab.host(), ties = d_ties.host(), cur = d_cur.host();
    std::vector<uint32_t> start(ns); std::vector<int32_t> idx(ns);
    unsigned long long total = 0;
    const int32_t ng = mc_gb_plan(ties.data(), nseq, start.data(), idx.data(), &total);      // (the tie table's pairs: candidates size the slices)
    const bool read = launch && cur[1] == 0 && cur[0] == total && cur[0] <= cap;            // (what McAbundance::read_tie_bootstrap asks before it reads)
    int32_t status[4] = {launch ? 1 : 0, 0, ng, read ? 1 : 0};
    Sections body;
    body.put(tab); body.put(ties); body.put(d_list.host()); body.put(cur);
    body.put(d_tab.pad()); body.put(d_ties.pad()); body.put(d_list.pad()); body.put(d_cur.pad());
    if (read) {
        const size_t n = (size_t)cur[0], need = (size_t)ng * (size_t)B;
        std::vector<double> s32((size_t)B);
        int32_t m = 0;
        for (int32_t b = 0; b < B; b++) { s32[(size_t)b] = mc_tb_scale(scale[b]); m += mc_gb_used(s32[(size_t)b]) ? 1 : 0; }
        Dev<uint32_t> d_cursor(start.data(), ns);
        Dev<int32_t> d_idx(idx.data(), ns);
        Dev<McTbEntry> d_sorted(n, 0xEE);
        Dev<unsigned long long> d_mat(need);
        Dev<double> d_scale(s32.data(), (size_t)B), d_out((size_t)MC_GB_NOUT * (size_t)ng, 0xFF);
        const McTieBootRead Rd = {nseq, ng, (long long)n, d_list, d_cursor, d_idx, d_sorted, d_mat, d_scale, B, m, seed[0], d_out};
        const hipEvent_t rev[2] = {own[5], own[6]};
        if (mc_tieboot_launch(Rd, nullptr, rev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
        body.put(d_sorted.host()); body.put(d_mat.host()); body.put(d_out.host());
        body.put(d_sorted.pad()); body.put(d_mat.pad()); body.put(d_out.pad()); body.put(d_cursor.pad()); body.put(d_idx.pad()); body.put(d_scale.pad());
    } else {
        for (int k = 0; k < 9; k++) body.put(status, 0);            // (sections 9 - 17 stay empty)
    }
    if (launch && cap > 0) {
        // the owner's own path on the same launches: the switches in the order the library asks for, the launch, the read and its refusal
        McAbundance ab;
        ab.bind(nseq, 0, nullptr);
        if (ab.set_counts(true, *A) || ab.set_ties(true, nullptr, 0) || ab.set_gene_bootstrap((int64_t)nrows) || ab.set_tie_bootstrap((int64_t)cap) || (nperm && ab.set_classes(true))) {
            fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3;
        }
        if (!ab.tboot || !ab.gboot || !ab.ties) { fprintf(stderr, "the owner's switches: ties %d, gene bootstrap %d, tie bootstrap %d\n", (int)ab.ties, (int)ab.gboot, (int)ab.tboot); return 1; }
        if (nperm && ab.ride_begin(d_perm, base[0], 1, nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
            if (ab.launch(d_rows + at, (uint32_t)(cuts[c] - at), nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
            CK_LAUNCH();
            ab.range_done(0);
        }
        ab.ride_end();
        std::vector<uint64_t> shares(ns * (size_t)B, ~0ull);
        std::vector<int64_t> dropped(1, -1);
        std::vector<double> stats(ns * MC_GB_NOUT, -1.0);
        g_err.clear();
        status[1] = ab.read_tie_bootstrap(B, seed[0], scale, shares.data(), stats.data(), dropped.data());
        CK(hipDeviceSynchronize());
        body.put(dropped); body.put(shares); body.put(stats); body.put(g_err.data(), g_err.size());
    }
    out.put(status, 4);
    for (const std::vector<uint8_t> &b : body.s) out.put(b);
    sections_write(argv[3], out);
    return 0;
}
