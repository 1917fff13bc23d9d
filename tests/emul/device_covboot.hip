// tests/emul/device_covboot.hip - the coverage bootstrap's kernels (csrc/k_covboot.h: k_covboot_collect, behind the counting kernel
// k_abundance_cov on a range's rows, and at read time k_covboot_scatter, k_covboot_cover and the gene bootstrap's k_geneboot_summary) on
// synthetic rows built to reach their edges: a stand-alone program that includes the library's headers - it compiles the text the library
// compiles and copies none of it - and links neither the library nor the reader.
//   device_covboot run IN OUT      (files of sections: order_io.h; tests/test_gpu_covboot_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), four int32 (nseq, B, capacity - 0 .. 2^24 -, launch: 0 hands the launches NO coverage list), off (nseq + 1
//      residue offsets; a gene has 1 .. 65,535 residues), the rows (McRow), the launches (uint32: the row index behind each launch's last
//      row, ascending, the last one == the number of rows; rows ascend by read id WITHIN a launch), the seed (uint64), perm (uint32; none: a
//      row's query is the read's id; else every query is an index into it), base (int64) and need (nseq uint32, none of them 0; or none).
// OUT: 0 status (int32: launch, the owner's return value, genes with reads, whether the read ran); 1 the count table ((nseq + 1) x 2); 2 the
//      difference array as k_abundance_cov left it (residues + nseq slots); 3 the list (capacity entries, 0xEE bytes where nothing was
//      written); 4 the cursor and dropped; 5 - 8 the 16 elements of padding behind those four; 9 - 20: when the read ran (the list was handed
//      over and nothing was dropped; empty otherwise) 9 the grouped list, 10 mat (genes with reads x B), 11 det (genes with reads; zeros
//      without need), 12 the six doubles of those genes, 13 - 20 the padding behind the grouped list, mat, det, the output, the genes'
//      cursors, their compact indices, their records and the ones; then, when a list was handed over and the capacity is not 0,
//      McAbundance's own answer on the same launches: 21 dropped, 22 covered (nseq x B), 23 stats (nseq x 6), 24 detected (nseq; empty
//      without need), 25 its error message, 26 covered of its coverage scan (nseq); behind them coverage is turned off, which must take the
//      coverage bootstrap with it.
// Every launch goes through mc_abund_launch and the read through mc_covboot_launch (csrc/mc_abund.h), the functions the library launches
// through.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an error is printed and ends
// the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_covboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, noff, nrows, ncuts, nseed, nperm, nbase, nneed;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    const uint32_t *perm = in.take<uint32_t>(&nperm);
    const int64_t *base = in.take<int64_t>(&nbase);
    const uint32_t *need = in.take<uint32_t>(&nneed);
    // the input is a legal state: a database within the gene-space limits, B and a capacity as the ABI takes them, rows by ascending read
    // id, every id below 2^31, no need of 0
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[0] > 32767 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 0 || meta[2] > (1 << 24) || noff != (size_t)meta[0] + 1 || off[0] != 0 ||
        nseed != 1 || nbase != 1 || base[0] < 0 || (nneed && nneed != (size_t)meta[0])) {
        fprintf(stderr, "input: cut-offs, sizes, offsets, seed, base or need malformed\n"); return 2;
    }
    const int32_t nseq = meta[0], B = meta[1];
    for (int32_t s = 0; s < nseq; s++) {
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 65535u) { fprintf(stderr, "input: gene %d has %lld residues\n", s, (long long)off[s + 1] - (long long)off[s]); return 2; }
        if (nneed && !need[s]) { fprintf(stderr, "input: need[%d] is 0\n", s); return 2; }
    }
    if (nrows < 1 || nrows > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows || off[nseq] > (1u << 26)) { fprintf(stderr, "input: %zu rows, %zu launches\n", nrows, ncuts); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++) {
            if (rows[i].query < 0 || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a negative read id, or read ids descend within a launch\n", i); return 2; }
            if (nperm && ((size_t)rows[i].query >= nperm || base[0] + (int64_t)perm[rows[i].query] > 0x7fffffffll)) { fprintf(stderr, "input: row %zu: no id in the map\n", i); return 2; }
        }
    }
    const size_t ns = (size_t)nseq, nres = off[nseq], cap = (size_t)meta[2];
    const bool launch = meta[3] != 0;

    Dev<McRow> d_rows(rows, nrows);
    Dev<uint32_t> d_perm(perm, nperm), d_off(off, noff), d_diff(mc_diff_slots(nres, ns));
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_cur(2);
    Dev<McCbEntry> d_list(cap, 0xEE);
    McEvent own[8];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs Bf = {nseq, d_off, d_tab, d_diff, nullptr, nullptr, nullptr};
    const McCovBootBufs V = {d_list, (unsigned long long)cap, d_cur, own[3]};
    Dev<unsigned long long> d_cls(MC_AC_SLOTS);
    const McIdMap map = {d_perm, base[0]};
    const McClassRide R = {map, d_cls, 1, 0, 0ull, own[4]};          // (a ride of one class: the id map of the launches, as a class run hands it over)
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (mc_abund_launch(*A, Bf, d_rows + at, (uint32_t)(cuts[c] - at), nullptr, ev, nullptr, nullptr, nperm ? &R : nullptr, nullptr, launch ? &V : nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    const std::vector<unsigned long long> tab = d_tab.host(), cur = d_cur.host();
    std::vector<uint32_t> start(ns); std::vector<int32_t> idx(ns);
    unsigned long long total = 0;
    const int32_t ng = mc_gb_plan(tab.data(), nseq, start.data(), idx.data(), &total);
    const bool read = launch && cur[1] == 0 && cur[0] == total && cur[0] <= cap;            // (what McAbundance::read_coverage_bootstrap asks before it reads)
    int32_t status[4] = {launch ? 1 : 0, 0, ng, read ? 1 : 0};
    Sections body;
    body.put(tab); body.put(d_diff.host()); body.put(d_list.host()); body.put(cur);
    body.put(d_tab.pad()); body.put(d_diff.pad()); body.put(d_list.pad()); body.put(d_cur.pad());
    if (read) {
        const size_t n = (size_t)cur[0], want = (size_t)ng * (size_t)B;
        std::vector<McCbGene> genes((size_t)ng);
        for (size_t s = 0; s < ns; s++)
            if (idx[s] >= 0) genes[(size_t)idx[s]] = {start[s], (uint32_t)tab[mc_pair_at(s)], off[s + 1] - off[s], nneed ? need[s] : 0u};
        const std::vector<double> ones((size_t)B, 1.0);
        Dev<uint32_t> d_cursor(start.data(), ns);
        Dev<int32_t> d_idx(idx.data(), ns);
        Dev<McCbEntry> d_sorted(n, 0xEE);
        Dev<McCbGene> d_genes(genes.data(), (size_t)ng);
        Dev<unsigned long long> d_mat(want, 0xEE), d_det((size_t)ng);
        Dev<double> d_ones(ones.data(), (size_t)B), d_out((size_t)MC_GB_NOUT * (size_t)ng, 0xFF);
        const McCovBootRead Rd = {nseq, ng, (long long)n, d_list, d_cursor, d_idx, d_sorted, d_genes, d_mat, nneed ? (unsigned long long *)d_det : nullptr, d_ones, B, seed[0], d_out};
        const hipEvent_t rev[2] = {own[5], own[6]};
        if (mc_covboot_launch(Rd, nullptr, rev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
        body.put(d_sorted.host()); body.put(d_mat.host()); body.put(d_det.host()); body.put(d_out.host());
        body.put(d_sorted.pad()); body.put(d_mat.pad()); body.put(d_det.pad()); body.put(d_out.pad()); body.put(d_cursor.pad()); body.put(d_idx.pad()); body.put(d_genes.pad()); body.put(d_ones.pad());
    } else {
        for (int k = 0; k < 12; k++) body.put(status, 0);           // (sections 9 - 20 stay empty)
    }
    if (launch && cap > 0) {
        // the owner's own path on the same launches: the switches in the order the library asks for, the launch, the read and its refusal
        McAbundance ab;
        ab.bind(nseq, nres, d_off);
        if (ab.set_counts(true, *A) || ab.set_coverage(true) || ab.set_coverage_bootstrap((int64_t)cap) || (nperm && ab.set_classes(true))) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        if (!ab.cboot || !ab.cov || ab.gboot || ab.ties) { fprintf(stderr, "the owner's switches: coverage %d, coverage bootstrap %d, gene bootstrap %d, ties %d\n", (int)ab.cov, (int)ab.cboot, (int)ab.gboot, (int)ab.ties); return 1; }
        if (nperm && ab.ride_begin(d_perm, base[0], 1, nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
            if (ab.launch(d_rows + at, (uint32_t)(cuts[c] - at), nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
            CK_LAUNCH();
            ab.range_done(0);
        }
        ab.ride_end();
        std::vector<int64_t> covered(ns * (size_t)B, -1), dropped(1, -1), detected(nneed ? ns : 0, -1), scan(ns, -1);
        std::vector<double> stats(ns * MC_GB_NOUT, -1.0);
        g_err.clear();
        status[1] = ab.read_coverage_bootstrap(B, seed[0], nneed ? need : nullptr, covered.data(), stats.data(), nneed ? detected.data() : nullptr, dropped.data());
        CK(hipDeviceSynchronize());
        const std::string err = g_err;
        if (ab.read_figures(false, scan.data(), nullptr, nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        // coverage going off takes the switch with it, and frees its list
        if (ab.set_coverage(false) || ab.cboot || ab.d_clist || !ab.on) { fprintf(stderr, "coverage went off and the coverage bootstrap stayed on\n"); return 1; }
        CK(hipDeviceSynchronize());
        body.put(dropped); body.put(covered); body.put(stats); body.put(detected); body.put(err.data(), err.size()); body.put(scan);
    }
    out.put(status, 4);
    for (const std::vector<uint8_t> &b : body.s) out.put(b);
    sections_write(argv[3], out);
    return 0;
}
