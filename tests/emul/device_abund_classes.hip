// tests/emul/device_abund_classes.hip - the kernels of the counts on class runs (csrc/k_geneboot.h: k_geneboot_collect_mapped, which takes a
// read's id through the batch's id map; csrc/k_abund_classes.h: k_abund_class_add, the per-class table) on synthetic rows built to reach
// their edges: a stand-alone program that includes the library's headers - it compiles the text the library compiles and copies none of
// it - and links neither the library nor the reader.
//   device_abund_classes run IN OUT      (files of sections: order_io.h; tests/test_gpu_abund_classes_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars); five int32 (nseq, capacity, mapped: 0 hands the launches NO class ride, K, the rows below the lowest
//      class); the id base (int64); the rows (McRow; `query` is a position of the sorted batch); the launches (uint32: the row index
//      behind each launch's last row, ascending, the last one == the number of rows; rows ascend by `query` WITHIN a launch); every
//      launch's class (int32) and reads (uint64); perm (uint32: the row index of every sorted position).
// OUT: 0 status (int32: mapped, the owner's `searched`); 1 tab ((nseq + 1) x 2 counters of the counting kernel); 2 the list (capacity
//      entries, 0xEE bytes where nothing was written); 3 the cursor and dropped; 4 the per-class buffer (MC_AC_SLOTS counters; untouched
//      zeros without a ride); 5 - 8 the 16 elements of padding behind those four; then McAbundance's own answer on the same launches
//      (the switches, ride_begin, ride_piece, launch, rows_below, ride_end; without a ride: the launches alone): 9 its list, 10 its cursor
//      and dropped, 11 the rows and 12 the assigned of its per-class table (K + 1 values each; empty without a ride).
// Every launch goes through mc_abund_launch (csrc/mc_abund.h), the function the library launches through.  The input is checked before
// anything is launched (exit status 2) - every `query` lies inside perm and every id below 2^31 -; every HIP call is checked: an error
// is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_abund_classes run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nbase, nrows, ncuts, ncls, nreads, nperm;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const int64_t *base = in.take<int64_t>(&nbase);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const int32_t *cls = in.take<int32_t>(&ncls);
    const uint64_t *reads = in.take<uint64_t>(&nreads);
    const uint32_t *perm = in.take<uint32_t>(&nperm);
    if (npars != 1 || nmeta != 5 || nbase != 1 || meta[0] < 1 || meta[0] > 32767 || meta[1] < 1 || meta[1] > (1 << 24) || meta[3] < 1 || meta[3] > MC_CLS_MAX || meta[4] < 0 || base[0] < 0) {
        fprintf(stderr, "input: cut-offs, sizes or base malformed\n"); return 2;
    }
    if (nrows > (1u << 24) || nperm < 1 || nperm > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows || ncls != ncuts || nreads != ncuts) { fprintf(stderr, "input: %zu rows, %zu launches, %zu positions\n", nrows, ncuts, nperm); return 2; }
    for (size_t i = 0; i < nperm; i++)
        if (base[0] + (int64_t)perm[i] > 0x7fffffffll) { fprintf(stderr, "input: position %zu: the id is not below 2^31\n", i); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at || cls[c] < 0 || cls[c] >= meta[3]) { fprintf(stderr, "input: launch %zu ends before it begins, or is of no class\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++)
            if (rows[i].query < 0 || (size_t)rows[i].query >= nperm || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a position outside perm, or positions descend within a launch\n", i); return 2; }
    }
    const int32_t nseq = meta[0], K = meta[3];
    const size_t ns = (size_t)nseq, cap = (size_t)meta[1];
    const bool mapped = meta[2] != 0;

    Dev<McRow> d_rows(rows, nrows);
    Dev<uint32_t> d_perm(perm, nperm);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_cur(2), d_cls(MC_AC_SLOTS);
    Dev<McGbEntry> d_list(cap, 0xEE);
    McEvent own[5];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs Bf = {nseq, nullptr, d_tab, nullptr, nullptr, nullptr, nullptr};
    const McGeneBootBufs G = {d_list, (unsigned long long)cap, d_cur, own[3]};
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        const McClassRide R = {McIdMap{d_perm, base[0]}, d_cls, K, cls[c], (unsigned long long)reads[c], own[4]};
        if (mc_abund_launch(*A, Bf, d_rows + at, (uint32_t)(cuts[c] - at), nullptr, ev, nullptr, &G, mapped ? &R : nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    if (mapped && meta[4]) {                                         // the rows below the lowest class: slot K, no counting kernel
        k_abund_class_add<<<dim3(1), dim3(64)>>>(d_cls, K, K, (unsigned long long)meta[4], d_tab + mc_pair_at(ns));
        CK_LAUNCH();
    }
    Sections body;
    body.put(d_tab.host()); body.put(d_list.host()); body.put(d_cur.host()); body.put(d_cls.host());
    body.put(d_tab.pad()); body.put(d_list.pad()); body.put(d_cur.pad()); body.put(d_cls.pad());

    // the owner's own path on the same launches
    McAbundance ab;
    ab.bind(nseq, 0, nullptr);
    if (ab.set_counts(true, *A) || ab.set_gene_bootstrap((int64_t)cap) || (mapped && ab.set_classes(true))) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    if (mapped && ab.ride_begin(d_perm, base[0], K, nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        ab.ride_piece(cls[c]);
        if (ab.launch(d_rows + at, (uint32_t)(cuts[c] - at), nullptr, (int64_t)reads[c])) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
        ab.range_done((int64_t)reads[c]);
    }
    if (ab.rows_below(meta[4], nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    ab.ride_end();
    std::vector<McGbEntry> olist(cap);
    std::vector<unsigned long long> ocur(2);
    CK(hipMemcpy(olist.data(), ab.d_glist, cap * sizeof(McGbEntry), hipMemcpyDeviceToHost));
    CK(hipMemcpy(ocur.data(), ab.d_gcur, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<int64_t> orows(mapped ? (size_t)K + 1 : 0, -1), oassigned(orows.size(), -1);
    if (mapped && ab.read_classes(orows.data(), oassigned.data(), K + 1)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    body.put(olist); body.put(ocur); body.put(orows); body.put(oassigned);
    const int32_t status[2] = {mapped ? 1 : 0, (int32_t)ab.searched};
    out.put(status, 2);
    for (const std::vector<uint8_t> &b : body.s) out.put(b);
    sections_write(argv[3], out);
    return 0;
}
