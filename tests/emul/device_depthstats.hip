// tests/emul/device_depthstats.hip - the selection kernel of the depth statistics (csrc/k_depthstats.h: k_depth_select) on depths that the
// library's own counting kernels mark from synthetic rows built to reach its edges: a stand-alone program that includes the library's headers -
// it compiles the text the library compiles and copies none of it - and links neither the library nor the reader.
//   device_depthstats run IN OUT      (files of sections: order_io.h; tests/test_gpu_depthstats_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), off (nseq + 1 residue offsets), the rows (McRow), ascending read id, keep (the percents P to read at, int32,
//      1 .. 100 each), and one int32: ties (0 / 1).
// OUT: 0 tab ((nseq + 1) x 2 counters); 1 k_coverage_scan's 3 x nseq figures and 2 the depth of every residue; 3 the difference array before the
//      reads and 4 behind them (nres + nseq slots each); 5 the reads' figures, per P nseq x 4 (median, trimmed_sum, low, high); with ties the same
//      six of the any-depth, the head of the tie table as its tab, in 6 .. 11 (without: six empty sections); then the 16 elements of padding
//      behind 12 tab, 13 the tie table, 14 the two difference arrays (zeros all), 15 the two figure arrays of the reads (0xFF bytes), which no
//      kernel may touch.
// The marks are made by mc_abund_launch (csrc/mc_abund.h), the function range_end launches them through; every read by mc_depthstats_launch,
// the function the library reads through.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an
// error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

// the reads of one depth: the scan with the depth, the difference array before and behind, and one selection per P
static void read_all(Sections &out, const unsigned long long *d_tab, const uint32_t *d_off, const Dev<uint32_t> &d_diff, int32_t nseq, size_t nres, const int32_t *keep, size_t nkeep,
                     const Dev<unsigned long long> &d_ds, const hipEvent_t (&ev)[2])
{
    const size_t ns = (size_t)nseq;
    Dev<unsigned long long> d_fig(3 * ns);
    Dev<uint32_t> d_depth(nres);
    k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_fig, d_depth); CK_LAUNCH();
    out.put(d_fig.host()); out.put(d_depth.host()); out.put(d_diff.host());
    std::vector<unsigned long long> all;
    for (size_t k = 0; k < nkeep; k++) {
        const McDepthRead R = {d_tab, d_off, d_diff, nseq, keep[k], d_ds};
        if (mc_depthstats_launch(R, nullptr, ev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); exit(3); }
        CK_LAUNCH();
        const std::vector<unsigned long long> one = d_ds.host();
        all.insert(all.end(), one.begin(), one.end());
    }
    out.put(d_diff.host()); out.put(all);
}

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_depthstats run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows, nkeep, nmeta;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const int32_t *keep = in.take<int32_t>(&nkeep);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    // the input is a legal state: a database within the limits of gene space (mc_fold.h), rows by ascending read id, percents the ABI accepts
    if (npars != 1 || noff < 2 || noff - 1 > 32767 || off[0] != 0 || nmeta != 1 || nkeep < 1 || nkeep > 16) { fprintf(stderr, "input: cut-offs, offsets, percents or the switch malformed\n"); return 2; }
    const int32_t nseq = (int32_t)(noff - 1);
    const bool ties = meta[0] != 0;
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 65535) { fprintf(stderr, "input: gene %d has %lld residues\n", s, (long long)off[s + 1] - (long long)off[s]); return 2; }
    for (size_t k = 0; k < nkeep; k++) if (!mc_ds_keep_ok(keep[k])) { fprintf(stderr, "input: P %d\n", keep[k]); return 2; }
    if (nrows > (1u << 24)) { fprintf(stderr, "input: %zu rows\n", nrows); return 2; }
    for (size_t i = 1; i < nrows; i++) if (rows[i].query < rows[i - 1].query) { fprintf(stderr, "input: row %zu: read ids descend\n", i); return 2; }
    const size_t nres = off[nseq], ns = (size_t)nseq, slots = mc_diff_slots(nres, ns);

    Dev<uint32_t> d_off(off, noff), d_diff(slots), d_any(ties ? slots : 0);
    Dev<McRow> d_rows(rows, nrows);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_ties(ties ? mc_tie_slots(ns, 0) : 0), d_ds(mc_ds_out_slots(ns), 0xFF), d_ds_any(mc_ds_out_slots(ns), 0xFF);
    McEvent own[3];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]}, ev_read[2] = {own[0], own[1]};
    const McAbundBufs B = {nseq, d_off, d_tab, d_diff, ties ? (unsigned long long *)d_ties : nullptr, nullptr, ties ? (uint32_t *)d_any : nullptr};
    if (mc_abund_launch(*A, B, d_rows, (uint32_t)nrows, nullptr, ev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    out.put(d_tab.host());
    read_all(out, d_tab, d_off, d_diff, nseq, nres, keep, nkeep, d_ds, ev_read);
    if (ties) {
        out.put(d_ties.host().data(), mc_tie_share_at(ns));
        read_all(out, d_ties, d_off, d_any, nseq, nres, keep, nkeep, d_ds_any, ev_read);
    } else {
        for (int k = 0; k < 6; k++) out.put((const uint32_t *)nullptr, 0);
    }
    out.put(d_tab.pad()); out.put(d_ties.pad());
    { std::vector<uint32_t> p = d_diff.pad(), p2 = d_any.pad(); p.insert(p.end(), p2.begin(), p2.end()); out.put(p); }
    { std::vector<unsigned long long> p = d_ds.pad(), p2 = d_ds_any.pad(); p.insert(p.end(), p2.begin(), p2.end()); out.put(p); }
    sections_write(argv[3], out);
    return 0;
}
