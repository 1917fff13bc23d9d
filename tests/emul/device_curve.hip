// tests/emul/device_curve.hip - the curve kernels (csrc/k_curve.h: k_curve, behind the counting kernel on a range's rows, and
// k_curve_scan) on synthetic rows built to reach their edges: a stand-alone program that includes the library's headers - it compiles the
// text the library compiles and copies none of it - and links neither the library nor the reader.
//   device_curve run IN OUT      (files of sections: order_io.h; tests/test_gpu_curve_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), off (nseq + 1 residue offsets), the rows (McRow), the K points (uint64), the launches (uint32: the row
//      index behind each launch's last row, ascending, the last one == the number of rows; rows ascend by read id WITHIN a launch), and
//      one int32: coverage (0 / 1).
// OUT: tab ((nseq + 1) x 2 counters of the counting kernel), the bin table ((K + 1) x nseq x 2), first (nres; without coverage no kernel is
//      handed it), the scan's output (K x nseq x 3, then K + 1 totals), and the 16 elements of padding behind tab and the bin table (zeros),
//      first and the scan's output (0xFF bytes) and the points (zeros), which no kernel may touch.
// Every launch goes through mc_abund_launch (csrc/mc_abund.h), the function range_end launches through; the scan with the grid of its
// launch site there.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an error is printed
// and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_curve run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows, npts, ncuts, nmeta;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const unsigned long long *pts = in.take<unsigned long long>(&npts);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    // the input is a legal state: a database within the engine's limits, points as mc_set_curve takes them, rows by ascending read id
    if (npars != 1 || noff < 2 || noff - 1 > 32767 || off[0] != 0 || nmeta != 1) { fprintf(stderr, "input: cut-offs, offsets or the switch malformed\n"); return 2; }
    const int32_t nseq = (int32_t)(noff - 1);
    const bool cov = meta[0] != 0;
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 2047) { fprintf(stderr, "input: gene %d has %lld residues\n", s, (long long)off[s + 1] - (long long)off[s]); return 2; }
    if (npts < 1 || npts > MC_CURVE_MAXK || pts[0] < 1) { fprintf(stderr, "input: %zu points, or a point below 1\n", npts); return 2; }
    for (size_t k = 1; k < npts; k++) if (pts[k] < pts[k - 1]) { fprintf(stderr, "input: point %zu descends\n", k); return 2; }
    if (nrows > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows) { fprintf(stderr, "input: %zu rows, %zu launches\n", nrows, ncuts); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++)
            if (rows[i].query < 0 || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a negative read id, or read ids descend within a launch\n", i); return 2; }
    }
    const size_t nres = off[nseq], ns = (size_t)nseq;
    const int32_t K = (int32_t)npts;

    Dev<uint32_t> d_off(off, noff), d_diff(mc_diff_slots(nres, ns)), d_first(nres, 0xFF);
    Dev<McRow> d_rows(rows, nrows);
    Dev<unsigned long long> d_pts(pts, npts), d_tab(mc_pair_slots(ns)), d_bins(mc_curve_bin_slots((size_t)K, ns)), d_out(mc_curve_out_slots((size_t)K, ns), 0xFF);
    McEvent own[4];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs B = {nseq, d_off, d_tab, cov ? (uint32_t *)d_diff : nullptr, nullptr, nullptr, nullptr};
    const McCurveBufs C = {K, d_pts, d_bins, cov ? (uint32_t *)d_first : nullptr, own[3]};
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (mc_abund_launch(*A, B, d_rows + at, (uint32_t)(cuts[c] - at), nullptr, ev, &C)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    const size_t tot = mc_curve_tot_at((size_t)K, ns);
    CK(hipMemset(d_out + tot, 0, ((size_t)K + 1) * sizeof(unsigned long long)));   // (McAbundance::read_curve zeroes the totals: the scan adds to them)
    k_curve_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_bins, d_pts, K, d_off, cov ? (uint32_t *)d_first : nullptr, nseq, d_out, d_out + tot); CK_LAUNCH();
    out.put(d_tab.host()); out.put(d_bins.host()); out.put(d_first.host()); out.put(d_out.host());
    out.put(d_tab.pad()); out.put(d_bins.pad()); out.put(d_first.pad()); out.put(d_out.pad()); out.put(d_pts.pad());
    sections_write(argv[3], out);
    return 0;
}
