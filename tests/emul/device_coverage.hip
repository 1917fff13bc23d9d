// tests/emul/device_coverage.hip - the coverage kernels (csrc/k_coverage.h: k_abundance_cov, the counting kernel that also marks, and
// k_coverage_scan) and the counting kernel without coverage (csrc/k_abundance.h: k_abundance) on synthetic rows built to reach their
// edges: a stand-alone program that includes the library's headers - it compiles the text the library compiles and copies none of it -
// and links neither the library nor the reader.
//   device_coverage run IN OUT      (files of sections: order_io.h; tests/order_cases.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), off (nseq + 1 residue offsets), the rows (McRow), ascending read id, and one int32: coverage (0 / 1).
// OUT: tab ((nseq + 1) x 2 counters), the scan's 3 x nseq figures and the depth of every residue from a scan WITH the depth, the 3 x nseq
//      figures of a second scan WITHOUT it (without coverage no scan runs: three empty sections), the difference array as the kernels
//      left it (nres + nseq slots; without coverage no kernel is handed it), and the 16 elements of padding behind tab (zeros), the two
//      figure arrays and the depth (0xFF bytes) and the difference array (zeros), which no kernel may touch.
// The counting kernel is launched by mc_abund_launch (csrc/mc_abund.h), the function range_end launches it through; the scans with the
// grid of their launch site there.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an
// error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_coverage run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows, nmeta;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    // the input is a legal state: a database within the engine's limits, rows by ascending read id
    if (npars != 1 || noff < 2 || noff - 1 > 32767 || off[0] != 0 || nmeta != 1) { fprintf(stderr, "input: cut-offs, offsets or the switch malformed\n"); return 2; }
    const int32_t nseq = (int32_t)(noff - 1);
    const bool cov = meta[0] != 0;
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 2047) { fprintf(stderr, "input: gene %d has %lld residues\n", s, (long long)off[s + 1] - (long long)off[s]); return 2; }
    if (nrows > (1u << 24)) { fprintf(stderr, "input: %zu rows\n", nrows); return 2; }
    for (size_t i = 1; i < nrows; i++) if (rows[i].query < rows[i - 1].query) { fprintf(stderr, "input: row %zu: read ids descend\n", i); return 2; }
    const size_t nres = off[nseq], ns = (size_t)nseq;

    Dev<uint32_t> d_off(off, noff), d_diff(mc_diff_slots(nres, ns)), d_depth(nres + 16, 0xFF);    // (d_depth: 16 elements of its own behind the nres that are zeroed below, and the padding)
    Dev<McRow> d_rows(rows, nrows);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_out(3 * ns, 0xFF), d_out2(3 * ns, 0xFF);
    McEvent own[3];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs B = {nseq, d_off, d_tab, cov ? (uint32_t *)d_diff : nullptr, nullptr, nullptr, nullptr};
    if (mc_abund_launch(*A, B, d_rows, (uint32_t)nrows, nullptr, ev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    out.put(d_tab.host());
    if (cov) {
        CK(hipMemset(d_depth, 0, nres * sizeof(uint32_t)));              // (mc_coverage_depth zeroes it: the genes without reads are not written)
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_out, d_depth); CK_LAUNCH();
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_out2, nullptr); CK_LAUNCH();
        out.put(d_out.host()); out.put(d_depth.host().data(), nres); out.put(d_out2.host());
    } else {
        for (int k = 0; k < 3; k++) out.put((const uint32_t *)nullptr, 0);
    }
    out.put(d_diff.host());
    out.put(d_tab.pad()); out.put(d_out.pad()); out.put(d_out2.pad()); out.put(d_depth.host().data() + nres, 16); out.put(d_depth.pad()); out.put(d_diff.pad());
    sections_write(argv[3], out);
    return 0;
}
