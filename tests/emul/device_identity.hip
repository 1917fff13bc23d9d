// tests/emul/device_identity.hip - the identity kernels (csrc/k_identity.h: k_identity, the third walk behind the counting kernel, and
// k_identity_scan) on synthetic rows built to reach their edges: a stand-alone program that includes the library's headers - it compiles
// the text the library compiles and copies none of it - and links neither the library nor the reader.
//   device_identity run IN OUT      (files of sections: order_io.h; tests/order_cases.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), two int32 (nseq; identity 0 / 1), the rows (McRow), ascending read id, and the levels (0 .. 8 int32).
// OUT: tab ((nseq + 1) x 2 counters), hist (nseq x MC_ID_STRIDE counters, the padding of every gene with it), sums (nseq records of four
//      uint64), the scan's nseq x (3 + nlevels) values (with the identity off no scan runs: the section holds what the buffer was filled
//      with), and the 16 elements of padding behind tab, hist, sums and the scan's output, which no kernel may touch.
// With the identity off the launch is handed a null pointer and hist, sums and the scan's output - handed to nobody - are filled with 0x5A
// bytes first: they must come back as they were.  With it on hist and sums start as zeros and the scan's output as 0xFF bytes.
// Both kernels are launched by the library's launch functions (csrc/mc_abund.h: mc_abund_launch, the function range_end launches
// through, and mc_identity_launch, the read's).  The input is checked before anything is launched (exit status 2); every HIP call is
// checked: an error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_identity run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nrows, nlev;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McRow *rows = in.take<McRow>(&nrows);
    const int32_t *lev = in.take<int32_t>(&nlev);
    // the input is a legal state: a database within the engine's limits, rows by ascending read id, levels the ABI would take
    if (npars != 1 || nmeta != 2 || meta[0] < 1 || meta[0] > 32767 || nlev > MC_ID_LEVELS || mc_id_bad_level(lev, (int)nlev) >= 0) { fprintf(stderr, "input: cut-offs, sizes or levels malformed\n"); return 2; }
    if (nrows > (1u << 24)) { fprintf(stderr, "input: %zu rows\n", nrows); return 2; }
    for (size_t i = 1; i < nrows; i++) if (rows[i].query < rows[i - 1].query) { fprintf(stderr, "input: row %zu: read ids descend\n", i); return 2; }
    const int32_t nseq = meta[0];
    const bool ident = meta[1] != 0;
    const size_t ns = (size_t)nseq, nout = 3 + nlev;

    Dev<McRow> d_rows(rows, nrows);
    Dev<int32_t> d_lev(lev, nlev);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns));
    Dev<uint32_t> d_hist(mc_id_hist_slots(ns), ident ? 0 : 0x5A);
    Dev<McIdSums> d_sums(ns, ident ? 0 : 0x5A);
    Dev<long long> d_out(nout * ns, ident ? 0xFF : 0x5A);
    McEvent own[6];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs B = {nseq, nullptr, d_tab, nullptr, nullptr, nullptr, nullptr};
    const McIdentBufs I = {d_hist, d_sums, own[3]};
    if (mc_abund_launch(*A, B, d_rows, (uint32_t)nrows, nullptr, ev, nullptr, nullptr, nullptr, nullptr, nullptr, ident ? &I : nullptr)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    if (ident) {
        const McIdentRead R = {nseq, d_hist, d_lev, (int32_t)nlev, d_out};
        const hipEvent_t sev[2] = {own[4], own[5]};
        if (mc_identity_launch(R, nullptr, sev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
        CK_LAUNCH();
    }
    out.put(d_tab.host()); out.put(d_hist.host()); out.put(d_sums.host()); out.put(d_out.host());
    out.put(d_tab.pad()); out.put(d_hist.pad()); out.put(d_sums.pad()); out.put(d_out.pad());
    sections_write(argv[3], out);
    return 0;
}
