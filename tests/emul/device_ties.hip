// tests/emul/device_ties.hip - the tie kernel (csrc/k_ties.h: k_ties) behind the counting kernel on synthetic rows built to reach its
// edges: a stand-alone program that includes the library's kernel headers - it compiles the text the library compiles and copies none of
// it - and links neither the library nor the reader.
//   device_ties run IN OUT      (files of sections: order_io.h; tests/ties_cases.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), off (nseq + 1 residue offsets), the rows (McRow), ascending read id, group_of (nseq groups, or an
//      empty section: no map), and two int32: ngroups, coverage (0 / 1).
// OUT: 0 the counting kernel's tab ((nseq + 1) x 2), 1 the tie tab ((nseq + 1) x 2), 2 share (nseq), 3 group_unique (ngroups) - the three
//      parts of the ONE tie table, cut where csrc/mc_abund.h's layout cuts it; with coverage 4 the scan's 3 x nseq figures of the
//      any-depth, 5 the any-depth of every residue, 6 the depth of every residue (the counting kernel's marks), without it three empty
//      sections; then the 16 elements of padding behind 7 the counting tab, 8 the tie table, 9 the two difference arrays (zeros all),
//      which no kernel may touch.
// The kernels are launched by mc_abund_launch (csrc/mc_abund.h), the function range_end launches them through: k_abundance
// (k_abundance_cov with coverage), then k_ties on the same rows with the same grid; null pointers where range_end hands in null
// pointers.  The input is checked before anything is launched (exit status 2); every HIP call is checked: an error is printed and ends
// the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_ties run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows, ngo, nmeta;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const int32_t *group_of = in.take<int32_t>(&ngo);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    // the input is a legal state: a database within the engine's limits, rows by ascending read id, a map as mc_set_ties accepts it
    if (npars != 1 || noff < 2 || noff - 1 > 32767 || off[0] != 0 || nmeta != 2) { fprintf(stderr, "input: cut-offs, offsets or switches malformed\n"); return 2; }
    const int32_t nseq = (int32_t)(noff - 1), ngroups = meta[0];
    const bool cov = meta[1] != 0;
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 2047) { fprintf(stderr, "input: gene %d has %lld residues\n", s, (long long)off[s + 1] - (long long)off[s]); return 2; }
    if (ngroups < 0 || (ngo != 0 && ngo != (size_t)nseq) || (ngo == 0) != (ngroups == 0)) { fprintf(stderr, "input: %zu group entries, %d groups\n", ngo, ngroups); return 2; }
    for (size_t s = 0; s < ngo; s++) if (group_of[s] < 0 || group_of[s] >= ngroups) { fprintf(stderr, "input: group_of[%zu] = %d\n", s, group_of[s]); return 2; }
    if (nrows > (1u << 24)) { fprintf(stderr, "input: %zu rows\n", nrows); return 2; }
    for (size_t i = 1; i < nrows; i++) if (rows[i].query < rows[i - 1].query) { fprintf(stderr, "input: row %zu: read ids descend\n", i); return 2; }
    const size_t nres = off[nseq], ns = (size_t)nseq, slots = mc_diff_slots(nres, ns);

    Dev<uint32_t> d_off(off, noff), d_diff(cov ? slots : 0), d_any(cov ? slots : 0), d_depth(cov ? nres : 0), d_depth_any(cov ? nres : 0);
    Dev<McRow> d_rows(rows, nrows);
    Dev<int32_t> d_group(group_of, ngo);
    Dev<unsigned long long> d_tab(mc_pair_slots(ns)), d_ties(mc_tie_slots(ns, (size_t)ngroups)), d_out(3 * ns), d_out_any(3 * ns);
    McEvent own[3];
    for (McEvent &e : own) if (e.create()) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    const hipEvent_t ev[3] = {own[0], own[1], own[2]};
    const McAbundBufs B = {nseq, d_off, d_tab, cov ? (uint32_t *)d_diff : nullptr, d_ties, ngo ? (const int32_t *)d_group : nullptr, cov ? (uint32_t *)d_any : nullptr};
    if (mc_abund_launch(*A, B, d_rows, (uint32_t)nrows, nullptr, ev)) { fprintf(stderr, "HIP error: %s\n", g_err.c_str()); return 3; }
    CK_LAUNCH();
    const std::vector<unsigned long long> ties = d_ties.host();
    out.put(d_tab.host()); out.put(ties.data(), mc_tie_share_at(ns)); out.put(ties.data() + mc_tie_share_at(ns), ns); out.put(ties.data() + mc_tie_group_at(ns), (size_t)ngroups);
    if (cov) {
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_ties, d_off, d_any, nseq, d_out_any, d_depth_any); CK_LAUNCH();
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_out, d_depth); CK_LAUNCH();
        out.put(d_out_any.host()); out.put(d_depth_any.host()); out.put(d_depth.host());
    } else {
        for (int k = 0; k < 3; k++) out.put((const uint32_t *)nullptr, 0);
    }
    out.put(d_tab.pad()); out.put(d_ties.pad());
    { std::vector<uint32_t> p = d_diff.pad(), p2 = d_any.pad(); p.insert(p.end(), p2.begin(), p2.end()); out.put(p); }
    sections_write(argv[3], out);
    return 0;
}
