// tests/emul/device_ties.hip - the tie kernel (csrc/k_ties.h: k_ties) behind the counting kernel on synthetic rows built to reach its
// edges: a stand-alone program that includes the library's kernel headers - it compiles the text the library compiles and copies none of
// it - and links neither the library nor the reader.
//   device_ties run IN OUT      (files of sections: order_io.h; tests/ties_cases.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), off (nseq + 1 residue offsets), the rows (McRow), ascending read id, group_of (nseq groups, or an
//      empty section: no map), and two int32: ngroups, coverage (0 / 1).
// OUT: 0 the counting kernel's tab ((nseq + 1) x 2), 1 the tie tab ((nseq + 1) x 2), 2 share (nseq), 3 group_unique (ngroups); with
//      coverage 4 the scan's 3 x nseq figures of the any-depth, 5 the any-depth of every residue, 6 the depth of every residue (the
//      counting kernel's marks), without it three empty sections; then the 16 elements of padding behind 7 the counting tab, 8 the tie
//      tab, 9 share, 10 group_unique, 11 the two difference arrays (zeros all), which no kernel may touch.
// The kernels are launched as range_end launches them: k_abundance (k_abundance_cov with coverage), then k_ties on the same rows with
// the same grid; null pointers where range_end hands in null pointers.  The input is checked before anything is launched (exit status
// 2); every HIP call is checked: an error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "k_abundance.h"
#include "k_coverage.h"
#include "k_ties.h"

#include "order_io.h"

#define CK(call)                                                                                                            \
    do {                                                                                                                    \
        hipError_t e_ = (call);                                                                                             \
        if (e_ != hipSuccess) { fprintf(stderr, "HIP error: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); fflush(stderr); exit(3); } \
    } while (0)
#define CK_LAUNCH() do { CK(hipGetLastError()); CK(hipDeviceSynchronize()); } while (0)

// a device array: uploaded or zeroed, read back whole, freed with the object.  16 elements of zeroed padding lie behind it: pad() reads
// them back, and the test asserts that no kernel wrote there
template <class T> struct Dev {
    T *p = nullptr; size_t n = 0;
    Dev(size_t count) : n(count) { CK(hipMalloc((void **)&p, (n + 16) * sizeof(T))); CK(hipMemset(p, 0, (n + 16) * sizeof(T))); }
    Dev(const T *h, size_t count) : Dev(count) { if (n) CK(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice)); }
    Dev(const Dev &) = delete;
    ~Dev() { (void)hipFree(p); }
    std::vector<T> host() const { std::vector<T> h(n); if (n) CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return h; }
    std::vector<T> pad() const { std::vector<T> h(16); CK(hipMemcpy(h.data(), p + n, 16 * sizeof(T), hipMemcpyDeviceToHost)); return h; }
    operator T *() const { return p; }
};

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
    const size_t nres = off[nseq], slots = nres + (size_t)nseq;

    Dev<uint32_t> d_off(off, noff), d_diff(cov ? slots : 0), d_any(cov ? slots : 0), d_depth(cov ? nres : 0), d_depth_any(cov ? nres : 0);
    Dev<McRow> d_rows(rows, nrows);
    Dev<int32_t> d_group(group_of, ngo);
    Dev<unsigned long long> d_tab(2 * ((size_t)nseq + 1)), d_ttab(2 * ((size_t)nseq + 1)), d_share((size_t)nseq), d_gu((size_t)ngroups), d_out(3 * (size_t)nseq), d_out_any(3 * (size_t)nseq);
    const uint32_t nr = (uint32_t)nrows;
    if (nr) {
        if (cov) k_abundance_cov<<<dim3((nr + 255) / 256), dim3(256)>>>(*A, d_rows, nr, nseq, d_tab, d_off, d_diff);
        else k_abundance<<<dim3((nr + 255) / 256), dim3(256)>>>(*A, d_rows, nr, nseq, d_tab);
        CK_LAUNCH();
        k_ties<<<dim3((nr + 255) / 256), dim3(256)>>>(*A, d_rows, nr, nseq, d_ttab, d_share, ngo ? (const int32_t *)d_group : nullptr, ngo ? (unsigned long long *)d_gu : nullptr,
                                                      cov ? (const uint32_t *)d_off : nullptr, cov ? (uint32_t *)d_any : nullptr);
        CK_LAUNCH();
    }
    out.put(d_tab.host()); out.put(d_ttab.host()); out.put(d_share.host()); out.put(d_gu.host());
    if (cov) {
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_ttab, d_off, d_any, nseq, d_out_any, d_depth_any); CK_LAUNCH();
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_out, d_depth); CK_LAUNCH();
        out.put(d_out_any.host()); out.put(d_depth_any.host()); out.put(d_depth.host());
    } else {
        for (int k = 0; k < 3; k++) out.put((const uint32_t *)nullptr, 0);
    }
    out.put(d_tab.pad()); out.put(d_ttab.pad()); out.put(d_share.pad()); out.put(d_gu.pad());
    { std::vector<uint32_t> p = d_diff.pad(), p2 = d_any.pad(); p.insert(p.end(), p2.begin(), p2.end()); out.put(p); }
    sections_write(argv[3], out);
    return 0;
}
