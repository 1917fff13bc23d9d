// tests/emul/device_coverage.hip - the coverage kernels (csrc/k_coverage.h: k_abundance_cov, the counting kernel that also marks, and
// k_coverage_scan) on synthetic rows built to reach their edges: a stand-alone program that includes the library's kernel headers - it
// compiles the text the library compiles and copies none of it - and links neither the library nor the reader.
//   device_coverage run IN OUT      (files of sections: order_io.h; tests/order_cases.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars), off (nseq + 1 residue offsets), the rows (McRow), ascending read id.
// OUT: tab ((nseq + 1) x 2 counters), the scan's 3 x nseq figures and the depth of every residue from a scan WITH the depth, the 3 x nseq
//      figures of a second scan WITHOUT it, the difference array as both scans left it (nres + nseq slots), and the 16 elements of padding
//      behind tab (zeros), the two figure arrays and the depth (0xFF bytes) and the difference array (zeros), which no kernel may touch.
// The kernels are launched with the grids of their launch sites in mc_hip.hip.  The input is checked before anything is launched (exit
// status 2); every HIP call is checked: an error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "k_abundance.h"
#include "k_coverage.h"

#include "order_io.h"

#define CK(call)                                                                                                            \
    do {                                                                                                                    \
        hipError_t e_ = (call);                                                                                             \
        if (e_ != hipSuccess) { fprintf(stderr, "HIP error: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); fflush(stderr); exit(3); } \
    } while (0)
#define CK_LAUNCH() do { CK(hipGetLastError()); CK(hipDeviceSynchronize()); } while (0)

// a device array: uploaded or filled with one byte, read back whole, freed with the object.  16 elements of padding lie behind it,
// filled with the same byte: pad() reads them back, and the test asserts that no kernel wrote there
template <class T> struct Dev {
    T *p = nullptr; size_t n = 0;
    Dev(size_t count, int fill = 0) : n(count) { CK(hipMalloc((void **)&p, (n + 16) * sizeof(T))); CK(hipMemset(p, fill, (n + 16) * sizeof(T))); }
    Dev(const T *h, size_t count) : Dev(count) { if (n) CK(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice)); }
    Dev(const Dev &) = delete;
    ~Dev() { (void)hipFree(p); }
    std::vector<T> host() const { std::vector<T> h(n); if (n) CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return h; }
    std::vector<T> pad() const { std::vector<T> h(16); CK(hipMemcpy(h.data(), p + n, 16 * sizeof(T), hipMemcpyDeviceToHost)); return h; }
    operator T *() const { return p; }
};

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_coverage run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    // the input is a legal state: a database within the engine's limits, rows by ascending read id
    if (npars != 1 || noff < 2 || noff - 1 > 32767 || off[0] != 0) { fprintf(stderr, "input: cut-offs or offsets malformed\n"); return 2; }
    const int32_t nseq = (int32_t)(noff - 1);
    for (int32_t s = 0; s < nseq; s++)
        if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 2047) { fprintf(stderr, "input: gene %d has %lld residues\n", s, (long long)off[s + 1] - (long long)off[s]); return 2; }
    if (nrows > (1u << 24)) { fprintf(stderr, "input: %zu rows\n", nrows); return 2; }
    for (size_t i = 1; i < nrows; i++) if (rows[i].query < rows[i - 1].query) { fprintf(stderr, "input: row %zu: read ids descend\n", i); return 2; }
    const size_t nres = off[nseq], slots = nres + (size_t)nseq;

    Dev<uint32_t> d_off(off, noff), d_diff(slots), d_depth(nres + 16, 0xFF);    // (d_depth: 16 elements of its own behind the nres that are zeroed below, and the padding)
    Dev<McRow> d_rows(rows, nrows);
    Dev<unsigned long long> d_tab(2 * ((size_t)nseq + 1)), d_out(3 * (size_t)nseq, 0xFF), d_out2(3 * (size_t)nseq, 0xFF);
    const uint32_t nr = (uint32_t)nrows;
    if (nr) { k_abundance_cov<<<dim3((nr + 255) / 256), dim3(256)>>>(*A, d_rows, nr, nseq, d_tab, d_off, d_diff); CK_LAUNCH(); }
    CK(hipMemset(d_depth, 0, nres * sizeof(uint32_t)));                  // (mc_coverage_depth zeroes it: the genes without reads are not written)
    k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_out, d_depth); CK_LAUNCH();
    k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256)>>>(d_tab, d_off, d_diff, nseq, d_out2, nullptr); CK_LAUNCH();
    out.put(d_tab.host()); out.put(d_out.host()); out.put(d_depth.host().data(), nres); out.put(d_out2.host()); out.put(d_diff.host());
    out.put(d_tab.pad()); out.put(d_out.pad()); out.put(d_out2.pad()); out.put(d_depth.host().data() + nres, 16); out.put(d_depth.pad()); out.put(d_diff.pad());
    sections_write(argv[3], out);
    return 0;
}
