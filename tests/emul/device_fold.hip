// tests/emul/device_fold.hip - the fold of long genes (csrc/k_fold.h: k_fold, in front of the abundance kernels; csrc/mc_fold.h states the
// rule) on synthetic rows built to reach its edges: a stand-alone program that includes the library's headers - it compiles the text the
// library compiles and copies none of it - and links neither the library nor the reader.  No search runs.
//   device_fold run IN OUT      (files of sections: order_io.h; tests/test_gpu_fold_units.py writes IN and reads OUT)
// IN:  the cut-offs (McAbundPars); five int32 (the segments of the index, the genes, K points of a curve or 0, B replicates of a gene
//      bootstrap or 0, its capacity); the segment records (McFoldSeg, one per segment); the genes' residue offsets (uint32, genes + 1); the
//      rows (McRow, subjects are SEGMENTS); the launches (uint32: the row index behind each launch's last row, ascending, the last one ==
//      the number of rows; rows ascend by read id within a launch); the curve's points (uint64); scale (B doubles); the seed (uint64).
// OUT: 0 the folded rows of every launch, one after the other, as k_fold left them in the owner's buffer; 1 edge_rows and the genes
//      mc_gene_fold_stats would report (int64 x 2); 2 - 4 reads, aligned (int64 per gene), [searched, assigned]; 5 - 7 covered, spanned,
//      max_depth; 8 the depth of every residue of every gene; 9 - 11 candidates, unique, share; 12 [ambiguous]; 13 covered_any; then with
//      K > 0: 14 - 16 the curve's reads, aligned, covered (K x genes), 17 assigned (K), 18 [beyond]; otherwise five empty sections; then
//      with B > 0: 19 counts (genes x B), 20 stats (genes x 6), 21 [dropped]; otherwise three empty sections.
// Everything runs through the owner, McAbundance (csrc/mc_abund.h): set_fold, the switches, launch - which folds and then calls
// mc_abund_launch, the one site the library has - and the readers, all in gene space.  The input is checked before anything is launched
// (exit status 2); every HIP call is checked: an error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "mc_abund.h"

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH

#define OWN(call) do { if ((call) != 0) { fprintf(stderr, "HIP error: %s: %s (line %d)\n", #call, g_err.c_str(), __LINE__); fflush(stderr); exit(3); } } while (0)

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: device_fold run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nseg, ngoff, nrows, ncuts, npts, nscale, nseed;
    const McAbundPars *A = in.take<McAbundPars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McFoldSeg *seg = in.take<McFoldSeg>(&nseg);
    const uint32_t *goff = in.take<uint32_t>(&ngoff);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const unsigned long long *pts = in.take<unsigned long long>(&npts);
    const double *scale = in.take<double>(&nscale);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    // the input is a legal state: segments within the engine's limits, records that point into their genes, rows by ascending read id
    if (npars != 1 || nmeta != 5 || meta[0] < 1 || meta[0] > MC_FOLD_MAX_SEGS || meta[1] < 1 || meta[1] > meta[0] || nseg != (size_t)meta[0] || ngoff != (size_t)meta[1] + 1 || goff[0] != 0 ||
        meta[2] < 0 || meta[2] > MC_CURVE_MAXK || npts != (size_t)meta[2] || meta[3] < 0 || meta[3] > MC_GB_MAXB || nscale != (size_t)meta[3] || meta[4] < 0 || meta[4] > (1 << 24) || nseed != 1) {
        fprintf(stderr, "input: cut-offs, sizes, records, offsets, points, scale or seed malformed\n"); return 2;
    }
    const int32_t nsegs = meta[0], ngenes = meta[1], K = meta[2], B = meta[3];
    for (int32_t g = 0; g < ngenes; g++)
        if (goff[g + 1] <= goff[g] || goff[g + 1] - goff[g] > MC_FOLD_MAX_GENE) { fprintf(stderr, "input: gene %d has %lld residues\n", g, (long long)goff[g + 1] - (long long)goff[g]); return 2; }
    for (int32_t s = 0; s < nsegs; s++) {
        const McFoldSeg &r = seg[s];
        const bool ok = r.gene >= 0 && r.gene < ngenes && r.off >= 0 && (uint32_t)r.off < goff[r.gene + 1] - goff[r.gene] && r.lo >= -1 && r.lo <= 0 && r.hi >= -1 && r.hi < MC_FOLD_SEG_LEN;
        if (!ok) { fprintf(stderr, "input: the record of segment %d points outside its gene\n", s); return 2; }
    }
    if (nrows > (1u << 24) || ncuts < 1 || cuts[ncuts - 1] != nrows) { fprintf(stderr, "input: %zu rows, %zu launches\n", nrows, ncuts); return 2; }
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        for (size_t i = at; i < cuts[c]; i++)
            if (rows[i].query < 0 || (i > at && rows[i].query < rows[i - 1].query)) { fprintf(stderr, "input: row %zu: a negative read id, or read ids descend within a launch\n", i); return 2; }
    }
    const size_t ng = (size_t)ngenes, nres = goff[ngenes];

    McRow *d_rows = nullptr;
    CK(hipMalloc((void **)&d_rows, (nrows + 1) * sizeof(McRow)));
    if (nrows) CK(hipMemcpy(d_rows, rows, nrows * sizeof(McRow), hipMemcpyHostToDevice));
    {
        McAbundance ab;
        ab.bind(nsegs, 0, nullptr);                                   // (the index's offsets: nothing reads them under a fold)
        OWN(ab.set_fold(ngenes, seg, goff));
        OWN(ab.set_counts(true, *A)); OWN(ab.set_coverage(true)); OWN(ab.set_ties(true, nullptr, 0));
        if (K) OWN(ab.set_curve(K, pts));
        if (B) OWN(ab.set_gene_bootstrap((int64_t)meta[4]));
        std::vector<McRow> folded(nrows);
        for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
            const size_t n = cuts[c] - at;
            OWN(ab.launch(d_rows + at, (uint32_t)n, nullptr));
            CK_LAUNCH();
            if (n > ab.folded_cap) { fprintf(stderr, "the folded rows hold %zu, the launch had %zu\n", ab.folded_cap, n); return 3; }
            if (n) CK(hipMemcpy(folded.data() + at, ab.d_folded, n * sizeof(McRow), hipMemcpyDeviceToHost));
            ab.range_done(0);
        }
        out.put(folded);
        int64_t edge[2] = {-1, ab.fold ? ab.nseq : 0};
        OWN(ab.read_fold(&edge[0]));
        out.put(edge, 2);
        std::vector<int64_t> a(ng), b(ng), c3(ng), tot(2);
        OWN(ab.read_counts(a.data(), b.data(), &tot[0], &tot[1]));
        out.put(a); out.put(b); out.put(tot);
        OWN(ab.read_figures(false, a.data(), b.data(), c3.data()));
        out.put(a); out.put(b); out.put(c3);
        std::vector<uint32_t> depth(nres);
        OWN(ab.read_depth(depth.data()));
        out.put(depth);
        std::vector<uint64_t> share(ng); int64_t amb[2] = {0, 0};
        OWN(ab.read_ties(a.data(), b.data(), share.data(), nullptr, &amb[0], &amb[1]));
        out.put(a); out.put(b); out.put(share); out.put(amb, 1);
        OWN(ab.read_figures(true, a.data(), nullptr, nullptr));
        out.put(a);
        if (K) {
            std::vector<int64_t> cr((size_t)K * ng), ca((size_t)K * ng), cc((size_t)K * ng), cas((size_t)K), beyond(1);
            OWN(ab.read_curve(cr.data(), ca.data(), cc.data(), cas.data(), beyond.data()));
            out.put(cr); out.put(ca); out.put(cc); out.put(cas); out.put(beyond);
        } else for (int k = 0; k < 5; k++) out.put((const int64_t *)nullptr, 0);
        if (B) {
            std::vector<int64_t> counts(ng * (size_t)B), dropped(1, -1);
            std::vector<double> stats(ng * MC_GB_NOUT);
            OWN(ab.read_gene_bootstrap(B, seed[0], scale, counts.data(), stats.data(), dropped.data()));
            out.put(counts); out.put(stats); out.put(dropped);
        } else for (int k = 0; k < 3; k++) out.put((const int64_t *)nullptr, 0);
        CK(hipDeviceSynchronize());
    }
    CK(hipFree(d_rows));
    sections_write(argv[3], out);
    return 0;
}
