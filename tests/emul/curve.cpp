// tests/emul/curve.cpp - the rules of the rarefaction curve that need no GPU (csrc/mc_curve.h: mc_curve_bin and mc_curve_first_bin, the
// very text the kernels k_curve and k_curve_scan run per thread, and mc_curve_gene, the scan's rule for one gene in serial form) compiled
// by g++ and run on the CPU: a stand-alone program that includes the library's header and copies none of it.
//   curve run IN OUT      (files of sections: order_io.h; tests/curve_cases.py writes IN - the files of device_curve.hip - and reads OUT)
// IN:  the cut-offs (4 + 4 + 8 + 8 bytes: min_ident, min_aln, min_bits, max_loge), off (nseq + 1 residue offsets), the rows (McRow), the
//      K points (uint64), the launches (uint32: the row index behind each launch's last row) and one int32: coverage (0 / 1).
// OUT: the bin table ((K + 1) x nseq x 2), first (nres; all 0xFFFFFFFF without coverage), the scan's output (K x nseq x 3, then K + 1 totals).
// The best row is found by the four comparisons of the statement (k_abundance.h has the device's); counts are added plainly.
// Every array lives in a std::vector of its exact size and is indexed with at(): -fsanitize=address sees an access behind any of them.
#include "../../microbecensus_amd/csrc/mc_curve.h"

#include "order_io.h"

struct Pars { int32_t min_ident, min_aln; double min_bits, max_loge; };

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: curve run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows, npts, ncuts, nmeta;
    const Pars *A = in.take<Pars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const unsigned long long *pts = in.take<unsigned long long>(&npts);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    if (npars != 1 || noff < 2 || off[0] != 0 || nmeta != 1 || npts < 1 || npts > MC_CURVE_MAXK || pts[0] < 1 || ncuts < 1 || cuts[ncuts - 1] != nrows) { fprintf(stderr, "input: malformed\n"); return 2; }
    for (size_t k = 1; k < npts; k++) if (pts[k] < pts[k - 1]) { fprintf(stderr, "input: point %zu descends\n", k); return 2; }
    const size_t ns = noff - 1, nres = off[ns];
    const int K = (int)npts;
    const bool cov = meta[0] != 0;
    const std::vector<unsigned long long> n(pts, pts + npts);        // (exact-size copies: a read past the last point or row is seen)
    std::vector<unsigned long long> bins(2 * (npts + 1) * ns, 0);
    std::vector<uint32_t> first(nres, MC_CURVE_NEVER);
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        const std::vector<McRow> r(rows + at, rows + cuts[c]);
        for (size_t i = 0; i < r.size(); i++) {
            if (r[i].query < 0 || (i && r[i].query < r[i - 1].query)) { fprintf(stderr, "input: row %zu of launch %zu\n", i, c); return 2; }
            if (i && r[i - 1].query == r[i].query) continue;         // (the kernel's "one thread per read: the one at its first row")
            const McRow *best = nullptr;
            for (size_t k = i; k < r.size() && r[k].query == r[i].query; k++) {
                const McRow &x = r.at(k);
                if (!(100 * x.frame >= A->min_ident * x.alnlen && x.alnlen >= A->min_aln && x.bits >= A->min_bits && x.loge <= A->max_loge)) continue;
                if (!best || best->bits < x.bits) best = &x;
            }
            if (!best || best->subject < 0 || (size_t)best->subject >= ns) continue;
            const uint32_t q = (uint32_t)best->query;
            const size_t s = (size_t)best->subject, slot = 2 * ((size_t)mc_curve_bin(n.data(), K, q) * ns + s);
            bins.at(slot) += 1; bins.at(slot + 1) += (unsigned long long)best->alnlen;
            const uint32_t len = off[s + 1] - off[s];
            if (cov && best->sstart >= 0 && best->sstart <= best->send && (uint32_t)best->send < len)
                for (int32_t p = best->sstart; p <= best->send; p++) { uint32_t &f = first.at(off[s] + (uint32_t)p); if (f > q) f = q; }
        }
    }
    std::vector<unsigned long long> res(3 * npts * ns + npts + 1, 0), br(npts + 1), ba(npts + 1), rk(npts), ak(npts), ck(npts);
    std::vector<uint32_t> hist(npts + 1);
    for (size_t s = 0; s < ns; s++) {
        for (size_t b = 0; b <= npts; b++) { br.at(b) = bins.at(2 * (b * ns + s)); ba.at(b) = bins.at(2 * (b * ns + s) + 1); }
        const std::vector<uint32_t> f(first.begin() + off[s], first.begin() + off[s + 1]);
        mc_curve_gene(n.data(), K, br.data(), ba.data(), cov ? f.data() : nullptr, (uint32_t)f.size(), hist.data(), rk.data(), ak.data(), ck.data());
        for (size_t k = 0; k < npts; k++) {
            res.at(3 * (k * ns + s)) = rk[k]; res.at(3 * (k * ns + s) + 1) = ak[k]; res.at(3 * (k * ns + s) + 2) = ck[k];
            res.at(3 * npts * ns + k) += rk[k];
        }
        res.at(3 * npts * ns + npts) += br[npts];
    }
    out.put(bins); out.put(first); out.put(res);
    sections_write(argv[3], out);
    return 0;
}
