// tests/emul/geneboot.cpp - the rules of the gene bootstrap that need no GPU (csrc/mc_geneboot.h: mc_gb_used, mc_gb_value, mc_gb_index,
// mc_gb_thread_sum and mc_gb_tree - the very text k_geneboot_summary runs - and mc_gb_gene, the rule for one gene in serial form; the
// weights are csrc/mc_boot.h's) compiled by g++ and run on the CPU: a stand-alone program that includes the library's header and copies
// none of it.
//   geneboot run IN OUT      (files of sections: order_io.h; tests/geneboot_cases.py writes IN - the files of device_geneboot.hip - and reads OUT)
//   geneboot sums IN OUT     IN: counts (uint64, B of them), scale (B doubles); OUT: the six doubles of that one gene
// IN:  the cut-offs (4 + 4 + 8 + 8 bytes: min_ident, min_aln, min_bits, max_loge), four int32 (nseq, B, capacity, launch: the last two are
//      the device harness'), the rows (McRow), the launches (uint32: the row index behind each launch's last row), scale (B doubles), seed.
// OUT: the replicate counts (nseq x B uint64, [s * B + b]) and the six doubles of every gene (nseq x 6).
// The best row is found by the four comparisons of the statement (k_abundance.h has the device's); weights are added plainly.
// Every array lives in a std::vector of its exact size and is indexed with at(): -fsanitize=address sees an access behind any of them.
#include "../../microbecensus_amd/csrc/mc_geneboot.h"

#include "order_io.h"

struct Pars { int32_t min_ident, min_aln; double min_bits, max_loge; };

static std::vector<double> gene(const std::vector<unsigned long long> &c, const std::vector<double> &scale)
{
    std::vector<double> x(c.size()), part(MC_GB_THREADS), out(MC_GB_NOUT);
    mc_gb_gene(c.data(), scale.data(), (int)c.size(), x.data(), part.data(), out.data());
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 4 || (strcmp(argv[1], "run") && strcmp(argv[1], "sums"))) { fprintf(stderr, "usage: geneboot run|sums IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    if (!strcmp(argv[1], "sums")) {
        size_t nc, nsc;
        const unsigned long long *c = in.take<unsigned long long>(&nc);
        const double *sc = in.take<double>(&nsc);
        if (nc < 1 || nc > MC_GB_MAXB || nsc != nc) { fprintf(stderr, "input: malformed\n"); return 2; }
        out.put(gene(std::vector<unsigned long long>(c, c + nc), std::vector<double>(sc, sc + nsc)));
        sections_write(argv[3], out);
        return 0;
    }
    size_t npars, nmeta, nrows, ncuts, nscale, nseed;
    const Pars *A = in.take<Pars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const double *sc = in.take<double>(&nscale);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[1] < 1 || meta[1] > MC_GB_MAXB || nscale != (size_t)meta[1] || nseed != 1 || ncuts < 1 || cuts[ncuts - 1] != nrows) {
        fprintf(stderr, "input: malformed\n"); return 2;
    }
    const size_t ns = (size_t)meta[0], B = (size_t)meta[1];
    const std::vector<double> scale(sc, sc + B);
    std::vector<uint64_t> key(B);
    for (size_t b = 0; b < B; b++) key.at(b) = mc_boot_key(seed[0], b);
    std::vector<unsigned long long> counts(ns * B, 0);
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        const std::vector<McRow> r(rows + at, rows + cuts[c]);       // (exact-size copies: a read past the last row is seen)
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
            for (size_t b = 0; b < B; b++) counts.at((size_t)best->subject * B + b) += (unsigned long long)mc_boot_weight(key[b], (uint64_t)(uint32_t)best->query);
        }
    }
    std::vector<double> stats;
    for (size_t s = 0; s < ns; s++) {
        const std::vector<double> o = gene(std::vector<unsigned long long>(counts.begin() + s * B, counts.begin() + (s + 1) * B), scale);
        stats.insert(stats.end(), o.begin(), o.end());
    }
    out.put(counts); out.put(stats);
    sections_write(argv[3], out);
    return 0;
}
