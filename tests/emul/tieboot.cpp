// tests/emul/tieboot.cpp - the rules of the tie bootstrap that need no GPU (csrc/mc_tieboot.h: the two sinks of mc_ties_read and the two
// halves of a read, mc_tb_count and mc_tb_write - the very text k_tieboot_collect runs per thread -, mc_tb_share, mc_tb_scale, mc_tb_id;
// the walk is csrc/mc_ties.h's, the weights csrc/mc_boot.h's, the six doubles csrc/mc_geneboot.h's mc_gb_gene) compiled by g++ and run on
// the CPU: a stand-alone program that includes the library's headers and copies none of them.
//   tieboot run IN OUT      (files of sections: order_io.h; tests/tieboot_cases.py writes IN - the files of device_tieboot.hip - and reads OUT)
// IN:  the cut-offs (4 + 4 + 8 + 8 bytes: min_ident, min_aln, min_bits, max_loge), four int32 (nseq, B, capacity, launch: the last is the
//      device harness'), the rows (McRow), the launches (uint32: the row index behind each launch's last row), scale (B doubles), seed,
//      perm (uint32; none: a row's query is the id) and base (int64).
// OUT: the list (min(entries, capacity) entries of 12 bytes, in the order of the rows), two uint64 (the cursor, dropped), the replicate
//      shares (nseq x B uint64, [s * B + b]; of the entries that fitted) and the six doubles of every gene (nseq x 6).
// The slot reservation is a running count; weights times shares are added plainly.  Every array lives in a std::vector of its exact size
// and is indexed with at(): -fsanitize=address sees an access behind any of them - the list among them, which is `capacity` long.
#include "../../microbecensus_amd/csrc/mc_tieboot.h"

#include "order_io.h"

struct Pars { int32_t min_ident, min_aln; double min_bits, max_loge; };
struct Pass {
    Pars A;
    bool operator()(const McRow &r) const { return 100 * r.frame >= A.min_ident * r.alnlen && r.alnlen >= A.min_aln && r.bits >= A.min_bits && r.loge <= A.max_loge; }
};

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: tieboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, nrows, ncuts, nscale, nseed, nperm, nbase;
    const Pars *A = in.take<Pars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const double *sc = in.take<double>(&nscale);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    const uint32_t *perm = in.take<uint32_t>(&nperm);
    const int64_t *base = in.take<int64_t>(&nbase);
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 0 || meta[2] > MC_TB_MAXCAP || nscale != (size_t)meta[1] || nseed != 1 || nbase != 1 ||
        ncuts < 1 || cuts[ncuts - 1] != nrows) {
        fprintf(stderr, "input: malformed\n"); return 2;
    }
    const size_t ns = (size_t)meta[0], B = (size_t)meta[1], cap = (size_t)meta[2];
    Pass pass; pass.A = *A;
    std::vector<McTbEntry> list(cap);
    unsigned long long cursor = 0, dropped = 0;
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        const std::vector<McRow> r(rows + at, rows + cuts[c]);       // (exact-size copies: a read past the last row is seen)
        for (size_t i = 0; i < r.size(); i++) {
            if (r[i].query < 0 || (i && r[i].query < r[i - 1].query) || (nperm && (size_t)r[i].query >= nperm)) { fprintf(stderr, "input: row %zu of launch %zu\n", i, c); return 2; }
            if (i && r[i - 1].query == r[i].query) continue;         // (the kernel's "one thread per read: the one at its first row")
            const uint32_t k = mc_tb_count(pass, r.data(), (uint32_t)r.size(), (uint32_t)i, (int32_t)ns);
            if (!k) continue;
            dropped += mc_tb_write(pass, r.data(), (uint32_t)r.size(), (uint32_t)i, (int32_t)ns, mc_tb_id(nperm ? perm : nullptr, base[0], r[i].query), list.data(), cap, cursor);
            cursor += k;
        }
    }
    const size_t n = cursor < cap ? (size_t)cursor : cap;
    list.resize(n);
    if (dropped != cursor - n) { fprintf(stderr, "the cursor counts %llu entries, %zu fitted, %llu were dropped\n", cursor, n, dropped); return 1; }
    std::vector<uint64_t> key(B);
    for (size_t b = 0; b < B; b++) key.at(b) = mc_boot_key(seed[0], b);
    std::vector<unsigned long long> shares(ns * B, 0);
    for (size_t i = 0; i < n; i++) {
        const McTbEntry &e = list.at(i);
        for (size_t b = 0; b < B; b++) shares.at((size_t)e.gene * B + b) += (unsigned long long)mc_boot_weight(key[b], (uint64_t)e.q) * mc_tb_share(e);
    }
    std::vector<double> s32(B), stats;
    for (size_t b = 0; b < B; b++) s32.at(b) = mc_tb_scale(sc[b]);
    for (size_t s = 0; s < ns; s++) {
        std::vector<double> x(B), part(MC_GB_THREADS), o(MC_GB_NOUT);
        const std::vector<unsigned long long> c(shares.begin() + s * B, shares.begin() + (s + 1) * B);
        mc_gb_gene(c.data(), s32.data(), (int)B, x.data(), part.data(), o.data());
        stats.insert(stats.end(), o.begin(), o.end());
    }
    const std::vector<unsigned long long> cur = {cursor, dropped};
    out.put(list); out.put(cur); out.put(shares); out.put(stats);
    sections_write(argv[3], out);
    return 0;
}
