// tests/emul/covboot.cpp - the rules of the coverage bootstrap that need no GPU (csrc/mc_covboot.h: mc_cb_read - the very text
// k_covboot_collect runs per thread -, mc_cb_entry, mc_cb_id, mc_cb_present, mc_cb_clip and the serial cover of one gene and replicate,
// window by window, mc_cb_cover; the weights are csrc/mc_boot.h's, the six doubles csrc/mc_geneboot.h's mc_gb_gene) compiled by g++ and run
// on the CPU: a stand-alone program that includes the library's headers and copies none of them.
//   covboot run IN OUT      (files of sections: order_io.h; tests/covboot_cases.py writes IN - the files of device_covboot.hip - and reads OUT)
// IN:  the cut-offs (4 + 4 + 8 + 8 bytes: min_ident, min_aln, min_bits, max_loge), four int32 (nseq, B, capacity, launch: the last is the
//      device harness'), off (nseq + 1 residue offsets), the rows (McRow), the launches (uint32: the row index behind each launch's last
//      row), seed, perm (uint32; none: a row's query is the id), base (int64) and need (nseq uint32, or none).
// OUT: the list (min(entries, capacity) entries of 12 bytes, in the order of the rows), two uint64 (the cursor, dropped), the covered
//      residues (nseq x B uint64, [s * B + b]; of the entries that fitted), the six doubles of every gene (nseq x 6) and det (nseq uint64;
//      empty without need).
// The slot reservation is a running count.  Every array lives in a std::vector of its exact size and is indexed with at():
// -fsanitize=address sees an access behind any of them - the list among them, which is `capacity` long, and the window's marks.
#include "../../microbecensus_amd/csrc/mc_covboot.h"

#include "order_io.h"

struct Pars { int32_t min_ident, min_aln; double min_bits, max_loge; };
struct Pass {
    Pars A;
    bool operator()(const McRow &r) const { return 100 * r.frame >= A.min_ident * r.alnlen && r.alnlen >= A.min_aln && r.bits >= A.min_bits && r.loge <= A.max_loge; }
};
struct Len {
    const std::vector<uint32_t> *off;
    uint32_t operator()(int32_t s) const { return off->at((size_t)s + 1) - off->at((size_t)s); }
};

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: covboot run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, nmeta, noff, nrows, ncuts, nseed, nperm, nbase, nneed;
    const Pars *A = in.take<Pars>(&npars);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const uint32_t *offp = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const uint32_t *cuts = in.take<uint32_t>(&ncuts);
    const uint64_t *seed = in.take<uint64_t>(&nseed);
    const uint32_t *perm = in.take<uint32_t>(&nperm);
    const int64_t *base = in.take<int64_t>(&nbase);
    const uint32_t *need = in.take<uint32_t>(&nneed);
    if (npars != 1 || nmeta != 4 || meta[0] < 1 || meta[1] < 1 || meta[1] > MC_GB_MAXB || meta[2] < 0 || noff != (size_t)meta[0] + 1 || nseed != 1 || nbase != 1 ||
        (nneed && nneed != (size_t)meta[0]) || ncuts < 1 || cuts[ncuts - 1] != nrows) {
        fprintf(stderr, "input: malformed\n"); return 2;
    }
    const size_t ns = (size_t)meta[0], B = (size_t)meta[1], cap = (size_t)meta[2];
    const std::vector<uint32_t> off(offp, offp + noff);
    for (size_t s = 0; s < ns; s++) if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 65535u) { fprintf(stderr, "input: gene %zu\n", s); return 2; }
    for (size_t s = 0; s < nneed; s++) if (!need[s]) { fprintf(stderr, "input: need[%zu] is 0\n", s); return 2; }
    Pass pass; pass.A = *A;
    const Len len = {&off};
    std::vector<McCbEntry> list(cap);
    unsigned long long cursor = 0, dropped = 0;
    for (size_t c = 0, at = 0; c < ncuts; at = cuts[c++]) {
        if (cuts[c] < at) { fprintf(stderr, "input: launch %zu ends before it begins\n", c); return 2; }
        const std::vector<McRow> r(rows + at, rows + cuts[c]);       // (exact-size copies: a read past the last row is seen)
        for (size_t i = 0; i < r.size(); i++) {
            if (r[i].query < 0 || (i && r[i].query < r[i - 1].query) || (nperm && (size_t)r[i].query >= nperm)) { fprintf(stderr, "input: row %zu of launch %zu\n", i, c); return 2; }
            if (i && r[i - 1].query == r[i].query) continue;         // (the kernel's "one thread per read: the one at its first row")
            McCbEntry e;
            if (!mc_cb_read(pass, len, r.data(), (uint32_t)r.size(), (uint32_t)i, (int32_t)ns, mc_cb_id(nperm ? perm : nullptr, base[0], r[i].query), &e)) continue;
            if (cursor < cap) list.at((size_t)cursor) = e; else dropped++;
            cursor++;
        }
    }
    const size_t n = cursor < cap ? (size_t)cursor : cap;
    list.resize(n);
    if (dropped != cursor - n) { fprintf(stderr, "the cursor counts %llu entries, %zu fitted, %llu were dropped\n", cursor, n, dropped); return 1; }
    std::vector<unsigned long long> cov(ns * B, 0), det;
    std::vector<double> stats;
    const std::vector<double> ones(B, 1.0);
    for (size_t s = 0; s < ns; s++) {
        std::vector<McCbEntry> mine;
        for (size_t i = 0; i < n; i++) if (list.at(i).gene == s) mine.push_back(list[i]);
        std::vector<uint8_t> mark(MC_CB_WINDOW);
        for (size_t b = 0; b < B; b++) cov.at(s * B + b) = mc_cb_cover(mine.data(), mine.size(), len((int32_t)s), mc_boot_key(seed[0], b), mark.data());
        std::vector<double> x(B), part(MC_GB_THREADS), o(MC_GB_NOUT);
        const std::vector<unsigned long long> c(cov.begin() + s * B, cov.begin() + (s + 1) * B);
        mc_gb_gene(c.data(), ones.data(), (int)B, x.data(), part.data(), o.data());
        stats.insert(stats.end(), o.begin(), o.end());
        if (nneed) { unsigned long long d = 0; for (size_t b = 0; b < B; b++) d += c[b] >= need[s] ? 1 : 0; det.push_back(d); }
    }
    const std::vector<unsigned long long> cur = {cursor, dropped};
    out.put(list); out.put(cur); out.put(cov); out.put(stats); out.put(det);
    sections_write(argv[3], out);
    return 0;
}
