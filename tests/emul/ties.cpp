// tests/emul/ties.cpp - the per-read walk of the tie accounting (csrc/mc_ties.h: mc_ties_read, the very text the kernel k_ties runs
// per thread) compiled by g++ and run on the CPU: a stand-alone program that includes the library's header and copies none of it.
//   ties run IN OUT      (files of sections: order_io.h; tests/ties_cases.py writes IN and reads OUT - the files of device_ties.hip)
// IN:  the cut-offs (4 + 4 + 8 + 8 bytes: min_ident, min_aln, min_bits, max_loge), off (nseq + 1 residue offsets), the rows (McRow),
//      ascending read id, group_of (nseq groups, or an empty section: no map), and two int32: ngroups, coverage (0 / 1).
// OUT: tab ((nseq + 1) x 2: candidates, unique; [nseq]: ambiguous, group_ambiguous), share (nseq), group_unique (ngroups), the
//      any-depth of every residue (nres; all zero without coverage).
// The sink adds plainly, residue by residue; the cut-offs are the four comparisons of the statement (k_abundance.h has the device's).
// Every array the walk may write lives in a std::vector of its exact size: -fsanitize=address sees a write behind any of them.
#include "../../microbecensus_amd/csrc/mc_ties.h"

#include "order_io.h"

struct Pars { int32_t min_ident, min_aln; double min_bits, max_loge; };
struct Pass {
    Pars A;
    bool operator()(const McRow &r) const { return 100 * r.frame >= A.min_ident * r.alnlen && r.alnlen >= A.min_aln && r.bits >= A.min_bits && r.loge <= A.max_loge; }
};
struct Sink {
    std::vector<uint64_t> tab, shr, gu;
    std::vector<uint32_t> depth;
    const uint32_t *off; bool cov;
    bool marks() const { return cov; }
    void cand(int32_t s) { tab.at(2 * (size_t)s)++; }
    void uniq(int32_t s) { tab.at(2 * (size_t)s + 1)++; }
    void share(int32_t s, unsigned long long v) { shr.at((size_t)s) += v; }
    void group_uniq(int32_t g) { gu.at((size_t)g)++; }
    void mark(int32_t s, int32_t a, int32_t b)
    {
        const uint32_t len = off[s + 1] - off[s];
        if (a >= 0 && a <= b && (uint32_t)b < len) for (int32_t p = a; p <= b; p++) depth.at(off[s] + (uint32_t)p)++;
    }
};

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: ties run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npars, noff, nrows, ngo, nmeta;
    const Pars *A = in.take<Pars>(&npars);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McRow *rows = in.take<McRow>(&nrows);
    const int32_t *group_of = in.take<int32_t>(&ngo);
    const int32_t *meta = in.take<int32_t>(&nmeta);
    if (npars != 1 || noff < 2 || off[0] != 0 || nmeta != 2 || meta[0] < 0 || (ngo != 0 && ngo != noff - 1) || (ngo == 0) != (meta[0] == 0)) { fprintf(stderr, "input: malformed\n"); return 2; }
    const int32_t nseq = (int32_t)(noff - 1), ngroups = meta[0];
    for (size_t s = 0; s < ngo; s++) if (group_of[s] < 0 || group_of[s] >= ngroups) { fprintf(stderr, "input: group_of[%zu]\n", s); return 2; }
    for (size_t i = 1; i < nrows; i++) if (rows[i].query < rows[i - 1].query) { fprintf(stderr, "input: row %zu: read ids descend\n", i); return 2; }
    std::vector<McRow> r(rows, rows + nrows);                        // (an exact-size copy: a read past the last row is seen)
    Pass pass; pass.A = *A;
    Sink sink; sink.tab.assign(2 * ((size_t)nseq + 1), 0); sink.shr.assign((size_t)nseq, 0); sink.gu.assign((size_t)ngroups, 0); sink.depth.assign(off[nseq], 0);
    sink.off = off; sink.cov = meta[1] != 0;
    for (uint32_t i = 0; i < (uint32_t)nrows; i++) {
        if (i && r[i - 1].query == r[i].query) continue;             // (the kernel's "one thread per read: the one at its first row")
        const McTieRead t = mc_ties_read(pass, r.data(), (uint32_t)nrows, i, nseq, ngo ? group_of : nullptr, sink);
        if (t.k > 1) sink.tab[2 * (size_t)nseq]++;
        if (t.across) sink.tab[2 * (size_t)nseq + 1]++;
    }
    out.put(sink.tab); out.put(sink.shr); out.put(sink.gu); out.put(sink.depth);
    sections_write(argv[3], out);
    return 0;
}
