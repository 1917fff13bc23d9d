// gapped_win - the two host-compilable statements of the gapped X-drop extension (csrc/mc_core.h) on given flanks, without the
// marker index and without the search: tests/test_gapped_host.py holds them to the oracle's rs_align_gapped().
//
//   gapped_win IN OUT W [W ...]      (files of sections: order_io.h; tests/gapped_cases.py builds the flanks)
// IN:  0 offsets of the query flanks (nf + 1), 1 their residues (dense codes, walking order), 2 offsets of the subject flanks, 3 their
//      residues, 4 one int8 per flank: +1 walked forwards, -1 walked backwards in place (the residues are then laid out reversed in
//      memory and the function starts on the last one, as k_gapped_lds walks a left flank).
// OUT: one section of nf x (1 + number of W) x 9 int32: gain, c1, c2, ident, steps, runs, gapcols, overflow and the accessor's `ovf`
//      (a path statistic left its packed field) - first of mc_align_gapped on full-size cells, then of mc_align_gapped_win over a plain
//      array of the kernels' packed 8-byte cells (mc_gap_pack / mc_gap_unpack) for every W given.
#include "../../microbecensus_amd/csrc/mc_index.h"
#include "order_io.h"

struct HostWin {                                                     // the accessor k_gapped_lds hands the extension, over plain memory
    std::vector<uint32_t> W0, W1; uint32_t ovf = 0;
    explicit HostWin(int w) : W0(w), W1(w) {}
    void load(int c, int &h, int &d, uint32_t &ph, uint32_t &pd) const { mc_gap_unpack(W0.at(c), W1.at(c), h, d, ph, pd); }
    void store(int c, int h, int d, uint32_t ph, uint32_t pd) { ovf |= mc_gap_pack(h, d, ph, pd, W0.at(c), W1.at(c)); }
    int loadH(int c) const { return (int)(W0.at(c) << 20) >> 20; }
};

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: gapped_win IN OUT W [W ...]\n"); return 2; }
    Sections in = sections_read(argv[1]), out;
    size_t no1, nq, no2, ns, nst;
    const uint32_t *off1 = in.take<uint32_t>(&no1);
    const uint8_t *q = in.take<uint8_t>(&nq);
    const uint32_t *off2 = in.take<uint32_t>(&no2);
    const uint8_t *s = in.take<uint8_t>(&ns);
    const int8_t *st = in.take<int8_t>(&nst);
    if (no1 < 1 || no1 != no2 || nst != no1 - 1 || off1[no1 - 1] != nq || off2[no2 - 1] != ns) { fprintf(stderr, "input: offsets malformed\n"); return 2; }
    const size_t nf = nst;
    for (size_t k = 0; k < nf; k++) {
        if (off1[k + 1] < off1[k] || off2[k + 1] < off2[k] || off1[k + 1] - off1[k] >= MC_MAXAA || off2[k + 1] - off2[k] > 1200 - 8 || (st[k] != 1 && st[k] != -1)) { fprintf(stderr, "input: flank %zu is no flank of the pipeline\n", k); return 2; }
    }
    for (size_t i = 0; i < nq; i++) if (q[i] > MC_INV) { fprintf(stderr, "input: query residue %d\n", q[i]); return 2; }
    for (size_t i = 0; i < ns; i++) if (s[i] > MC_INV) { fprintf(stderr, "input: subject residue %d\n", s[i]); return 2; }
    std::vector<int> widths;
    for (int a = 3; a < argc; a++) { const int w = atoi(argv[a]); if (w < 16 || w > 1200) { fprintf(stderr, "W out of range (16..1200)\n"); return 2; } widths.push_back(w); }
    static McTables T;
    McHostIndex X;                                                   // the substitution scores and the X-drop threshold do not depend on the index
    X.rt_mask = 0; X.max_bucket = 0; X.freq_thr = 0; X.nres = 1000000; X.nseq = 1000;
    for (int g = 0; g < 10; g++) X.letter_p[g] = 0.1;
    mc_fill_tables(T, X, 510, 1.0);
    std::vector<McGapCell> cells(1200);
    std::vector<int32_t> res;
    auto put = [&](const McGapResult &R, uint32_t ovf) { for (int v : {R.gain, R.c1, R.c2, R.ident, R.steps, R.runs, R.gapcols, R.overflow, (int)(ovf != 0)}) res.push_back(v); };
    for (size_t k = 0; k < nf; k++) {
        const int n1 = (int)(off1[k + 1] - off1[k]), n2 = (int)(off2[k + 1] - off2[k]);
        std::vector<uint8_t> a(q + off1[k], q + off1[k + 1]), b(s + off2[k], s + off2[k + 1]);   // exactly the flank: a read past either end is an error of the tools that check this program
        if (st[k] < 0) { std::reverse(a.begin(), a.end()); std::reverse(b.begin(), b.end()); }
        const uint8_t *pa = a.empty() ? nullptr : (st[k] < 0 ? &a.back() : a.data()), *pb = b.empty() ? nullptr : (st[k] < 0 ? &b.back() : b.data());
        put(mc_align_gapped(T, pa, st[k], pb, st[k], n1, n2, cells.data(), (int)cells.size()), 0);
        for (int w : widths) {
            HostWin ws(w);
            const McGapResult R = mc_align_gapped_win(T, pa, st[k], pb, st[k], n1, n2, ws, w);
            put(R, ws.ovf);
        }
    }
    out.put(res);
    sections_write(argv[2], out);
    return 0;
}
