// tests/emul/seeds.cpp - the host statements of the seed stage (csrc/mc_core.h: mc_eval_seed_core, mc_make_hsp, mc_enumerate_seeds) on the
// inputs of tests/seed_cases.py, for tests/test_seeds_host.py to hold to the oracle's rs_extend_hit / rs_seed_ranges.  Built with g++.
//   seeds IN OUT      (files of sections: order_io.h)
// IN: 0 three int32 (read length, FP, reads), 1 the frames (reads x 6 x FP dense codes), 2 the subjects' letters, 3 their offsets,
//     4 the hits (seven int32 each: read, frame, qpos, sidx, dpos, seedlen, nkey), 5 the rows to enumerate (read * 6 + frame, int32).
// OUT: 0 per hit 24 int32: the result of mc_eval_seed_core (0 dropped, 1 ungapped, 2 to the gapped extension), the McGapTask's sidx, qp,
//      dp, L, qfwd, qbwd, score, nmatch, whether mc_make_hsp keeps the HSP of a result 1, and its score, frame, alnlen, mism, gaps, nmatch,
//      qaas, qaae, ds, de, qnts, qnte, two zeros; 1 per hit the HSP's loge; 2 per row the number of ranges; 3 the ranges (seven int32:
//      pos, bucket, seedlen, nkey, nst, ned, phase); 4 the postings of the index; 5 its bucket starts.
#include "../../microbecensus_amd/csrc/mc_finish.h"
#include "../../microbecensus_amd/csrc/mc_index.h"
#include "order_io.h"

struct Ranges {
    std::vector<int32_t> *out; int n;
    void operator()(int bucket, int nst, int cnt, int seedlen, int nkey, int pos, int phase)
    {
        const int32_t r[7] = {pos, bucket, seedlen, nkey, nst, nst + cnt, phase};
        out->insert(out->end(), r, r + 7); n++;
    }
};

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: seeds IN OUT\n"); return 2; }
    Sections in = sections_read(argv[1]), out;
    size_t nmeta, nfr, ntext, noff, nh, nrows;
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const uint8_t *frames = in.take<uint8_t>(&nfr);
    const char *text = (const char *)in.take<uint8_t>(&ntext);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const int32_t *hits = in.take<int32_t>(&nh);
    const int32_t *rows = in.take<int32_t>(&nrows);
    if (nmeta != 3 || nh % 7 || noff < 2) { fprintf(stderr, "input malformed\n"); return 2; }
    nh /= 7;
    const int L = meta[0], FP = meta[1], nreads = meta[2], nseq = (int)(noff - 1);
    if (nfr != (size_t)nreads * 6 * (size_t)FP || off[nseq] != ntext) { fprintf(stderr, "input malformed\n"); return 2; }
    std::vector<std::string> seqs(nseq), names(nseq);
    std::vector<const char *> np(nseq), sp(nseq);
    for (int s = 0; s < nseq; s++) { seqs[s].assign(text + off[s], text + off[s + 1]); names[s] = "s" + std::to_string(s); np[s] = names[s].c_str(); sp[s] = seqs[s].c_str(); }
    McHostIndex H; std::string err;
    if (!mc_build_index(H, np.data(), sp.data(), nseq, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    static McTables T;
    mc_fill_tables(T, H, L, 1.0);
    McIndex X; memset(&X, 0, sizeof X);
    X.res = H.res.data(); X.off = H.off.data(); X.bstart = H.bstart.data(); X.post = H.post.data(); X.keys = H.keys.data(); X.rec = H.rec.empty() ? nullptr : H.rec.data();
    X.filt = H.filt.data(); X.wild = H.wild.data(); X.pair = H.pair.data(); X.rt = H.rt.data(); X.rt_mask = H.rt_mask; X.nseq = H.nseq;

    std::vector<int32_t> res(nh * 24, 0);
    std::vector<double> loge(nh, 0.0);
    for (size_t k = 0; k < nh; k++) {
        const int32_t *h = hits + 7 * k;
        const int read = h[0], frame = h[1], qpos = h[2], sidx = h[3], dpos = h[4], seedlen = h[5], nkey = h[6];
        const int qlen = (L - frame % 3) / 3;
        if (read < 0 || read >= nreads || frame < 0 || frame > 5 || sidx < 0 || sidx >= nseq || qpos < 0 || qpos + seedlen > qlen || dpos < 0 || (uint32_t)dpos >= off[sidx + 1] - off[sidx]) { fprintf(stderr, "hit %zu out of range\n", k); return 2; }
        const uint8_t *q = frames + ((size_t)read * 6 + frame) * FP, *d = H.res.data() + off[sidx];
        McGapTask g; memset(&g, 0, sizeof g);
        const int rc = mc_eval_seed_core(T, q, qlen, frame, qpos, d, (int)(off[sidx + 1] - off[sidx]), dpos, sidx, seedlen, nkey, &g);
        int32_t *o = res.data() + 24 * k;
        o[0] = rc;
        if (rc) { o[1] = (int32_t)g.sidx; o[2] = g.qp; o[3] = g.dp; o[4] = g.L; o[5] = g.qfwd; o[6] = g.qbwd; o[7] = g.score; o[8] = g.nmatch; }
        if (rc == 1) {
            McHsp hs; memset(&hs, 0, sizeof hs);
            o[9] = mc_make_hsp(T, L, frame, g, g.qfwd, g.qfwd, g.qbwd, g.qbwd, g.score, g.nmatch, g.qfwd + g.L + g.qbwd, 0, 0, &hs) ? 1 : 0;
            loge[k] = g.score >= 0 && g.score < MC_SMAX ? T.loge_r[g.score] : 0.0;
            if (o[9]) { const int32_t v[12] = {hs.score, hs.frame, hs.alnlen, hs.mism, hs.gaps, hs.nmatch, hs.qaas, hs.qaae, hs.ds, hs.de, hs.qnts, hs.qnte}; memcpy(o + 10, v, sizeof v); }
        }
    }
    out.put(res); out.put(loge);

    std::vector<int32_t> counts, ranges;
    for (size_t k = 0; k < nrows; k++) {
        if (rows[k] < 0 || rows[k] >= nreads * 6) { fprintf(stderr, "row %zu out of range\n", k); return 2; }
        const int frame = rows[k] % 6, qlen = (L - frame % 3) / 3;
        Ranges e = {&ranges, 0};
        McSeedCount sc = {0, 0, 0};
        mc_enumerate_seeds(T, X, frames + (size_t)rows[k] * FP, qlen, e, &sc);
        counts.push_back(e.n);
    }
    out.put(counts); out.put(ranges); out.put(H.post); out.put(H.bstart);
    sections_write(argv[2], out);
    return 0;
}
