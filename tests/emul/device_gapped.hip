// tests/emul/device_gapped.hip - the seven kernels of the gapped stage (csrc/k_gapped.h) on task records and flanks built to reach
// their edges: a stand-alone program that includes the library's kernel headers in mc_hip.hip's order - it compiles the text the
// library compiles and copies none of it - and links neither the library nor the reader.
//   device_gapped VERB IN OUT      (files of sections: order_io.h; tests/gapped_cases.py writes IN, tests/test_gpu_gapped_units.py reads OUT)
// IN, every verb but sort: 0 three int32 (read length, FP, reads), 1 the frames (reads x 6 x FP dense codes), 2 the subjects' letters,
// 3 their offsets, 4 the McGapTask records; the verb's own sections follow.  The tables are built on the host as tests/emul/mc_emul.cpp
// builds them: the index builder on the subjects, mc_fill_tables at the read length.
//   dedupe   5 one uint32: the table's slots.  k_gap_dedupe alone.
//            OUT: leader, key, item (2 n each), the counters.
//   sort     IN: 0 the number of sets, then per set keys, items, two uint32 (n, cap).  k_gap_sort_hist, k_gap_sort_scan,
//            k_gap_sort_scatter (mc_gap_sort_launch).
//            OUT, per set: the output list (cap entries over a fill of 0xFF), the histogram as the scatter leaves it, the 16 guard words behind the list.
//   extend   5 the number of cases, then per case the item list and three int32: the grids of the three launches, 0 = the product's
//            formula.  k_gapped_lds<MC_GAP_WIN, 64, MC_GAP_REFILL>, k_gapped_lds<MC_GAP_WIN2, MC_GAP_LANES2, 1>, k_gapped
//            (mc_gap_extend_launch), on fresh counters, lists and results for every case.
//            OUT, per case: fout with 16 guard records on either side (all over a fill of 0xEE), the two retry lists, the counters.
//   chain    5 two uint32 (table slots, capacity of the HSP pool), 6 one double: the bit score from which an HSP makes its read a
//            candidate.  The whole stage: dedupe, sort, extend and k_gap_emit (mc_gap_launch).
//            OUT: the HSP pool, hkeys, hplace, low, cand, the counters, leader, fout, the guards behind pool, hkeys and hplace,
//            loge_r, bits_r, loge_thr.
// Every launch goes through csrc/mc_stages.h, the functions the library's own stage B calls: the grids, the counter slots and the
// order of the kernels under test are the product's, not a copy of them.
// A case that is no legal state of the pipeline is refused with status 2 before anything is launched; every HIP call is checked: an
// error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "k_translate_seg.h"
#include "k_enumerate.h"
#include "k_eval_seeds.h"
#include "k_gapped.h"
#include "mc_stages.h"

#include <set>
#include <tuple>

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

#define REFUSE(...) do { fprintf(stderr, "input: " __VA_ARGS__); fprintf(stderr, "\n"); exit(2); } while (0)

static int sort_verb(Sections &in, Sections &out)
{
    size_t nc;
    const uint32_t *count = in.take<uint32_t>(&nc);
    if (nc != 1 || count[0] > 1000) REFUSE("the number of sets");
    for (uint32_t c = 0; c < count[0]; c++) {
        size_t nk, ni, nm;
        const uint32_t *key = in.take<uint32_t>(&nk), *item = in.take<uint32_t>(&ni), *meta = in.take<uint32_t>(&nm);
        if (nm != 2 || nk != ni) REFUSE("set %u: keys, items or (n, cap) malformed", c);
        const uint32_t n = meta[0], cap = meta[1];
        if (cap > (1u << 28) || (n <= cap && n > nk)) REFUSE("set %u: n = %u of %zu keys, cap %u", c, n, nk, cap);
        for (size_t i = 0; i < nk; i++) if (key[i] < 1 || key[i] > MC_GS_BINS - 1) REFUSE("set %u: key %u", c, key[i]);
        Dev<uint32_t> d_key(key, nk), d_item(item, ni), d_n(&n, 1), d_hist(MC_GS_BINS), d_out(cap, 0xFF);
        CK_STAGE(mc_gap_sort_launch(d_key, d_item, d_n, cap, d_hist, d_out, nullptr));
        out.put(d_out.host()); out.put(d_hist.host()); out.put(d_out.pad());
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: device_gapped dedupe|sort|extend|chain IN OUT\n"); return 2; }
    const std::string verb = argv[1];
    Sections in = sections_read(argv[2]), out;
    if (verb == "sort") { sort_verb(in, out); sections_write(argv[3], out); return 0; }
    if (verb != "dedupe" && verb != "extend" && verb != "chain") REFUSE("no verb %s", verb.c_str());

    // ---- the world: a legal state of the pipeline, or nothing is launched
    size_t nmeta, nfr, ntext, noff, ntasks;
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const uint8_t *frames = in.take<uint8_t>(&nfr);
    const char *text = (const char *)in.take<uint8_t>(&ntext);
    const uint32_t *off = in.take<uint32_t>(&noff);
    const McGapTask *tasks = in.take<McGapTask>(&ntasks);
    if (nmeta != 3) REFUSE("read length, FP, reads");
    const int L = meta[0], FP = meta[1], nreads = meta[2];
    if (L < 18 || L > 3 * MC_MAXAA || FP < L / 3 + 2 || nreads < 1 || nreads > (1 << 21) - 1 || nfr != (size_t)nreads * 6 * (size_t)FP) REFUSE("reads of %d bases, FP %d, %d reads, %zu frame bytes", L, FP, nreads, nfr);
    if (noff < 2 || noff - 1 > 32767 || off[0] != 0 || off[noff - 1] != ntext) REFUSE("offsets malformed");
    const int nseq = (int)(noff - 1);
    for (int s = 0; s < nseq; s++) if (off[s + 1] <= off[s] || off[s + 1] - off[s] > MC_GAP_W - 8) REFUSE("subject %d has %lld residues", s, (long long)off[s + 1] - (long long)off[s]);
    for (size_t i = 0; i < ntext; i++) if (text[i] == 0) REFUSE("a NUL among the subjects' letters");
    for (int r = 0; r < nreads; r++)
        for (int f = 0; f < 6; f++) {
            const uint8_t *row = frames + ((size_t)r * 6 + f) * FP;
            const int qlen = (L - f % 3) / 3;
            for (int i = 0; i < FP; i++) if (row[i] > MC_INV || (i >= qlen && row[i] != MC_INV)) REFUSE("read %d frame %d residue %d is %d", r, f, i, row[i]);
        }
    if (ntasks < 1 || ntasks >= (1u << 27) - 2) REFUSE("%zu tasks", ntasks);
    typedef std::tuple<uint32_t, uint32_t, int, int, int, int> Seg;
    std::set<Seg> segs;
    auto flank = [&](const McGapTask &g, int side, int &n1, int &n2) {
        const int frame = (int)(g.chrono >> 25), qlen = (L - frame % 3) / 3, dlen = (int)(off[g.sidx + 1] - off[g.sidx]);
        if (side == 0) { n1 = qlen - (g.qfwd + g.qp + g.L); n2 = dlen - (g.qfwd + g.dp + g.L); } else { n1 = g.qp - g.qbwd; n2 = g.dp - g.qbwd; }
        return n1 > 2 && n2 > 2;
    };
    for (size_t p = 0; p < ntasks; p++) {
        const McGapTask &g = tasks[p];
        if (g.read == MC_TASK_NONE) continue;
        const int frame = (int)(g.chrono >> 25);
        if (g.read >= (uint32_t)nreads || g.sidx >= (uint32_t)nseq || frame > 5) REFUSE("task %zu: read %u subject %u frame %d", p, g.read, g.sidx, frame);
        const int qlen = (L - frame % 3) / 3, dlen = (int)(off[g.sidx + 1] - off[g.sidx]);
        if (g.L < 1 || g.qfwd < 0 || g.qbwd < 0 || g.qp - g.qbwd < 0 || g.dp - g.qbwd < 0 || g.qp + g.L + g.qfwd > qlen || g.dp + g.L + g.qfwd > dlen || g.score < 0 || g.score >= 2048 || g.nmatch < 0)
            REFUSE("task %zu: the segment leaves its frame or its subject", p);
        segs.insert(Seg(g.read, g.sidx, frame, g.qp - g.qbwd, g.dp - g.qbwd, g.qp + g.L + g.qfwd));
    }
    std::vector<std::string> seqs(nseq), names(nseq);
    std::vector<const char *> np(nseq), sp(nseq);
    for (int s = 0; s < nseq; s++) { seqs[s].assign(text + off[s], text + off[s + 1]); names[s] = "s" + std::to_string(s); np[s] = names[s].c_str(); sp[s] = seqs[s].c_str(); }
    McHostIndex H; std::string err;
    if (!mc_build_index(H, np.data(), sp.data(), nseq, err)) REFUSE("%s", err.c_str());
    if (memcmp(H.off.data(), off, noff * 4)) REFUSE("the index builder's offsets differ");
    static McTables T;
    mc_fill_tables(T, H, L, 1.0);
    const uint32_t n = (uint32_t)ntasks;

    // ---- on the device.  The residues lie 64 bytes inside their array, as mc_set_db places them (k_gapped_lds reads 16 bytes around a flank's first residues)
    std::vector<uint8_t> res(H.res.size() + 128, (uint8_t)MC_INV);
    memcpy(res.data() + 64, H.res.data(), H.res.size());
    Dev<uint8_t> d_res(res.data(), res.size()), d_frames(frames, nfr);
    Dev<uint32_t> d_off(off, noff), d_counters(C_N), d_leader(n, 0xFF), d_key(2 * (size_t)n), d_item(2 * (size_t)n), d_list(2 * (size_t)n), d_hist(MC_GS_BINS);
    Dev<McGapTask> d_tasks(tasks, ntasks);
    Dev<McTables> d_T(&T, 1);
    McIndex X; memset(&X, 0, sizeof X);
    X.res = d_res.p + 64; X.off = d_off; X.nseq = nseq;

    // what the launch functions of csrc/mc_stages.h are given: the run, and every array of the stage as a pointer of its own
    McRun R = {d_T, X, nullptr, nullptr, L, FP};
    Dev<McGapCell> d_ws((size_t)MC_GAP_THREADS_FULL * MC_GAP_W);     // (full-size rows for all of the last launch's threads: 460 MB)
    McGapBufs B = {};
    B.frames = d_frames; B.gaps = d_tasks; B.counters = d_counters; B.leader = d_leader; B.key = d_key; B.item = d_item; B.list = d_list; B.hist = d_hist; B.ws_full = d_ws;
    auto table = [&](uint32_t slots) {
        if (slots < 2 || (slots & (slots - 1)) || slots > (1u << 27) || slots <= segs.size()) REFUSE("%u table slots for %zu distinct segments: a power of two with a free slot", slots, segs.size());
        return slots;
    };

    if (verb == "dedupe") {
        size_t ns;
        const uint32_t *slots = in.take<uint32_t>(&ns);
        if (ns != 1) REFUSE("the table's slots");
        Dev<unsigned long long> d_tab(table(slots[0]));
        B.tab = d_tab; B.slots = slots[0];
        CK_STAGE(mc_gap_dedupe_launch(R, B, n, nullptr));
        out.put(d_leader.host()); out.put(d_key.host()); out.put(d_item.host()); out.put(d_counters.host());
    } else if (verb == "extend") {
        size_t nc;
        const uint32_t *count = in.take<uint32_t>(&nc);
        if (nc != 1 || count[0] > 1000) REFUSE("the number of cases");
        for (uint32_t c = 0; c < count[0]; c++) {
            size_t nl, ng;
            const uint32_t *list = in.take<uint32_t>(&nl);
            const int32_t *grid = in.take<int32_t>(&ng);
            if (ng != 3 || grid[0] < 0 || grid[1] < 0 || grid[2] < 0 || nl > 2 * (size_t)n) REFUSE("case %u: item list or grids malformed", c);
            std::set<uint32_t> seen;
            for (size_t k = 0; k < nl; k++) {
                int n1, n2;
                if (list[k] >= 2 * n || tasks[list[k] >> 1].read == MC_TASK_NONE || !flank(tasks[list[k] >> 1], (int)(list[k] & 1), n1, n2) || !seen.insert(list[k]).second) REFUSE("case %u: item %zu (%u) is no flank to extend, or listed twice", c, k, list[k]);
            }
            const McGapGrids G = mc_gap_grids(n, grid);                // (a grid of 0: the product's)
            if (G.lds > MC_GAP_GRID_MAX || G.lds2 > MC_GAP_GRID2 || G.full > MC_GAP_GRID_FULL) REFUSE("grids %u, %u, %u", G.lds, G.lds2, G.full);
            const uint32_t nitems = (uint32_t)nl;
            Dev<McFlankOut> d_fout(2 * (size_t)n + 16, 0xEE);          // (fout lies 16 records inside its array)
            Dev<uint32_t> d_retry(2 * (size_t)n + 1, 0xFF), d_retry2(2 * (size_t)n + 1, 0xFF);
            CK(hipMemset(d_counters.p, 0, C_N * sizeof(uint32_t)));
            if (nl) CK(hipMemcpy(d_list.p, list, nl * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(d_counters.p + C_ITEMS, &nitems, 4, hipMemcpyHostToDevice));
            B.fout = d_fout.p + 16; B.retry = d_retry; B.retry2 = d_retry2;
            CK_STAGE(mc_gap_extend_launch(R, B, d_list, G, nullptr));
            out.put(d_fout.host()); { std::vector<McFlankOut> p = d_fout.pad(); out.s.back().insert(out.s.back().end(), (const uint8_t *)p.data(), (const uint8_t *)(p.data() + p.size())); }
            out.put(d_retry.host()); out.put(d_retry2.host()); out.put(d_counters.host());
        }
    } else {
        size_t ns, nb;
        const uint32_t *sc = in.take<uint32_t>(&ns);
        const double *bits = in.take<double>(&nb);
        if (ns != 2 || nb != 1 || sc[1] > (1u << 24)) REFUSE("table slots, pool capacity, candidate score");
        const uint32_t cap_hsps = sc[1];
        static McClassPars P; memset(&P, 0, sizeof P);
        P.nfam = 1; P.read_len = L; P.min_score[0] = bits[0]; P.min_cov[0] = 0.0; P.max_aaid[0] = 1000; P.aln_stat[0] = 0;
        std::vector<int32_t> fam(nseq, 0);
        Dev<McClassPars> d_P(&P, 1);
        Dev<int32_t> d_fam(fam.data(), fam.size());
        Dev<McHsp> d_hsps(cap_hsps, 0xEE);
        Dev<uint64_t> d_hkeys(cap_hsps, 0xEE), d_hplace(cap_hsps, 0xEE);
        Dev<uint8_t> d_low((size_t)nreads), d_cand((size_t)nreads);
        Dev<unsigned long long> d_tab(table(sc[0]));
        Dev<McFlankOut> d_fout(2 * (size_t)n + 16, 0xEE);
        Dev<uint32_t> d_retry(2 * (size_t)n + 1, 0xFF), d_retry2(2 * (size_t)n + 1, 0xFF);
        R.P = d_P; R.fam = d_fam;
        B.tab = d_tab; B.slots = sc[0]; B.fout = d_fout.p + 16; B.retry = d_retry; B.retry2 = d_retry2;
        B.hsps = d_hsps; B.cap_hsps = cap_hsps; B.cand = d_cand; B.hkeys = d_hkeys; B.low = d_low; B.hplace = d_hplace;
        CK_STAGE(mc_gap_launch(R, B, n, nullptr));
        out.put(d_hsps.host()); out.put(d_hkeys.host()); out.put(d_hplace.host()); out.put(d_low.host()); out.put(d_cand.host()); out.put(d_counters.host());
        out.put(d_leader.host()); out.put(d_fout.host());
        out.put(d_hsps.pad()); out.put(d_hkeys.pad()); out.put(d_hplace.pad());
        out.put(T.loge_r, MC_SMAX); out.put(T.bits_r, MC_SMAX); out.put(&T.loge_thr, 1);
    }
    sections_write(argv[3], out);
    return 0;
}
