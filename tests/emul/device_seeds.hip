// tests/emul/device_seeds.hip - the kernels of the seed stage (csrc/k_enumerate.h, csrc/k_eval_seeds.h) on frames, subjects and seed hits
// built to reach their edges: a stand-alone program that includes the library's kernel headers in mc_hip.hip's order - it compiles the
// text the library compiles and copies none of it - and links neither the library nor the reader.
//   device_seeds VERB IN OUT      (files of sections: order_io.h; tests/seed_cases.py writes IN, tests/test_gpu_seeds_units.py reads OUT)
// IN, every verb: 0 three int32 (read length, FP, reads), 1 the frames (reads x 6 x FP dense codes), 2 the subjects' letters, 3 their
// offsets; the verb's own sections follow.  The index and the tables are built on the host as tests/emul/mc_emul.cpp builds them: the
// index builder on the subjects, mc_fill_tables at the read length.  Residues and frames lie 64 bytes inside their arrays, the room
// filled with MC_INV, as the library lays them out.
//   post8      k_post8 (mc_post8_launch) on the index's postings.
//              OUT: post8 (4 words per posting), the 16 guard words behind it, the postings, the residues (dense, without the room).
//   eval       4 the hits (seven int32: read, frame, qpos, sidx, dpos, seedlen, nkey), 5 the places of the real records in the task
//              pool (uint32, ascending), 6 the hit of each (int32), 7 seven uint32: the pool's records (every other one is a padding
//              record, read = MC_TASK_NONE), ranges (1: posting indices for k_eval_seeds<true>, 0: MC_TASK_W3 / MC_TASK_READ records for
//              <false>), cap_hsps, cap_gaps, what *ntasks_p says (0xFFFFFFFF: the pool's records), cand (0: nullptr), 0; 8 one double:
//              the bit score from which an HSP makes its read a candidate.  A record's chrono word is MC_CHRONO(frame, qpos, 0, 0) with the
//              record's place among the real ones in its low 17 bits.  k_post8, then k_eval_seeds (mc_eval_seeds_launch).
//              OUT: the HSP pool, hkeys, hplace (cap_hsps over a fill of 0xEE), the gap tasks (cap_gaps), low, cand, the counters, the
//              guards behind hsps, hkeys, hplace and gaps.
//   enumerate  4 two uint32: the kernel (McSeedKernel: 0 k_enumerate, 1 k_enumerate_q, 2 k_enumerate_count), cap_tasks.
//              OUT: the task pool (cap_tasks over a fill of 0xEE), the counters, the guard behind the pool, the postings, the offsets.
// Every launch goes through csrc/mc_stages.h, the functions the library's own stage A calls.  A case that is no legal state of the
// pipeline is refused with status 2 before anything is launched; every HIP call is checked: an error is printed and ends the program
// with status 3 at once.
#include "mc_hip_common.h"
#include "k_translate_seg.h"
#include "k_enumerate.h"
#include "k_eval_seeds.h"
#include "k_gapped.h"
#include "mc_stages.h"

#include <map>

#include "order_io.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

#define REFUSE(...) do { fprintf(stderr, "input: " __VA_ARGS__); fprintf(stderr, "\n"); exit(2); } while (0)

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: device_seeds post8|eval|enumerate IN OUT\n"); return 2; }
    const std::string verb = argv[1];
    if (verb != "post8" && verb != "eval" && verb != "enumerate") REFUSE("no verb %s", verb.c_str());
    Sections in = sections_read(argv[2]), out;

    // ---- the world: a legal state of the pipeline, or nothing is launched
    size_t nmeta, nfr, ntext, noff;
    const int32_t *meta = in.take<int32_t>(&nmeta);
    const uint8_t *frames = in.take<uint8_t>(&nfr);
    const char *text = (const char *)in.take<uint8_t>(&ntext);
    const uint32_t *off = in.take<uint32_t>(&noff);
    if (nmeta != 3) REFUSE("read length, FP, reads");
    const int L = meta[0], FP = meta[1], nreads = meta[2];
    // (the shortest read: a frame of ten residues, the shortest that can hold a seed of every kind)
    if (L < 30 || L > 3 * MC_MAXAA || FP != (((L / 3 + 2) + 3) & ~3) || nreads < 1 || nreads > (1 << 21) - 1 || nfr != (size_t)nreads * 6 * (size_t)FP) REFUSE("reads of %d bases, FP %d, %d reads, %zu frame bytes", L, FP, nreads, nfr);
    if (noff < 2 || noff - 1 > 32767 || off[0] != 0 || off[noff - 1] != ntext) REFUSE("offsets malformed");
    const int nseq = (int)(noff - 1);
    for (int s = 0; s < nseq; s++) if (off[s + 1] <= off[s] || off[s + 1] - off[s] > 2047) REFUSE("subject %d has %lld residues", s, (long long)off[s + 1] - (long long)off[s]);
    for (size_t i = 0; i < ntext; i++) if (text[i] == 0) REFUSE("a NUL among the subjects' letters");
    for (int r = 0; r < nreads; r++)
        for (int f = 0; f < 6; f++) {
            const uint8_t *row = frames + ((size_t)r * 6 + f) * FP;
            const int qlen = (L - f % 3) / 3;
            for (int i = 0; i < FP; i++) if (row[i] > MC_INV || (i >= qlen && row[i] != MC_INV)) REFUSE("read %d frame %d residue %d is %d", r, f, i, row[i]);
        }
    std::vector<std::string> seqs(nseq), names(nseq);
    std::vector<const char *> np(nseq), sp(nseq);
    for (int s = 0; s < nseq; s++) { seqs[s].assign(text + off[s], text + off[s + 1]); names[s] = "s" + std::to_string(s); np[s] = names[s].c_str(); sp[s] = seqs[s].c_str(); }
    McHostIndex H; std::string err;
    if (!mc_build_index(H, np.data(), sp.data(), nseq, err)) REFUSE("%s", err.c_str());
    if (memcmp(H.off.data(), off, noff * 4)) REFUSE("the index builder's offsets differ");
    if (H.res.size() >= MC_TASK_ABS_LIMIT || H.post.empty() || H.post.size() >= (1u << 26)) REFUSE("%zu residues, %zu postings", H.res.size(), H.post.size());
    static McTables T;
    mc_fill_tables(T, H, L, 1.0);
    const uint32_t npost = (uint32_t)H.post.size();

    // ---- the verb's own sections
    size_t nh = 0, nplace = 0, nwhich = 0, npar = 0, nb = 0;
    const int32_t *hits = nullptr, *which = nullptr;
    const uint32_t *place = nullptr, *par = nullptr;
    const double *bits = nullptr;
    uint32_t n = 0, cap_hsps = 0, cap_gaps = 0, cap_tasks = 0;
    bool ranges = false;
    std::vector<McSeedTask> rec;
    if (verb == "eval") {
        hits = in.take<int32_t>(&nh);
        place = in.take<uint32_t>(&nplace);
        which = in.take<int32_t>(&nwhich);
        par = in.take<uint32_t>(&npar);
        bits = in.take<double>(&nb);
        if (nh % 7 || nplace != nwhich || npar != 7 || nb != 1) REFUSE("hits, places or parameters malformed");
        nh /= 7;
        n = par[0]; cap_hsps = par[2]; cap_gaps = par[3]; ranges = par[1] != 0;
        if (n > (1u << 24) || par[1] > 1 || cap_hsps > (1u << 22) || cap_gaps > (1u << 22) || nplace > n || nplace >= (1u << 17) || (par[4] != 0xFFFFFFFFu && par[4] != n + 1) || par[5] > 1) REFUSE("%u records, caps %u, %u", n, cap_hsps, cap_gaps);
        std::map<uint32_t, uint32_t> index_of;
        for (uint32_t i = 0; i < npost; i++) index_of[H.post[i]] = i;
        rec.resize(nplace);
        for (size_t k = 0; k < nplace; k++) {
            if (place[k] >= n || (k && place[k] <= place[k - 1]) || which[k] < 0 || (size_t)which[k] >= nh) REFUSE("record %zu: place %u, hit %d", k, place[k], which[k]);
            const int32_t *h = hits + 7 * (size_t)which[k];
            const int read = h[0], frame = h[1], qpos = h[2], sidx = h[3], dpos = h[4], seedlen = h[5], nkey = h[6];
            if (read < 0 || read >= nreads || frame < 0 || frame > 5 || sidx < 0 || sidx >= nseq || seedlen < 6 || seedlen > 10 || nkey != (seedlen == 10 ? 4 : seedlen - 6)) REFUSE("hit %d: out of range", which[k]);
            const int qlen = (L - frame % 3) / 3, dlen = (int)(off[sidx + 1] - off[sidx]);
            if (qpos < 0 || qpos + seedlen > qlen || dpos < 0 || dpos + 6 > dlen) REFUSE("hit %d: the seed leaves its frame or its subject's postings", which[k]);
            const uint8_t *q = frames + ((size_t)read * 6 + frame) * FP, *d = H.res.data() + off[sidx];
            int miss = 0;
            for (int i = 0; i < seedlen && dpos + i < dlen; i++)
                if (T.grp[q[qpos + i]] == MC_INVGRP || T.grp[q[qpos + i]] != T.grp[d[dpos + i]]) { miss++; if (seedlen != 10 || i < 3 || i > 6) miss = 99; }
            if (miss > 1) REFUSE("hit %d: the seed does not match", which[k]);
            const uint32_t posting = ((uint32_t)sidx << 11) | (uint32_t)dpos;
            auto it = index_of.find(posting);
            if (it == index_of.end()) REFUSE("hit %d: (%d, %d) is no posting", which[k], sidx, dpos);
            const uint32_t abs = off[sidx] + (uint32_t)dpos;
            McSeedTask &t = rec[k];
            t.chrono = MC_CHRONO(frame, qpos, 0, 0) | (uint32_t)k;
            if (ranges) { t.read = (uint32_t)read; t.posting = it->second; t.seedlen_nkey = MC_TASK_W3(0, seedlen, nkey); }
            else { t.read = MC_TASK_READ(read, dlen - dpos); t.posting = posting; t.seedlen_nkey = MC_TASK_W3(abs, seedlen, nkey); }
        }
    } else if (verb == "enumerate") {
        par = in.take<uint32_t>(&npar);
        if (npar != 2 || par[0] > 2 || par[1] > (1u << 24)) REFUSE("kernel, cap_tasks");
        if (par[0] != MC_SEED_PLAIN && (T.freq_thr != 0 || H.rec.empty())) REFUSE("the position-parallel seed kernels need a threshold of 0 and the bucket records");
        cap_tasks = par[1];
    }

    // ---- on the device
    std::vector<uint8_t> res(H.res.size() + 128, (uint8_t)MC_INV), fr(nfr + 64 + 4096, (uint8_t)MC_INV);
    memcpy(res.data() + 64, H.res.data(), H.res.size());
    memcpy(fr.data() + 64, frames, nfr);
    Dev<uint8_t> d_res(res.data(), res.size()), d_frames(fr.data(), fr.size());
    Dev<uint32_t> d_off(off, noff), d_post(H.post.data(), H.post.size()), d_counters(C_N);
    Dev<unsigned long long> d_post8((size_t)npost * MC_POST_WORDS, 0xEE);
    Dev<McTables> d_T(&T, 1);
    McIndex X; memset(&X, 0, sizeof X);
    X.res = d_res.p + 64; X.off = d_off; X.post = d_post; X.post8 = d_post8; X.nseq = nseq;
    CK_STAGE(mc_post8_launch(d_post, d_off, X.res, npost, d_post8, nullptr));

    if (verb == "post8") {
        out.put(d_post8.host()); out.put(d_post8.pad()); out.put(H.post); out.put(H.res);
    } else if (verb == "eval") {
        static McClassPars P; memset(&P, 0, sizeof P);
        P.nfam = 1; P.read_len = L; P.min_score[0] = bits[0]; P.min_cov[0] = 0.0; P.max_aaid[0] = 1000; P.aln_stat[0] = 0;
        std::vector<int32_t> fam(nseq, 0);
        Dev<McClassPars> d_P(&P, 1);
        Dev<int32_t> d_fam(fam.data(), fam.size());
        Dev<McSeedTask> d_tasks(n, 0xFF);                             // (every record a padding record: read = MC_TASK_NONE)
        for (size_t k = 0; k < nplace; k++) CK(hipMemcpy(d_tasks.p + place[k], &rec[k], sizeof(McSeedTask), hipMemcpyHostToDevice));
        Dev<McHsp> d_hsps(cap_hsps, 0xEE);
        Dev<uint64_t> d_hkeys(cap_hsps, 0xEE), d_hplace(cap_hsps, 0xEE);
        Dev<McGapTask> d_gaps(cap_gaps, 0xEE);
        Dev<uint8_t> d_low((size_t)nreads), d_cand((size_t)nreads);
        const uint32_t says = par[4] == 0xFFFFFFFFu ? n : par[4];
        CK(hipMemcpy(d_counters.p + C_TASKS, &says, 4, hipMemcpyHostToDevice));
        McRun R = {d_T, X, d_P, d_fam, L, FP};
        McSeedBufs B = {};
        B.frames = d_frames.p + 64; B.tasks = d_tasks; B.cap_tasks = n; B.counters = d_counters;
        B.hsps = d_hsps; B.cap_hsps = cap_hsps; B.gaps = d_gaps; B.cap_gaps = cap_gaps; B.cand = par[5] ? d_cand.p : nullptr; B.hkeys = d_hkeys; B.low = d_low; B.hplace = d_hplace;
        CK_STAGE(mc_eval_seeds_launch(R, B, ranges, nullptr));
        out.put(d_hsps.host()); out.put(d_hkeys.host()); out.put(d_hplace.host()); out.put(d_gaps.host()); out.put(d_low.host()); out.put(d_cand.host()); out.put(d_counters.host());
        out.put(d_hsps.pad()); out.put(d_hkeys.pad()); out.put(d_hplace.pad()); out.put(d_gaps.pad());
    } else {
        Dev<uint32_t> d_bstart(H.bstart.data(), H.bstart.size()), d_bitmap(H.bitmap.data(), H.bitmap.size()), d_filt(H.filt.data(), H.filt.size()), d_wild(H.wild.data(), H.wild.size()), d_pair(H.pair.data(), H.pair.size());
        Dev<uint16_t> d_keys(H.keys.data(), H.keys.size());
        Dev<McBucketRec> d_rec(H.rec.data(), H.rec.size());
        Dev<unsigned long long> d_rt(H.rt.data(), H.rt.size()), d_stats(S_N);
        X.bstart = d_bstart; X.keys = d_keys; X.rec = H.rec.empty() ? nullptr : d_rec.p; X.filt = d_filt; X.wild = d_wild; X.pair = d_pair; X.rt = d_rt; X.rt_mask = H.rt_mask;
        Dev<McSeedTask> d_tasks(cap_tasks, 0xEE);
        McRun R = {d_T, X, nullptr, nullptr, L, FP};
        McSeedBufs B = {};
        B.frames = d_frames.p + 64; B.bitmap = d_bitmap; B.tasks = d_tasks; B.cap_tasks = cap_tasks; B.counters = d_counters; B.stats = d_stats;
        CK_STAGE(mc_enumerate_launch(R, B, nreads, (McSeedKernel)par[0], nullptr));
        out.put(d_tasks.host()); out.put(d_counters.host()); out.put(d_tasks.pad()); out.put(H.post); out.put(H.off);
    }
    sections_write(argv[3], out);
    return 0;
}
