// mc_stages.h - the one owner of the search pipeline's launches: every grid, LDS size, hipFuncSetAttribute and fork / join of the
// stages A0, A1, B, C and D, as plain functions over raw device pointers, a stream and events, 0 / -1 through HIPCK.  mc_hip.hip's
// stage_a .. stage_d keep the sequencing (counters on the host, overflow, the events that delimit the stage times) and fill the pointer
// structs below from the handle's pools (carve_*, beside McCtx); tests/emul/device_gapped.hip and device_order.hip fill them from
// arrays of their own and launch through the same functions.  Nothing here knows the handle, the pools, or that two of the pointers
// it is given alias in the product.
#pragma once
#include "k_translate_seg.h"
#include "k_enumerate.h"
#include "k_eval_seeds.h"
#include "k_gapped.h"
#include "k_order.h"
#include "k_finish.h"

// ---- Shapes: the grid, block and LDS sizes both sides need by name -----------------------------------------------------------------
static constexpr uint32_t MC_CUS = 256u;                            // the grids of the persistent kernels are multiples of the CUs
static constexpr int MC_GAP_THREADS_FULL = 16 * 1024;               // full-size DP rows for the last-resort launch (460 MB of McGapCell)
static constexpr uint32_t MC_GAP_SORT_BLOCKS = 512u;                // k_gap_sort_hist, k_gap_sort_scatter
static constexpr uint32_t MC_GAP_GRID_MAX = MC_CUS * 8u;            // k_gapped_lds<MC_GAP_WIN>: 8 waves per CU
static constexpr uint32_t MC_GAP_GRID2 = MC_CUS * 4u;               // k_gapped_lds<MC_GAP_WIN2>
static constexpr uint32_t MC_GAP_GRID_FULL = (uint32_t)MC_GAP_THREADS_FULL / 128u;   // k_gapped
static constexpr uint32_t MC_BIN_BLOCKS = MC_CUS * 8u;              // k_bin_count, k_bin_scatter, k_order_copy
// the LDS of k_order_heavy<NT, CAP> (and of whoever stages mc_group_mergesort's two buffers): 18 bytes per item
static inline size_t mc_order_heavy_lds(uint32_t cap) { return (size_t)cap * 18; }
// k_finish_heavy<MAXN>: the items and the three index arrays of mc_wave_std_sort
static inline size_t mc_finish_heavy_lds(int maxn) { return (size_t)maxn * 16 + 3 * (size_t)(maxn + 2) * 2; }
// k_heap_lanes: MC_MAX_M8 + 2 words per lane, transposed
static inline size_t mc_heap_lanes_lds() { return (size_t)(MC_MAX_M8 + 2) * 64 * 4; }
// k_finish<TPB, ITEMS, .>: a thread's own stretch of ITEMS items and a spare one
static inline size_t mc_finish_lds(int tpb, int items) { return (size_t)tpb * (items * 16 + 16); }

// what every stage reads of the run: the tables, the index, the classification parameters, the read length and the frames' pitch
struct McRun { const McTables *T; McIndex X; const McClassPars *P; const int32_t *fam; int L, FP; };
// two side streams and the events of a fork from, and two joins into, the stage's own stream (stages C and D)
struct McFork { hipStream_t side, side2; hipEvent_t fork, join, join2; };

// ---- A0: translation + SEG ---------------------------------------------------------------------------------------------------------
// k_translate_seg of n reads of L bases at `reads` into `frames`, in st.  staged (if given) receives the form that was launched, narrow
// (if given) whether it was the instantiation for frames of at most MC_NARROW_MAXAA residues.
static int mc_translate_launch(const McTables *T, const uint64_t *segtab, const uint8_t *reads, int L, int FP, int64_t n, uint8_t *frames, hipStream_t st, int *staged_out = nullptr,
                               int *narrow_out = nullptr)
{
    const size_t lds_rest = (size_t)MC_TS_NLNF(FP) * 8 + (size_t)MC_TS_THREADS * MC_TS_STRIDE(FP);
    const size_t lds_staged = (size_t)MC_TS_STAGE(L) + lds_rest, lds_direct = (size_t)MC_TS_STAGE(0) + lds_rest;
    static const int ts_force = getenv("MC_TS_STAGED") ? atoi(getenv("MC_TS_STAGED")) : -1;
    const size_t cu_lds = 160 * 1024 - 1024;                      // (static LDS of the kernel and allocation granules)
    const bool staged = ts_force >= 0 ? ts_force != 0 : cu_lds / lds_staged >= cu_lds / lds_direct;   // staging stays while it does not cost a resident workgroup
    const size_t lds = staged ? lds_staged : lds_direct;
    if (staged_out) *staged_out = staged ? 1 : 0;
    const unsigned ts_blocks = (unsigned)((n + MC_TS_READS - 1) / MC_TS_READS);
    // Reads up to 191 bp: no frame has more than L / 3 <= MC_NARROW_MAXAA = 63 residues, so every position and every count of the SEG bit
    // sets is below 64 (McBits64 never shifts by 64) and the work list holds at most 63 / 13 = 4 entries.  The choice between staged and
    // direct stays the one above, made from the wide layout's sizes; the narrow launch only asks for less LDS (under 11 KB: no attribute).
    const bool narrow = L / 3 <= MC_NARROW_MAXAA;
    static_assert(MC_NARROW_MAXAA <= 63 && MC_SEG_STK_NARROW * 13 + 12 >= MC_NARROW_MAXAA, "the narrow form's one-word bit sets and four-entry work list");
    if (narrow_out) *narrow_out = narrow ? 1 : 0;
    if (narrow) {
        const size_t lds_n = (size_t)MC_TS_STAGE(staged ? L : 0) + (size_t)MC_TS_NLNF(FP) * 8 + MC_TS_ROWS_N(FP);
        if (staged) k_translate_seg<true, true><<<dim3(ts_blocks), dim3(MC_TS_THREADS), lds_n, st>>>(T, reads, L, n, frames, FP, segtab);
        else k_translate_seg<false, true><<<dim3(ts_blocks), dim3(MC_TS_THREADS), lds_n, st>>>(T, reads, L, n, frames, FP, segtab);
    } else if (staged) {
        if (lds > 48 * 1024) HIPCK(hipFuncSetAttribute((const void *)k_translate_seg<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_translate_seg<true><<<dim3(ts_blocks), dim3(MC_TS_THREADS), lds, st>>>(T, reads, L, n, frames, FP, segtab);
    } else {
        if (lds > 48 * 1024) HIPCK(hipFuncSetAttribute((const void *)k_translate_seg<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_translate_seg<false><<<dim3(ts_blocks), dim3(MC_TS_THREADS), lds, st>>>(T, reads, L, n, frames, FP, segtab);
    }
    return 0;
}

// ---- A1: seed enumeration, seed evaluation -----------------------------------------------------------------------------------------
// cand: null unless only best hits are wanted
struct McSeedBufs {
    const uint8_t *frames; const uint32_t *bitmap; McSeedTask *tasks; uint32_t cap_tasks; uint32_t *counters; unsigned long long *stats;
    McHsp *hsps; uint32_t cap_hsps; McGapTask *gaps; uint32_t cap_gaps; uint8_t *cand; uint64_t *hkeys; uint8_t *low; uint64_t *hplace;
};
enum McSeedKernel { MC_SEED_PLAIN, MC_SEED_QUEUES, MC_SEED_COUNTING };   // k_enumerate, k_enumerate_q, k_enumerate_count

// beside_lookahead: a translation of the next range is about to run beside the kernel.  shape_out (if given) receives waves per
// workgroup x workgroups per CU of the launch (0: k_enumerate).
static int mc_enumerate_launch(const McRun &R, const McSeedBufs &B, int64_t n, McSeedKernel kind, hipStream_t st, bool beside_lookahead = false, int *shape_out = nullptr)
{
    const int L = R.L, FP = R.FP;
    if (shape_out) *shape_out = 0;
    if (kind != MC_SEED_PLAIN) {
        // k_enumerate_q (round 5: queues that persist across the reads of a chunk) is the kernel of the product path; the counting form
        // (mc_set_counting: what the reference would read) is k_enumerate_count (rounds 2 - 4's one-wave-per-read kernel without filters).
        const bool enq = kind == MC_SEED_QUEUES;
        const size_t per_wave = enq ? MC_ENQ_WAVE_LDS(FP, L) : sizeof(McEnWave) + MC_EN_WAVE_LDS(FP, L);
        // Launch shape.  k_enumerate_q: SIXTEEN waves per CU (2 workgroups of 8) where the LDS holds them - the kernel is bound by the
        // scattered lines its CU's vector L1 has to fetch, not by issue or latency, and more resident waves only thrash
        // that cache: per 1 M reads of 100 / 150 / 300 bp 24 (20 at 300 bp) waves 3.85 / 6.23 / 13.29 ms, 16 waves 3.77 / 6.11 / 13.21.
        // The counting form (rounds 2 - 4's kernel, issue bound): as many as fit, up to 24 (16 waves 6.77 ms, 20: 6.45, 24: 6.39).
        int waves = 0, bpc = 1;
        {
            static const int shapes_q[][2] = {{8, 2}, {4, 4}, {16, 1}, {12, 1}, {4, 3}, {8, 1}, {4, 2}, {4, 1}};
            static const int shapes_c[][2] = {{12, 2}, {8, 3}, {4, 6}, {4, 5}, {16, 1}, {8, 2}, {4, 4}, {12, 1}, {4, 3}, {8, 1}, {4, 2}, {4, 1}};
            // Beside a lookahead's narrow translation (reads up to 191 bp) TWELVE waves in one workgroup, tried first: at 150 bp 79,840 B
            // of LDS instead of 2 x 53,248 leave room for nine translation workgroups of 8,960 B instead of six, and 3 x 80 registers of
            // a SIMD's lanes leave 272 for two translation waves of 96 - eight waves per CU, as many as the registers allow.  The seed
            // kernel takes 0.35 ms per 1 M reads longer and k_eval_seeds, beside which less of the translation is left, 0.6 less.
            // The arithmetic is that of 150 bp and the rule was measured at 100 and 150 bp only: for shorter reads, whose per-wave LDS is
            // smaller, it is an extrapolation - safe for the results, which no shape changes, and not known to be the fastest shape there
            if (enq && beside_lookahead && L / 3 <= MC_NARROW_MAXAA && 64 + 12 * per_wave <= 160 * 1024) { waves = 12; bpc = 1; }
            if (enq) { for (const auto &sh : shapes_q) if (!waves && (size_t)sh[1] * (64 + sh[0] * per_wave) <= 160 * 1024) { waves = sh[0]; bpc = sh[1]; } }
            else for (const auto &sh : shapes_c) if (!waves && (size_t)sh[1] * (64 + sh[0] * per_wave) <= 160 * 1024) { waves = sh[0]; bpc = sh[1]; }
        }
        if (!waves) { g_err = "reads too long for the seed kernel's LDS layout"; return -1; }
        const size_t lds2 = 64 + waves * per_wave;
        if (shape_out) *shape_out = waves * bpc;
#define MC_LAUNCH_EN(KERNEL, WV)                                                                                                                   \
    do {                                                                                                                                           \
        HIPCK(hipFuncSetAttribute((const void *)KERNEL<WV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));                               \
        const int blocks_ = (int)std::min<int64_t>((int64_t)MC_CUS * bpc, (n + WV - 1) / WV);                                                      \
        KERNEL<WV><<<dim3(blocks_), dim3(64 * WV), lds2, st>>>(R.T, R.X, B.bitmap, B.frames, FP, L, n, B.tasks, B.cap_tasks, B.counters, B.stats); \
    } while (0)
        if (enq) { if (waves == 16) MC_LAUNCH_EN(k_enumerate_q, 16); else if (waves == 12) MC_LAUNCH_EN(k_enumerate_q, 12); else if (waves == 8) MC_LAUNCH_EN(k_enumerate_q, 8); else MC_LAUNCH_EN(k_enumerate_q, 4); }
        else { if (waves == 16) MC_LAUNCH_EN(k_enumerate_count, 16); else if (waves == 12) MC_LAUNCH_EN(k_enumerate_count, 12); else if (waves == 8) MC_LAUNCH_EN(k_enumerate_count, 8); else MC_LAUNCH_EN(k_enumerate_count, 4); }
#undef MC_LAUNCH_EN
    } else
        k_enumerate<<<dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, st>>>(R.T, R.X, B.frames, FP, L, n, B.tasks, B.cap_tasks, B.counters, B.stats);
    return 0;
}

// (once per database, not per range: the n postings' words k_eval_seeds fetches in one load - k_post8)
static int mc_post8_launch(const uint32_t *post, const uint32_t *off, const uint8_t *res, uint32_t n, unsigned long long *post8, hipStream_t st)
{
    k_post8<<<dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, st>>>(post, off, res, n, post8);
    return 0;
}

// the number of seed hits stays on the device: persistent workgroups walk the pool.  ranges: k_enumerate_q wrote the pool (ranges of
// hits); the other two seed kernels write single hits
static int mc_eval_seeds_launch(const McRun &R, const McSeedBufs &B, bool ranges, hipStream_t st)
{
    const size_t lds_ev = (size_t)(MC_EV_BS / 64) * MC_EV_QCAP * 32;   // a queue of survivors per wave: 32 KB per workgroup
    HIPCK(hipFuncSetAttribute(ranges ? (const void *)k_eval_seeds<true> : (const void *)k_eval_seeds<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ev));
    if (ranges) k_eval_seeds<true><<<dim3(MC_CUS * MC_EV_BPC), dim3(MC_EV_BS), lds_ev, st>>>(R.T, R.X, B.frames, R.FP, R.L, B.tasks, B.counters + C_TASKS, B.cap_tasks, B.hsps, B.cap_hsps, B.gaps, B.cap_gaps, B.counters, R.P, R.fam, B.cand, B.hkeys, B.low, B.hplace);
    else k_eval_seeds<false><<<dim3(MC_CUS * MC_EV_BPC), dim3(MC_EV_BS), lds_ev, st>>>(R.T, R.X, B.frames, R.FP, R.L, B.tasks, B.counters + C_TASKS, B.cap_tasks, B.hsps, B.cap_hsps, B.gaps, B.cap_gaps, B.counters, R.P, R.fam, B.cand, B.hkeys, B.low, B.hplace);
    return 0;
}

// ---- B: gapped extension -----------------------------------------------------------------------------------------------------------
// gaps: the ngaps task records.  tab: the dedupe's table of `slots` entries (a power of two); leader: ngaps.  key, item, list: 2 ngaps
// words each - the flanks' sort keys, the flanks, the flanks ordered by DP size; hist: MC_GS_BINS.  fout: 2 ngaps flank results.
// retry, retry2: 2 ngaps each - the flanks that leave the first / the second window.  ws_full: MC_GAP_THREADS_FULL x MC_GAP_W cells.
// hsps .. hplace: where k_gap_emit appends (cand: null unless only best hits are wanted).
struct McGapBufs {
    const uint8_t *frames; const McGapTask *gaps; uint32_t *counters;
    unsigned long long *tab; uint32_t slots; uint32_t *leader, *key, *item, *list, *hist;
    McFlankOut *fout; uint32_t *retry, *retry2; McGapCell *ws_full;
    McHsp *hsps; uint32_t cap_hsps; uint8_t *cand; uint64_t *hkeys; uint8_t *low; uint64_t *hplace;
};
// the grids of the three DP launches for ngaps tasks; over (if given): a grid that is not 0 replaces the product's
struct McGapGrids { uint32_t lds, lds2, full; };
static inline McGapGrids mc_gap_grids(uint32_t ngaps, const int32_t *over = nullptr)
{
    McGapGrids g = {std::min<uint32_t>((2 * ngaps + 63) / 64, MC_GAP_GRID_MAX), MC_GAP_GRID2, MC_GAP_GRID_FULL};
    if (over) { if (over[0]) g.lds = (uint32_t)over[0]; if (over[1]) g.lds2 = (uint32_t)over[1]; if (over[2]) g.full = (uint32_t)over[2]; }
    return g;
}

// 1. group the tasks that extend the same ungapped segment and list the flanks of the distinct ones (tab and hist cleared by the caller)
static int mc_gap_dedupe_launch(const McRun &R, const McGapBufs &B, uint32_t ngaps, hipStream_t st)
{
    k_gap_dedupe<<<dim3((ngaps + 255) / 256), dim3(256), 0, st>>>(R.X, R.L, B.gaps, ngaps, B.tab, B.slots - 1, B.leader, B.key, B.item, B.counters);
    return 0;
}
// 2. a counting sort of up to cap items by key, the largest key first: the count at n_p stays on the device
static int mc_gap_sort_launch(const uint32_t *key, const uint32_t *item, const uint32_t *n_p, uint32_t cap, uint32_t *hist, uint32_t *out, hipStream_t st)
{
    k_gap_sort_hist<<<dim3(MC_GAP_SORT_BLOCKS), dim3(256), 0, st>>>(key, n_p, cap, hist);
    k_gap_sort_scan<<<dim3(1), dim3(1024), 0, st>>>(hist);
    k_gap_sort_scatter<<<dim3(MC_GAP_SORT_BLOCKS), dim3(256), 0, st>>>(key, item, n_p, cap, hist, out);
    return 0;
}
// 3. the flanks of `list` (counters[C_ITEMS] of them) with the DP rows in LDS, those whose band leaves the window again with a wider
// one, the rest with full-size rows
static int mc_gap_extend_launch(const McRun &R, const McGapBufs &B, const uint32_t *list, const McGapGrids &G, hipStream_t st)
{
    k_gapped_lds<MC_GAP_WIN, 64, MC_GAP_REFILL><<<dim3(G.lds), dim3(64), 0, st>>>(R.T, R.X, B.frames, R.FP, R.L, B.gaps, list, B.counters + C_ITEMS, B.fout,
                                                                                B.counters + C_RETRY, B.retry, B.counters + C_GTAKE);   // (8 waves per CU)
    k_gapped_lds<MC_GAP_WIN2, MC_GAP_LANES2, 1><<<dim3(G.lds2), dim3(64), 0, st>>>(R.T, R.X, B.frames, R.FP, R.L, B.gaps, B.retry, B.counters + C_RETRY, B.fout, B.counters + C_RETRY2, B.retry2, B.counters + C_GTAKE2);
    k_gapped<<<dim3(G.full), dim3(128), 0, st>>>(R.T, R.X, B.frames, R.FP, R.L, B.gaps, B.retry2, B.counters + C_RETRY2, B.fout, B.counters, B.ws_full, MC_GAP_W);
    return 0;
}
// 4. every task takes its HSP from its group's flank results
static int mc_gap_emit_launch(const McRun &R, const McGapBufs &B, uint32_t ngaps, hipStream_t st)
{
    k_gap_emit<<<dim3((ngaps + 255) / 256), dim3(256), 0, st>>>(R.T, R.X, R.L, B.gaps, ngaps, B.leader, B.fout, B.hsps, B.cap_hsps, B.counters, R.P, R.fam, B.cand, B.hkeys, B.low, B.hplace);
    return 0;
}
// The stage: 1. - 4. in st.  The counts of 2. - 4. stay on the device.
static int mc_gap_launch(const McRun &R, const McGapBufs &B, uint32_t ngaps, hipStream_t st)
{
    HIPCK(hipMemsetAsync(B.tab, 0, (size_t)B.slots * 8, st));
    HIPCK(hipMemsetAsync(B.hist, 0, MC_GS_BINS * sizeof(uint32_t), st));
    if (mc_gap_dedupe_launch(R, B, ngaps, st) || mc_gap_sort_launch(B.key, B.item, B.counters + C_ITEMS, 2 * ngaps, B.hist, B.list, st) ||
        mc_gap_extend_launch(R, B, B.list, mc_gap_grids(ngaps), st) || mc_gap_emit_launch(R, B, ngaps, st)) return -1;
    return 0;
}

// ---- C: binning and ordering -------------------------------------------------------------------------------------------------------
// hkeys, hplace: the HSP pool's keys and place words (cap_hsps; counters[C_HSPS] used); cand: the reads that are binned at all, or null
// for all.  heads: n + 2 (heads[0] = 0; heads + 1: counts -> starts -> ends); scan: mc_scan_u32's sums.  keys, places, slots, order, gsz:
// one per binned HSP.  heavy, heavy2, heavy3: the lists of k_order_lists, up to n reads each.  scratch: 12 words per binned HSP.
struct McOrderBufs {
    const uint64_t *hkeys, *hplace; uint32_t cap_hsps; const uint8_t *cand; uint32_t *counters;
    uint32_t *heads, *scan; uint64_t *keys, *places; uint32_t *slots, *order, *heavy, *heavy2, *heavy3;
    const uint8_t *low; uint32_t *gsz, *nv, *nrow; uint64_t *scratch; const McHsp *hsps; McHsp *v;
};
static int mc_bin_count_launch(const McOrderBufs &B, hipStream_t st)
{
    k_bin_count<<<dim3(MC_BIN_BLOCKS), dim3(256), 0, st>>>(B.hkeys, B.counters, B.cap_hsps, B.cand, B.heads + 1);
    return 0;
}
static int mc_bin_scatter_launch(const McOrderBufs &B, hipStream_t st)
{
    k_bin_scatter<<<dim3(MC_BIN_BLOCKS), dim3(256), 0, st>>>(B.hkeys, B.counters, B.cap_hsps, B.cand, B.heads + 1, B.hplace, B.keys, B.places, B.slots);
    return 0;
}
// HSPs into per-read segments: counts, their scan in place, the scatter
static int mc_bin_launch(const McOrderBufs &B, uint32_t n, hipStream_t st)
{
    uint32_t *cur = B.heads + 1;                                    // heads[0] = 0; cur[r]: counts -> starts -> ends = heads[r + 1]
    if (mc_bin_count_launch(B, st) || mc_scan_u32(cur, n, cur, B.scan, st) || mc_bin_scatter_launch(B, st)) return -1;
    return 0;
}
// The segments ordered by (subject, hit order) and stacked: the lists, the four ordering kernels, the copy.  one_side: the two long
// shapes share F.side.
static int mc_order_launch(const McOrderBufs &B, uint32_t n, hipStream_t st, const McFork &F, bool one_side)
{
    // the long segments beside the short ones (the few segments of more than 512 HSPs are a long tail on a nearly empty GPU)
    k_order_lists<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(B.heads, n, B.counters, B.heavy, B.heavy2, B.heavy3);
    hipStream_t side = F.side, side2 = one_side ? F.side : F.side2;   // (best hits only: few reads are ordered at all - a third stream only costs)
    HIPCK(hipEventRecord(F.fork, st)); HIPCK(hipStreamWaitEvent(F.side, F.fork, 0)); HIPCK(hipStreamWaitEvent(F.side2, F.fork, 0));
    HIPCK(hipFuncSetAttribute((const void *)k_order_heavy<1024, MC_ORDER_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mc_order_heavy_lds(MC_ORDER_LDS)));
    k_order_heavy<1024, MC_ORDER_LDS><<<dim3(MC_CUS), dim3(1024), mc_order_heavy_lds(MC_ORDER_LDS), side>>>(B.keys, B.places, B.slots, B.heads, B.heavy3, B.counters + C_ORDER3, B.counters + C_OTAKE3, B.low, B.order, B.gsz, B.nv, B.nrow, B.scratch);
    k_order_heavy<256, MC_ORDER_MID><<<dim3(MC_CUS * 4u), dim3(256), mc_order_heavy_lds(MC_ORDER_MID), side2>>>(B.keys, B.places, B.slots, B.heads, B.heavy2, B.counters + C_ORDER2, B.counters + C_OTAKE2, B.low, B.order, B.gsz, B.nv, B.nrow, B.scratch);
    HIPCK(hipEventRecord(F.join, F.side)); HIPCK(hipEventRecord(F.join2, F.side2));
    k_order_light<<<dim3((n + MC_OL_READS - 1) / MC_OL_READS), dim3(256), 0, st>>>(B.keys, B.places, B.slots, B.heads, n, B.low, B.order, B.gsz, B.nv, B.nrow);
    k_order_heavy<64, MC_ORDER_SMALL><<<dim3(MC_CUS * 16u), dim3(64), mc_order_heavy_lds(MC_ORDER_SMALL), st>>>(B.keys, B.places, B.slots, B.heads, B.heavy, B.counters + C_ORDER, B.counters + C_OTAKE, B.low, B.order, B.gsz, B.nv, B.nrow, B.scratch);
    HIPCK(hipStreamWaitEvent(st, F.join, 0)); HIPCK(hipStreamWaitEvent(st, F.join2, 0));
    k_order_copy<<<dim3(MC_BIN_BLOCKS), dim3(256), 0, st>>>(B.order, B.gsz, B.hsps, B.heads, n, B.v);
    return 0;
}
// The stage for n reads whose HSPs fill nslots slots of the pool: heads, row counts and order cleared, the binning, the ordering
static int mc_order_stage_launch(const McOrderBufs &B, uint32_t n, uint32_t nslots, hipStream_t st, const McFork &F, bool one_side)
{
    HIPCK(hipMemsetAsync(B.heads, 0, ((size_t)n + 2) * sizeof(uint32_t), st));
    HIPCK(hipMemsetAsync(B.nrow, 0, ((size_t)n + 1) * sizeof(uint32_t), st));
    HIPCK(hipMemsetAsync(B.order, 0xFF, (size_t)nslots * sizeof(uint32_t), st));
    if (mc_bin_launch(B, n, st) || mc_order_launch(B, n, st, F, one_side)) return -1;
    return 0;
}

// ---- D: per-read finishing, rows into m8 order -------------------------------------------------------------------------------------
// nv, heads, v, tmp, nrow: as stage C left them (tmp: two McHsp per stacked HSP, every read's scratch and then its rows).  heavy: the
// reads that get a wave; heavy1 .. heavy3: its entries by kernel; sorted1, sorted2: the first two with the longest stacks first;
// heap_order: heavy by rows - up to nheads entries each.  light: the four size classes of the other reads at light_pitch > nheads.
// rowoff, scan: the scan of nrow.  rows (cap_rows), best_of, best: the results.
struct McFinishBufs {
    const uint32_t *nv, *heads; McHsp *v, *tmp; uint32_t *nrow, *rowoff, *scan; McBestHit *best_of, *best; uint32_t *counters;
    uint32_t *heavy, *heavy1, *heavy2, *heavy3, *sorted1, *sorted2, *heap_order, *light; uint32_t light_pitch;
    McRow *rows; uint32_t cap_rows;
};
// nheads reads with nh stacked HSPs between them, numbered from first_read_id.  best_only: no rows, and the light kernels' threshold
// is MC_FH_MIN_BEST.  rows_free: an event st waits for before k_emit_rows writes B.rows, or null.
static int mc_finish_launch(const McRun &R, const McFinishBufs &B, uint32_t nheads, uint32_t nh, int64_t first_read_id, bool best_only, hipStream_t st, const McFork &F, hipEvent_t rows_free)
{
    // the thread-per-read kernel (reads with few HSPs) on this stream, the wave-per-read kernels one after the other on a
    // second one (each hands the reads its LDS arrays cannot hold to the next)
    k_heavy_lists<<<dim3((nheads + 255) / 256), dim3(256), 0, st>>>(B.nv, nheads, B.nrow, B.best_of, B.counters, B.heavy, B.light, B.light_pitch, best_only ? MC_FH_MIN_BEST : MC_FH_MIN,
                                                                     B.heavy1, B.heavy2, B.heavy3);
    HIPCK(hipEventRecord(F.fork, st));
    {
        const size_t l1 = mc_finish_heavy_lds(MC_FH_N1), l2 = mc_finish_heavy_lds(MC_FH_N2), l3 = mc_finish_heavy_lds(MC_FH_N3);
        HIPCK(hipFuncSetAttribute((const void *)k_finish_heavy<MC_FH_N3, C_HEAVY3, -1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l3));
        HIPCK(hipStreamWaitEvent(F.side, F.fork, 0));
        HIPCK(hipStreamWaitEvent(F.side2, F.fork, 0));
        // the two kernels of the larger reads (few reads, long chains, a fraction of the GPU) beside the first one.  (Round 5, kernel trace:
        // second + third, 0.84 ms per 1 M reads, is the longer chain in front of MergeRes' heap sort; the third in front of the thread-per-read
        // kernels on this stream, or in front of the first on its stream, made the stage 0.1 - 0.2 ms LONGER - whatever runs behind the
        // third waits for its few long reads, and they hold 135 KB of a CU's LDS each.)
        const unsigned wpc2 = (unsigned)std::min<size_t>(8, std::max<size_t>(1, (size_t)(158 * 1024) / (l2 + 1024)));   // waves per CU the LDS holds
        // (the lists of the first two kernels with the longest stacks first - k_heavy_order; the third has a few dozen reads)
        k_heavy_order<<<dim3(1), dim3(1024), 0, F.side2>>>(B.heavy2, B.counters + C_HEAVY2, B.heavy, B.nv, 2, B.sorted2);
        k_finish_heavy<MC_FH_N2, C_HEAVY2, -1><<<dim3(MC_CUS * wpc2), dim3(64), l2, F.side2>>>(R.T, R.X, R.P, R.fam, B.nv, B.heads, nheads, B.v, B.tmp, first_read_id,
                                                                                            B.nrow, B.best_of, B.counters, B.heavy, B.sorted2, nullptr);
        k_finish_heavy<MC_FH_N3, C_HEAVY3, -1><<<dim3(MC_CUS), dim3(64), l3, F.side2>>>(R.T, R.X, R.P, R.fam, B.nv, B.heads, nheads, B.v, B.tmp, first_read_id,
                                                                                     B.nrow, B.best_of, B.counters, B.heavy, B.heavy3, nullptr);
        HIPCK(hipEventRecord(F.join2, F.side2));
        k_heavy_order<<<dim3(1), dim3(1024), 0, F.side>>>(B.heavy1, B.counters + C_HEAVY1, B.heavy, B.nv, 0, B.sorted1);
        k_finish_heavy<MC_FH_N1, C_HEAVY1, -1><<<dim3(MC_CUS * 12), dim3(64), l1, F.side>>>(R.T, R.X, R.P, R.fam, B.nv, B.heads, nheads, B.v, B.tmp, first_read_id,
                                                                                        B.nrow, B.best_of, B.counters, B.heavy, B.sorted1, nullptr);
        HIPCK(hipStreamWaitEvent(F.side, F.join2, 0));
        // MergeRes' heap sort of all of them (a lane per read), then their rows (a wave per read)
        const size_t lh = mc_heap_lanes_lds();
        HIPCK(hipFuncSetAttribute((const void *)k_heap_lanes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lh));
        k_heap_order<<<dim3(1), dim3(1024), 0, F.side>>>(B.heavy, B.nrow, B.counters, B.heap_order);
        k_heap_lanes<<<dim3(MC_CUS), dim3(64), lh, F.side>>>(B.heads, nheads, nh, B.tmp, B.nrow, B.counters, B.heavy, B.heap_order);
        k_heavy_rows<<<dim3(MC_CUS * 12), dim3(64), 0, F.side>>>(R.T, R.X, R.P, R.fam, B.heads, nheads, B.v, B.tmp, first_read_id, B.nrow, B.best_of, B.counters, B.heavy);
        HIPCK(hipEventRecord(F.join, F.side));
    }
    // the light reads: the four size classes side by side (the counts stay on the device; blocks past a class' count leave at once)
    {   // (size classes 2, 3 - up to 48 / MC_FH_MIN stacked HSPs - with MC_FH_MIN items of LDS per thread, classes 0, 1 - up to 4 / 16 - with 16; the
        // items are reached through generic pointers - mc_finish_stacked is shared with the host - and a flat access to LDS must stay
        // below 64 KB of the workgroup's allocation: 32 and 128 threads per workgroup)
        const size_t lb = mc_finish_lds(32, MC_FH_MIN), ls = mc_finish_lds(128, 16);
        HIPCK(hipFuncSetAttribute((const void *)k_finish<32, MC_FH_MIN, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb));
        k_finish<32, MC_FH_MIN, 2><<<dim3((nheads + 31) / 32, 2), dim3(32), lb, st>>>(R.T, R.X, R.P, R.fam, B.nv, B.heads, nheads, B.v, B.tmp,
                                                                             first_read_id, B.nrow, B.best_of, B.light, B.light_pitch, B.counters + C_LIGHT0);
        k_finish<128, 16, 0><<<dim3((nheads + 127) / 128, 2), dim3(128), ls, st>>>(R.T, R.X, R.P, R.fam, B.nv, B.heads, nheads, B.v, B.tmp,
                                                                                 first_read_id, B.nrow, B.best_of, B.light, B.light_pitch, B.counters + C_LIGHT0);
    }
    HIPCK(hipStreamWaitEvent(st, F.join, 0));
    if (mc_scan_u32(B.nrow, nheads, B.rowoff, B.scan, st)) return -1;
    if (rows_free) HIPCK(hipStreamWaitEvent(st, rows_free, 0));   // (the rows of the run before may still be leaving B.rows)
    k_emit_rows<<<dim3((nheads + 255) / 256), dim3(256), 0, st>>>(B.heads, nheads, B.nrow, B.rowoff, B.tmp, B.rows, B.cap_rows, B.best_of, B.best, B.counters, best_only ? 0 : 1);
    return 0;
}
