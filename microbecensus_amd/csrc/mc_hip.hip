// mc_hip.hip - libmcensus_hip.so for gfx950: the handle, the five-stage pipeline of a batch, the streaming forms and the C ABI
// (include/mcensus.h names what each entry point replaces in the reference).  One translation unit; the kernels live in
//   mc_hip_common.h    includes, counters, wave-level helpers
//   k_translate_seg.h  A1  six-frame translation + SEG: a wave per 10 reads, the trimming search dealt out over the wave
//   k_enumerate.h      A2  seed enumeration + index probes: a wave per read, a state machine over per-wave LDS queues that persist across the reads of a chunk (k_enumerate_q)
//   k_eval_seeds.h     A3  seed gate, growth, ungapped X-drop: persistent waves, gate and extension as two phases of a wave
//   k_gapped.h         B   gapped X-drop: one DP per distinct segment, a lane per flank, DP rows packed in LDS
//   k_order.h          C   HSPs binned per read (no global sort), ordered and stacked for the reads that can print
//   k_finish.h         D   sum statistics, std::sort / heap sort replayed, 500-row cap, classification; rows in m8 order
//   mc_stages.h            (host) the launches of A - D: grids, LDS sizes, forks and joins, over raw pointers; the stages below sequence them, the unit tests' harnesses share them
//   k_grid.h               the training workflow's grid classification
//   k_simulate.h           the library simulator of the training workflow and of mock communities: the kernels, the genome's placer
//   k_community.h          the placer of a mock community of genomes (mc_community_*)
//   k_varlen.h             reads of mixed lengths bucketed by length (mc_search_varlen)
//   k_classes.h            padded read rows sorted into length classes and trimmed (mc_search_classes)
//   k_bootstrap.h          the Poisson bootstrap of the per-family sums (mc_bootstrap)
//   k_wfit.h               the fit of the per-family weights, training step 5 (mc_fit_weights, mc_weights_mue)
//   k_abundance.h          per-gene read counts for RPKG, summed over the rows of every completed range (mc_set_abundance)
//   k_coverage.h           per-gene coverage breadth and depth beside them: marks in the counting kernel, a scan at read time (mc_set_coverage)
//   k_ties.h               the tie accounting beside them: unique, candidate and shared reads of the genes that tie for a read's best hit (mc_set_ties)
//   k_curve.h              the rarefaction curve beside them: per-gene counts per prefix of the sample, every residue's first read, a scan at read time (mc_set_curve)
//   k_tieboot.h            the bootstrap of the tie shares beside both: a device list of (read id, gene, share), per-gene replicate sums at read time (mc_set_tie_bootstrap)
//   k_covboot.h            the bootstrap of the coverage columns: a device list of (read id, gene, span), per-gene replicate covered residues at read time (mc_set_coverage_bootstrap)
//   k_geneboot.h           the bootstrap of the counts beside them: a device list of (read id, gene), per-gene replicate sums, sort and summary at read time (mc_set_gene_bootstrap)
//   k_groupboot.h          the bootstrap of the groups table behind it: every group's replicate values walked over its members' rows of the replicate sums, sort and summary (mc_group_bootstrap)
//   k_identity.h, mc_identity.h   the identity of the assigned reads: a histogram and three sums per gene on the rows of a range, min / median / max and levels by a scan at read time (mc_set_identity)
//   k_depthstats.h, mc_depthstats.h   the median and the truncated average of every gene's depth: a radix selection over the difference array at read time (mc_depth_stats)
//   k_abund_classes.h      the per-class table of the counts on class runs (mc_set_abundance_classes)
//   k_fold.h, mc_fold.h    genes longer than one sequence of the engine: segments, and the fold of a range's rows onto the genes (mc_set_gene_fold)
//   mc_abund.h             (host) the owner of those five: the tables' layout, the launch on a range's rows, which buffer exists when, the readers
//   mc_pieces.h            (host) a batch sorted into bins of one length each, cut into the ranges the pipeline runs once per length
// and the per-thread algorithms they share with the test-only emulation in mc_core.h / mc_finish.h / mc_index.h.
// Stage E copies rows and best hits to pinned host memory.  mc_run_range() issues the stages of one range; run_stream() feeds
// ranges from a host-side source (mc_search, mc_search_files, mc_search_files_multi) with upload and search overlapped.
#include "mc_hip_common.h"
#include "k_translate_seg.h"
#include "k_enumerate.h"
#include "k_eval_seeds.h"
#include "k_gapped.h"
#include "k_order.h"
#include "k_finish.h"
#include "mc_stages.h"
#include "k_grid.h"
#include "k_simulate.h"
#include "k_community.h"
#include "k_varlen.h"
#include "k_classes.h"
#include "k_bootstrap.h"
#include "k_wfit.h"
#include "mc_pieces.h"
#include "mc_ahead.h"
#include "mc_owned.h"
#include "mc_abund.h"

#include <map>

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// Everything the range in flight needs: streams, events, the pools of the stages, the pinned mirrors of the device counters.  One per
// handle: what overlaps is the host's work on the results of one range with the front of the next, and that needs no second set of
// pools - range_begin.
struct McCtx {
    McStream stream; hipStream_t side = nullptr, side2 = nullptr;   // the pipeline of a range, and two side streams of the ordering / finishing kernels (borrowed: the handle's)
    McEvent ev[8], ev_fork, ev_join, ev_join2;
    McEvent ev_wait[2]; bool waited = false;                       // around the stream's wait for a lookahead's kernel (range_begin); waited: this range's stream had one
    int64_t cap_reads = 0; int pool_len = 0;                       // the pools hold cap_reads reads of up to pool_len bases
    int ts_staged = -1;                                            // the form of k_translate_seg the last range launched (mc_debug_stage 5)
    int ts_narrow = -1;                                            // ... and whether it was the narrow instantiation (mc_debug_stage 6)
    int seed_shape = -1;                                           // waves per workgroup x workgroups per CU of the last seed launch (mc_debug_stage 7)
    uint32_t cap_tasks = 0, cap_gaps = 0, cap_hsps = 0, cap_rows = 0;
    // Two frame buffers (mc_ahead.h): d_frames is the RUNNING range's - the one every reader means - and a lookahead writes the other;
    // a range_begin that takes a lookahead makes that buffer the current one (frames_use).  Views 64 bytes in, behind an apron of MC_INV:
    // k_eval_seeds reads 8 bytes at a time backwards from a seed.
    McDev<uint8_t> d_frames_base[2]; uint8_t *d_frames = nullptr;
    uint8_t *frames_of(int b) const { return d_frames_base[b] + 64; }
    void frames_use(int b) { d_frames = frames_of(b); }
    McDev<unsigned long long> d_stats;
    McDev<McSeedTask> d_tasks; McDev<McGapTask> d_gaps; McDev<McHsp> d_hsps, d_v, d_tmp;
    McDev<uint64_t> d_k64, d_hkeys, d_hplace, d_places; McDev<uint32_t> d_idx, d_idxo, d_heads, d_scan, d_gsz, d_nv, d_ghist;
    McDev<uint32_t> d_counters;
    McDev<McRow> d_rows; McDev<uint32_t> d_nrow, d_rowoff; McDev<McBestHit> d_best, d_bestof; McDev<uint8_t> d_low, d_cand;
    McDev<McGapCell> d_gws_full; McDev<uint32_t> d_retry, d_retry2;
    McDev<unsigned long long> d_gtab; uint32_t gtab_slots = 0; McDev<uint32_t> d_gleader; McDev<McFlankOut> d_fout;
    // pinned host mirrors
    McPin<uint32_t> h_c; McPin<unsigned long long> h_stats; McPin<McBestHit> h_best; size_t h_best_cap = 0;
    // the range being processed
    const uint8_t *reads = nullptr; int64_t n = 0, first_read_id = 0, first = 0;   // (first: the range's first read in the resident set)
    int ahead_from = -1;                                           // the pair of the handle's ahead_ev around the lookahead this range used; -1: none
    bool predicts = false;                                         // the range issues the lookahead for the range behind it itself, at its begin (mc_range_begin); otherwise range_end is told
    bool own_a0 = true;                                            // ev[0], ev[1] are around a translation of the range's own (all of it, or the reads behind the lookahead's)
    uint32_t ntasks = 0, ngaps = 0, gpad = 0, nh = 0, nh_all = 0, nheads = 0, nrows = 0, nbest = 0, nsegs = 0;
    bool busy = false;                                             // a range has been begun and not ended
};

struct mc_handle {
    McHostIndex H;
    std::vector<int32_t> fam;
    int nfam = 0, device = 0;
    // device index + tables
    McDev<uint8_t> d_res_base; uint8_t *d_res = nullptr; McDev<uint32_t> d_off, d_bstart, d_post; McDev<unsigned long long> d_post8; McDev<uint16_t> d_keys; McDev<int32_t> d_fam;   // (d_res: a view 64 bytes in)
    McDev<McTables> d_T; McDev<McClassPars> d_P;
    McTables hT; McClassPars hP;
    int read_len = 0, FP = 0; bool run_set = false;
    McDev<uint32_t> d_bitmap;
    McDev<McBucketRec> d_rec;
    McDev<uint32_t> d_filt, d_wild, d_pair; McDev<uint64_t> d_segtab; McDev<unsigned long long> d_rt;
    bool fast_enum = false;
    bool count_traffic = false;
    int pipe_nout = 0;                    // mc_range_begin / mc_range_end: 1 while a range has been begun and not ended
    bool keep_rows = true;                // mc_search / mc_search_files hand out the m8 rows (mc_set_keep_rows)
    bool best_only = false;               // only the reads that can be classified are ranked; no rows (mc_set_best_hits_only)
    bool rows_stay = false;               // mc_train_library: the rows of a range stay in the context's d_rows (no copy to the host)
    float train_ms[3] = {0, 0, 0};        // mc_train_library: simulate, search, grid of the last library (HIP events)
    float comm_ms[2] = {0, 0};            // mc_community_library: simulate, search of the last library (HIP events)
    int64_t train_bases = 0;              // mc_train_library: the bases of the last library's reads (mc_train_library_bases)
    float boot_ms = 0;                    // mc_bootstrap: the two kernels of the last call (HIP events)
    float wfit_ms = 0;                    // mc_fit_weights / mc_weights_mue: the kernels of the last call (HIP events)
    McAbundance ab;                       // mc_set_abundance, mc_set_coverage, mc_set_ties: the switches and all that hangs on them (mc_abund.h)
    McPin<uint8_t> stage_pin[2]; McDev<uint8_t> stage_dev[2]; size_t stage_bytes = 0; McStream copy_stream;   // run_stream (stage_bytes: what all four hold, 0 until they do)
    // resident reads
    int64_t nreads = 0, cap_own = 0;
    McDev<uint8_t> d_reads;
    const uint8_t *reads_dev = nullptr;   // resident read set (own buffer or attached caller memory)
    McCtx ctx;
    // the lookahead (mc_ahead.h): the translation of the range expected next, on a stream of its own beside the front of the
    // running range, into the frame buffer that range does not use.  ahead_ev[p]: the events around the kernel of lookahead p (two
    // pairs in turn: the range that used lookahead p reads its interval at ITS range_end, after the lookahead for the range behind it has been issued);
    // ahead_wait: the kernel of ahead_ev[ahead_p] may still be running and nothing has been made to wait for it yet.
    McStream ahead_stream; McEvent ahead_ev[2][2]; int ahead_p = 0; bool ahead_wait = false;
    McAhead ahead; uint64_t reads_gen = 0, tables_gen = 0; int64_t ahead_used = 0;
    float ahead_ms = 0;                                            // the interval of the lookahead's kernel the range that ended last used (mc_ahead_kernel_ms); 0: it used none
    // host results: rows of the last run land in pinned memory; mc_search() accumulates its batches in all_rows
    // The rows travel to the host while the caller goes on (two pinned buffers in turn, a stream and an event of their own):
    // mc_run_range() returns when the best hits are there; whoever looks at the rows waits for their copy (rows_wait).
    McPin<mc_row> pin_slot[2]; size_t pin_slot_cap[2] = {0, 0}; int pin_cur = 0;   // (pin_cur: the slot of the current run)
    McStream side, side2;                                           // (McCtx::side, side2)
    McStream rows_stream; McEvent ev_rows; bool rows_pending = false, rows_ever = false;
    std::vector<mc_row> all_rows, split_rows;                       // accumulated over the batches of a stream / over the halves of a range that overflowed
    const mc_row *res_rows = nullptr; int64_t n_res_rows = 0;
    std::vector<mc_best_hit> best; mc_stats stats;
    McCtx *best_from = nullptr; uint32_t best_count = 0;           // the context whose best hits (pinned, unordered) are those of the last range, and how many: best_materialize
    std::map<int, McTables> vl_tables; double vl_thr = 0;           // mc_search_varlen: mc_fill_tables() per bucket length, for the E-value threshold vl_thr
    // length classes (mc_set_run_classes): the list, every class's classification parameters, and what the last class run left
    McClasses cls = {}; bool cls_set = false, cls_results = false; std::vector<McClassPars> cls_pars;
    std::vector<uint8_t> best_cls; int64_t cls_reads[MC_CL_BINS] = {};
};

// The lookahead is given up: its kernel is waited for (after its event it is harmless) and its frames are nobody's.  Before anything
// that assumes a quiet device once no range is in flight - new reads, new tables, new pools, a look at d_frames, the end of the handle.
static void ahead_drop(mc_handle *h)
{
    if (h->ahead_wait) { (void)hipStreamSynchronize(h->ahead_stream); h->ahead_wait = false; }   // (nothing but lookaheads runs in that stream)
    mc_ahead_drop(h->ahead);
}
static constexpr bool MC_AHEAD_ON = true;                          // lookaheads are issued (off: every range translates in its own range_begin, as before)
static McAheadKey ahead_key(const mc_handle *h, int64_t first, int64_t count) { return {h->reads_gen, first, count, h->read_len, h->FP, h->tables_gen}; }
// the resident reads are about to change (the buffer, or what it holds) / the run's tables on the device are
static void reads_change(mc_handle *h) { ahead_drop(h); h->reads_gen++; }
static void tables_change(mc_handle *h) { ahead_drop(h); h->tables_gen++; }

static McIndex dev_index(const mc_handle *h)
{
    McIndex X; X.res = h->d_res; X.off = h->d_off; X.bstart = h->d_bstart; X.post = h->d_post; X.post8 = h->d_post8; X.keys = h->d_keys; X.rec = h->d_rec; X.filt = h->d_filt; X.wild = h->d_wild; X.pair = h->d_pair; X.rt = h->d_rt; X.rt_mask = h->H.rt_mask; X.nseq = h->H.nseq;
    return X;
}

static McRun run_of(const mc_handle *h) { return {h->d_T, dev_index(h), h->d_P, h->d_fam, h->read_len, h->FP}; }
static McFork fork_of(const McCtx &c) { return {c.side, c.side2, c.ev_fork, c.ev_join, c.ev_join2}; }

// ---- The carving of the pools: what each stage's launch function (mc_stages.h) is given of them ---------------------------------
// The ONLY place that writes an offset into d_retry, d_retry2, d_k64, d_idx, d_idxo or d_tmp.  A stage borrows what another has
// finished with; beside every borrowed region stands what is written there and the condition under which that fits.  The conditions
// in the capacities alone are checked where the pools are sized (carve_fits, ensure_capacity); DESIGN.md 5.9 has the table.
// With cap = cap_reads and G = cap_gaps:  d_retry has 2 G + cap + 1 words, d_retry2 2 G, d_k64 cap_hsps of 8 bytes, d_idx and d_idxo
// cap_hsps of 4, d_tmp 2 cap_hsps McHsp.  G / 2 rounds down, so [0, G / 2) and [G / 2, G) hold G / 2 and G - G / 2 >= G / 2 words.

// A1: every array is its own pool
static McSeedBufs carve_seed(const mc_handle *h, const McCtx &c)
{
    return {c.d_frames, h->d_bitmap, c.d_tasks, c.cap_tasks, c.d_counters, c.d_stats, c.d_hsps, c.cap_hsps, c.d_gaps, c.cap_gaps, h->best_only ? c.d_cand.get() : nullptr, c.d_hkeys, c.d_low, c.d_hplace};
}
// B.  Borrowed from the HSP ordering, idle until stage C: the flanks' 2 ngaps sort keys of 4 bytes in d_k64 (8 cap_hsps bytes), the
// 2 ngaps flanks in d_idx, their sorted list in d_idxo (4 cap_hsps bytes each): 2 ngaps <= cap_hsps, which depends on the range and
// is checked per range (stage_b).  Its own: retry, retry2 - flanks that leave a window, at most 2 ngaps <= 2 G of 2 G words.
static McGapBufs carve_gap(const mc_handle *h, const McCtx &c, uint32_t slots)
{
    McGapBufs B = {};
    B.frames = c.d_frames; B.gaps = c.d_gaps; B.counters = c.d_counters;
    B.tab = c.d_gtab; B.slots = slots; B.leader = c.d_gleader; B.hist = c.d_ghist;
    B.key = (uint32_t *)c.d_k64.get(); B.item = c.d_idx; B.list = c.d_idxo;
    B.fout = c.d_fout; B.retry = c.d_retry; B.retry2 = c.d_retry2; B.ws_full = c.d_gws_full;
    B.hsps = c.d_hsps; B.cap_hsps = c.cap_hsps; B.cand = h->best_only ? c.d_cand.get() : nullptr; B.hkeys = c.d_hkeys; B.low = c.d_low; B.hplace = c.d_hplace;
    return B;
}
// C.  keys, slots, order in d_k64, d_idxo, d_idx (the gapped stage's sort buffers: free again) - one entry per binned HSP of at most
// cap_hsps, their own size.  Borrowed from the gapped stage, whose retry lists are done: the three lists of k_order_lists in d_retry2
// at 0, G and G + G / 2 - each lists a read at most once, n <= cap entries, in regions of G, G / 2 and G - G / 2 words: cap <= G / 2.
// scratch: all of d_tmp, 12 words of 8 bytes per HSP of a segment at 12 x its first slot - the two McHsp of 48 bytes d_tmp has per slot.
static McOrderBufs carve_order(const mc_handle *h, const McCtx &c)
{
    const size_t G = c.cap_gaps;
    McOrderBufs B = {};
    B.hkeys = c.d_hkeys; B.hplace = c.d_hplace; B.cap_hsps = c.cap_hsps; B.cand = h->best_only ? c.d_cand.get() : nullptr; B.counters = c.d_counters;
    B.heads = c.d_heads; B.scan = c.d_scan; B.keys = c.d_k64; B.places = c.d_places; B.slots = c.d_idxo; B.order = c.d_idx;
    B.heavy = c.d_retry2; B.heavy2 = c.d_retry2 + G; B.heavy3 = c.d_retry2 + G + G / 2;
    B.low = c.d_low; B.gsz = c.d_gsz; B.nv = c.d_nv; B.nrow = c.d_nrow; B.scratch = (uint64_t *)c.d_tmp.get(); B.hsps = c.d_hsps; B.v = c.d_v;
    return B;
}
// D.  All eight lists are borrowed: d_retry is free again (the gap tasks are done), and so is d_retry2 (the ordering kernels' lists:
// done).  Each of heavy .. heap_order holds a read, or an entry of heavy, at most once: nheads <= cap entries in a region of at least
// G / 2 words - cap <= G / 2 again.  The four light lists lie at pitch cap + 1 behind d_retry + G + G / 2 and end at
// G + G / 2 + 4 (cap + 1) of the array's 2 G + cap + 1 words: 3 (cap + 1) <= G - G / 2.
static McFinishBufs carve_finish(const McCtx &c)
{
    const size_t G = c.cap_gaps;
    McFinishBufs B = {};
    B.nv = c.d_nv; B.heads = c.d_heads; B.v = c.d_v; B.tmp = c.d_tmp; B.nrow = c.d_nrow; B.rowoff = c.d_rowoff; B.scan = c.d_scan;
    B.best_of = c.d_bestof; B.best = c.d_best; B.counters = c.d_counters; B.rows = c.d_rows; B.cap_rows = c.cap_rows;
    B.heavy = c.d_retry; B.heavy2 = c.d_retry + G / 2; B.heavy3 = c.d_retry + G; B.light = c.d_retry + G + G / 2; B.light_pitch = (uint32_t)c.cap_reads + 1;
    B.heavy1 = c.d_retry2; B.sorted1 = c.d_retry2 + G / 2; B.heap_order = c.d_retry2 + G; B.sorted2 = c.d_retry2 + G + G / 2;
    return B;
}
// The conditions above that depend on the capacities alone.  They hold for every batch the library accepts: cap <= 2^21 - 1, and
// G = min(cap (L / 8 + 8) + 2^18 + ev_pad, 2^27 - 2) with L >= 18 is at least 10 cap + 2^18 unclipped - 3 (cap + 1) <= 5 cap + 2^17 -
// and 2^27 - 2 clipped, where G - G / 2 = 2^26 - 1 >= 3 x 2^21.  The stronger one implies the other.
static bool carve_fits(int64_t cap, int64_t G) { return cap <= G / 2 && 3 * (cap + 1) <= G - G / 2; }

extern "C" void mc_debug_live(int64_t out[4]) { for (int k = 0; k < MC_LIVE_N; k++) out[k] = mc_live[k].load(); }

extern "C" int mc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Every resource of the handle is a member that frees itself (mc_owned.h).  What is left is order: the rows of the last run may
// still be on their way into a pinned slot, and that copy has to end before the slot does.
extern "C" void mc_close(mc_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    ahead_drop(h);                                                  // (a lookahead may still be writing d_frames)
    if (h->rows_stream) (void)hipStreamSynchronize(h->rows_stream);
    delete h;
}

// Host arrays -> device through two pinned bounce buffers (a memcpy into one while the other travels).  hipMemcpy from pageable
// memory pins the caller's pages on the way: the 110 MB of the index took 80 - 150 ms of the engine's 120 - 190 ms warm-cache
// open that way (the reference's default use is ONE run per process: microbe_census.py:375) - this takes ~25.
struct McUploader {
    static constexpr size_t CH = (size_t)8 << 20;
    McPin<uint8_t> pin[2]; McEvent ev[2]; McStream st; int k = 0; bool used[2] = {false, false};
    int init()
    {
        if (st.create()) return -1;
        for (int i = 0; i < 2; i++) if (pin[i].alloc(CH) || ev[i].create(false)) return -1;
        return 0;
    }
    int put(void *dst, const void *src, size_t bytes)
    {
        for (size_t at = 0; at < bytes; at += CH) {
            const size_t n = std::min(CH, bytes - at);
            if (used[k]) HIPCK(hipEventSynchronize(ev[k]));
            memcpy(pin[k], (const uint8_t *)src + at, n);
            HIPCK(hipMemcpyAsync((uint8_t *)dst + at, pin[k], n, hipMemcpyHostToDevice, st));
            HIPCK(hipEventRecord(ev[k], st)); used[k] = true;
            k ^= 1;
        }
        return 0;
    }
    int finish() { if (st) HIPCK(hipStreamSynchronize(st)); return 0; }
    ~McUploader() { if (st) (void)hipStreamSynchronize(st); }       // (a copy may still read a bounce buffer)
};

// h->H holds the host index (built from FASTA or loaded from a rapdb): everything device side
static int open_impl(mc_handle *h, const int32_t *marker_family, int32_t nfam, int32_t device)
{
    int ndev = 0;
    double t0 = mc_now();
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device available: libmcensus_hip has no CPU fallback"; return -1; }
    if (device < 0 || device >= ndev) { g_err = "device index out of range"; return -1; }
    if (nfam > 32) { g_err = "at most 32 gene families are supported"; return -1; }
    const int nseq = h->H.nseq;
    if (nseq > 32767) { g_err = "more than 32767 markers: the HSP sort key (read<<43 | subject<<28 | hit order) holds 15 bits of subject index"; return -1; }
    static_assert(MC_FOLD_SEG_LEN == MC_GAP_W - 8, "a segment of a long gene (mc_fold.h) is the longest sequence this check lets through");
    for (int s = 0; s < nseq; s++) if ((int)(h->H.off[s + 1] - h->H.off[s]) > MC_GAP_W - 8) { g_err = "marker longer than the gapped-extension workspace"; return -1; }
    if (marker_family) h->fam.assign(marker_family, marker_family + nseq); else h->fam.assign((size_t)nseq, 0);
    h->nfam = nfam; h->device = device;
    HIPCK(hipSetDevice(device));
    HIPCK(hipFree(nullptr));
    MC_OT("  HIP runtime, device", t0);
    // Streams: one for the pipeline of a range, two side streams for the ordering / finishing kernels of the longest reads
    // (the handle's), one for the rows on their way to the host, one for the
    // uploads of the streaming calls.  HIP multiplexes its streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the environment
    // says otherwise) and streams that share one wait for each other: with nine streams the front of a range could land behind the
    // 5 ms copy of the rows of the range before (measured: 51.2 instead of 53.6 M reads/s) - hence few streams.  The queue count is
    // the environment's: neither this library nor the package's entry points set it.
    // The ORDER of creation decides who shares: the runtime gives the first four streams a hardware queue each and every later one the
    // LAST-made queue among those with the fewest streams (read off the Queue_Id column of kernel traces).  The lookahead's
    // kernel lives for most of a range, and whatever shares its queue waits behind it - as the rows' copy did (a blit kernel), and
    // stage D behind that.  So: the range's stream, the lookahead's, side, side2 - four queues - then the rows' stream, which lands on
    // side2's queue (its copy of range i has long left when range i + 1 reaches its finishing kernels); the null stream comes to lie on
    // side's, and run_stream's copy stream, made last, on the lookahead's.  That policy is observed, not documented, and the layout
    // holds for the FIRST handle of a process whose caller has made no streams before mc_open: a second handle's streams, or a handle
    // behind a caller's own, join queues that are taken, wherever the fewest streams are.  Only speed depends on it, never a result.
    if (h->ctx.stream.create() || h->ahead_stream.create()) return -1;
    if (h->side.create() || h->side2.create()) return -1;
    {
        McCtx &c = h->ctx;
        c.side = h->side; c.side2 = h->side2;
        for (auto &e : c.ev) if (e.create()) return -1;
        if (c.ev_fork.create(false) || c.ev_join.create(false) || c.ev_join2.create(false)) return -1;
        for (auto &e : c.ev_wait) if (e.create()) return -1;
        if (c.d_counters.alloc(C_N) || c.d_stats.alloc(S_N) || c.d_ghist.alloc((size_t)MC_GS_BINS)) return -1;
        if (c.h_c.alloc(C_N) || c.h_stats.alloc(S_N)) return -1;
    }
    if (h->rows_stream.create() || h->ev_rows.create(false)) return -1;
    for (auto &pair : h->ahead_ev) for (auto &e : pair) if (e.create()) return -1;
    const McHostIndex &H = h->H;
    if (H.res.size() >= MC_TASK_ABS_LIMIT) { g_err = "marker database too large: more than 16 M residues (MC_TASK_W3)"; return -1; }
    if (h->d_res_base.alloc(H.res.size() + 128) || h->d_off.alloc(H.off.size()) || h->d_bstart.alloc(H.bstart.size()) || h->d_post.alloc(H.post.size() + 1) || h->d_post8.alloc((H.post.size() + 1) * MC_POST_WORDS) ||
        h->d_keys.alloc(H.keys.size()) || h->d_fam.alloc((size_t)nseq) || h->d_T.alloc(1) || h->d_P.alloc(1)) return -1;
    HIPCK(hipMemset(h->d_res_base, MC_INV, H.res.size() + 128));
    h->d_res = h->d_res_base + 64;                                 // (k_gapped_lds reads 16 bytes at a time around a flank's first residues)
    h->ab.bind(nseq, (size_t)H.nres, h->d_off);
    if (h->d_bitmap.alloc(H.bitmap.size()) || h->d_filt.alloc(H.filt.size()) || h->d_wild.alloc(H.wild.size()) || h->d_pair.alloc(H.pair.size()) || h->d_rt.alloc(H.rt.size())) return -1;
    if (!H.rec.empty() && h->d_rec.alloc(H.rec.size())) return -1;
    {
        McUploader up;
        if (up.init() || up.put(h->d_res, H.res.data(), H.res.size()) || up.put(h->d_off, H.off.data(), H.off.size() * 4) || up.put(h->d_bstart, H.bstart.data(), H.bstart.size() * 4) ||
            up.put(h->d_post, H.post.data(), H.post.size() * 4) || up.put(h->d_keys, H.keys.data(), H.keys.size() * 2) || up.put(h->d_fam, h->fam.data(), (size_t)nseq * 4) ||
            up.put(h->d_bitmap, H.bitmap.data(), H.bitmap.size() * 4) || up.put(h->d_pair, H.pair.data(), H.pair.size() * 4) || up.put(h->d_wild, H.wild.data(), H.wild.size() * 4) ||
            up.put(h->d_rt, H.rt.data(), H.rt.size() * 8) || up.put(h->d_filt, H.filt.data(), H.filt.size() * 4) ||
            (!H.rec.empty() && up.put(h->d_rec, H.rec.data(), H.rec.size() * sizeof(McBucketRec))) || up.finish()) return -1;
    }
    if (H.nseq > 32767) { g_err = "marker database too large: more than 32,767 sequences (MC_POST8)"; return -1; }
    if (mc_post8_launch(h->d_post, h->d_off, h->d_res, (uint32_t)H.post.size(), h->d_post8, nullptr)) return -1;
    HIPCK(hipDeviceSynchronize());
    MC_OT("  index upload", t0);
    if (H.max_bucket > 2047) { g_err = "a seed bucket holds more than 2047 postings: the hit-order key cannot index it"; return -1; }
    // the position-parallel seed kernel is exact only when the frequency threshold is 0 and no letter frequency is 0
    h->fast_enum = (H.freq_thr == 0) && !H.rec.empty() && !getenv("MC_FORCE_SEQUENTIAL_ENUM");
    for (int g = 0; g < 10; g++) if (!(H.letter_p[g] > 0.0)) h->fast_enum = false;
    return 0;
}

// The directory mc_open() keeps built indexes in (mc_set_index_cache; empty: none).  Process-wide, set before the engines are opened.
static std::mutex g_ixc_mu;
static std::string g_ixc_dir;
extern "C" int mc_set_index_cache(const char *dir)
{
    std::unique_lock<std::mutex> lk(g_ixc_mu);
    g_ixc_dir = dir ? dir : "";
    return 0;
}

// Host only (no GPU): does the index cache give back what was built?  Builds the index, writes it to <dir>, reads it back and
// compares every array; then damages one byte of the file and expects the load to refuse it.  0 = all of that held.
extern "C" int mc_index_cache_check(const char *const *names, const char *const *seqs, int32_t nseq, const char *dir)
{
    McHostIndex A, B, C2;
    std::string err;
    if (!dir || !mc_build_index(A, names, seqs, nseq, err)) { g_err = err.empty() ? "bad argument" : err; return -1; }
    const uint64_t ih = mc_ixc_input_hash(names, seqs, nseq);
    char nm[64]; snprintf(nm, sizeof nm, "/index_%016llx.mcix", (unsigned long long)ih);
    const std::string path = std::string(dir) + nm;
    if (!mc_index_save(A, ih, path.c_str())) { g_err = "cannot write " + path; return -1; }
    if (!mc_index_load(B, ih, nseq, path.c_str())) { g_err = "the file just written was not accepted"; return 1; }
    if (!(A.names == B.names && A.res_code == B.res_code && A.res == B.res && A.off == B.off && A.bstart == B.bstart && A.post == B.post && A.keys == B.keys && A.bitmap == B.bitmap &&
          A.filt == B.filt && A.wild == B.wild && A.pair == B.pair && A.rt == B.rt && A.rec.size() == B.rec.size() &&
          (A.rec.empty() || memcmp(A.rec.data(), B.rec.data(), A.rec.size() * sizeof(McBucketRec)) == 0) && A.rt_mask == B.rt_mask && A.max_bucket == B.max_bucket &&
          A.freq_thr == B.freq_thr && A.nres == B.nres && A.nseq == B.nseq && memcmp(A.letter_p, B.letter_p, sizeof A.letter_p) == 0)) { g_err = "the index read back differs from the one built"; return 2; }
    if (mc_index_load(C2, ih ^ 1, nseq, path.c_str())) { g_err = "a file of other sequences was accepted"; return 3; }
    if (!mc_index_matches_input(B, names, seqs, nseq)) { g_err = "the index read back does not pass the input comparison"; return 6; }
    {   // what the checksum cannot see: a well-formed file that is not the index of these sequences (a hash collision, a stale layout)
        McHostIndex D = B;
        if (D.nres > 0) { D.res[(size_t)D.nres / 2] ^= 1; if (mc_index_matches_input(D, names, seqs, nseq)) { g_err = "an index with another residue was accepted"; return 7; } D.res[(size_t)D.nres / 2] ^= 1; }
        if (!D.post.empty()) { const uint32_t keep = D.post[D.post.size() / 2]; D.post[D.post.size() / 2] = ((uint32_t)nseq << 11); if (mc_index_matches_input(D, names, seqs, nseq)) { g_err = "a posting outside the database was accepted"; return 8; } D.post[D.post.size() / 2] = keep; }
        if (!D.rec.empty()) { D.rec[D.rec.size() / 3].start += 1; if (mc_index_matches_input(D, names, seqs, nseq)) { g_err = "a bucket record outside its bucket was accepted"; return 9; } D.rec[D.rec.size() / 3].start -= 1; }
        if (nseq > 1) { std::vector<const char *> nm2(names, names + nseq); std::swap(nm2[0], nm2[1]); if (mc_index_matches_input(D, nm2.data(), seqs, nseq)) { g_err = "other marker names were accepted"; return 10; } }
    }
    {   // one byte of the payload flipped: the checksum must notice
        FILE *f = fopen(path.c_str(), "r+b");
        if (!f) { g_err = "cannot reopen " + path; return -1; }
        fseek(f, 0, SEEK_END); const long sz = ftell(f);
        fseek(f, sz / 2, SEEK_SET); int c = fgetc(f); fseek(f, sz / 2, SEEK_SET); fputc(c ^ 0x40, f); fclose(f);
        if (mc_index_load(C2, ih, nseq, path.c_str())) { g_err = "a damaged file was accepted"; return 4; }
        f = fopen(path.c_str(), "r+b"); fseek(f, sz / 2, SEEK_SET); fputc(c, f); fclose(f);
        if (truncate(path.c_str(), sz - 9) != 0 || mc_index_load(C2, ih, nseq, path.c_str())) { g_err = "a truncated file was accepted"; return 5; }
    }
    remove(path.c_str());
    return 0;
}

// stat_nres, stat_nseq: the statistics pair of the index (mc_index.h), 0, 0: unset
static mc_handle *open_fasta(const char *const *names, const char *const *seqs, int32_t nseq, const int32_t *marker_family, int32_t nfam, int32_t device, int64_t stat_nres, int32_t stat_nseq)
{
    mc_handle *h = new mc_handle();
    std::string err;
    double t0 = mc_now();
    std::string cache;
    uint64_t ih = 0;
    { std::unique_lock<std::mutex> lk(g_ixc_mu); cache = g_ixc_dir; }
    bool loaded = false;
    if (!cache.empty() && nseq > 0) {
        ih = mc_ixc_input_hash(names, seqs, nseq);
        char nm[64]; snprintf(nm, sizeof nm, "/index_%016llx.mcix", (unsigned long long)ih);
        cache += nm;
        loaded = mc_index_load(h->H, ih, nseq, cache.c_str());
        if (loaded && !mc_index_matches_input(h->H, names, seqs, nseq)) { loaded = false; h->H = McHostIndex(); }   // (not the index of THESE sequences, or offsets out of range: rebuilt)
        MC_OT(loaded ? "index cache: loaded" : "index cache: none / not usable", t0);
    }
    if (!loaded) {
        if (!mc_build_index(h->H, names, seqs, nseq, err)) { delete h; g_err = err; return nullptr; }
        MC_OT("mc_build_index", t0);
        if (!cache.empty()) { (void)mc_index_save(h->H, ih, cache.c_str()); MC_OT("index cache: written", t0); }
    }
    h->H.stat_nres = stat_nres; h->H.stat_nseq = stat_nseq;         // (not part of the cached index: the same segments serve any statistics)
    if (open_impl(h, marker_family, nfam, device) != 0) { std::string e = g_err; mc_close(h); g_err = e; return nullptr; }
    MC_OT("open_impl (device side)", t0);
    return h;
}

extern "C" mc_handle *mc_open(const char *const *names, const char *const *seqs, int32_t nseq, const int32_t *marker_family, int32_t nfam, int32_t device)
{
    return open_fasta(names, seqs, nseq, marker_family, nfam, device, 0, 0);
}

// mc_open on the SEGMENTS of a database whose alignment statistics are those of the unsplit sequences (mc_fold.h): stat_nseq sequences of
// stat_nres residues in all enter the length adjustment and the search space of every table (mc_fill_tables) - bits and loge of an
// alignment are what they would be against the unsplit database - and nothing else
extern "C" mc_handle *mc_open_stats(const char *const *names, const char *const *seqs, int32_t nseq, const int32_t *marker_family, int32_t nfam, int32_t device, int64_t stat_nres, int32_t stat_nseq)
{
    if (stat_nseq < 1 || stat_nres < stat_nseq) { g_err = "mc_open_stats: " + std::to_string(stat_nseq) + " sequences of " + std::to_string(stat_nres) + " residues are no database"; return nullptr; }
    return open_fasta(names, seqs, nseq, marker_family, nfam, device, stat_nres, stat_nseq);
}

extern "C" mc_handle *mc_open_rapdb(const char *rapdb_path, int32_t device)
{
    mc_handle *h = new mc_handle();
    std::string err;
    if (!mc_load_rapdb(h->H, rapdb_path, err)) { delete h; g_err = err; return nullptr; }
    if (open_impl(h, nullptr, 1, device) != 0) { std::string e = g_err; mc_close(h); g_err = e; return nullptr; }
    return h;
}

extern "C" int32_t mc_marker_count(const mc_handle *h) { return h ? h->H.nseq : -1; }
extern "C" const char *mc_marker_name(const mc_handle *h, int32_t i) { return (h && i >= 0 && i < h->H.nseq) ? h->H.names[(size_t)i].c_str() : nullptr; }

extern "C" int mc_set_families(mc_handle *h, const int32_t *marker_family, int32_t nfam)
{
    if (!h || !marker_family) { g_err = "null argument"; return -1; }
    if (nfam < 1 || nfam > 32) { g_err = "1..32 gene families are supported"; return -1; }
    for (int i = 0; i < h->H.nseq; i++) if (marker_family[i] < 0 || marker_family[i] >= nfam) { g_err = "family index out of range"; return -1; }
    HIPCK(hipSetDevice(h->device));
    h->fam.assign(marker_family, marker_family + h->H.nseq);
    h->nfam = nfam;
    HIPCK(hipMemcpy(h->d_fam, h->fam.data(), (size_t)h->H.nseq * 4, hipMemcpyHostToDevice));
    h->run_set = false;                                            // per-family parameters have to be set again
    return 0;
}

// Host only (no GPU): `prerapsearch -d <fasta> -n <path>` - builds the index from the sequences and writes <path> and
// <path>.info in RAPSearch2 2.15's on-disk format.
extern "C" int mc_rapdb_write(const char *const *names, const char *const *seqs, int32_t nseq, const char *path)
{
    McHostIndex A;
    std::string err;
    if (!mc_build_index(A, names, seqs, nseq, err) || !mc_write_rapdb(A, path, err)) { g_err = err; return -1; }
    return 0;
}

// Host only (no GPU): is the database prerapsearch wrote the same index mc_open() builds from these sequences?
// 0 = identical (residues, offsets, buckets, postings in order, suffix keys); > 0 = number of the first differing part.
extern "C" int mc_rapdb_verify(const char *rapdb_path, const char *const *names, const char *const *seqs, int32_t nseq)
{
    McHostIndex A, B;
    std::string err;
    if (!mc_load_rapdb(A, rapdb_path, err) || !mc_build_index(B, names, seqs, nseq, err)) { g_err = err; return -1; }
    if (A.nseq != B.nseq || A.off != B.off) { g_err = "sequence count / offsets differ"; return 1; }
    if (A.res != B.res) { g_err = "residues differ"; return 2; }
    if (A.bstart != B.bstart) { g_err = "bucket sizes differ"; return 3; }
    if (A.post != B.post) { g_err = "posting order differs"; return 4; }
    if (A.keys != B.keys) { g_err = "suffix keys differ"; return 5; }
    if (A.names != B.names) { g_err = "names differ"; return 6; }
    return 0;
}

extern "C" int mc_index_view(const mc_handle *h, const uint8_t **res_codes, const uint32_t **offsets, const uint32_t **bucket_starts, const uint32_t **postings,
                             const uint16_t **keys, int64_t *nres, int64_t *npostings, uint32_t *freq_thr, double letter_p[10])
{
    if (!h) { g_err = "null handle"; return -1; }
    *res_codes = h->H.res_code.data(); *offsets = h->H.off.data(); *bucket_starts = h->H.bstart.data(); *postings = h->H.post.data(); *keys = h->H.keys.data();
    *nres = h->H.nres; *npostings = (int64_t)h->H.post.size(); *freq_thr = h->H.freq_thr;
    for (int i = 0; i < 10; i++) letter_p[i] = h->H.letter_p[i];
    return 0;
}

// the run's own tables (mc_set_run's) to the device: when they are made, and when a borrowed length has ended (McLenBorrow)
static hipError_t run_tables_up(mc_handle *h) { return hipMemcpy(h->d_T, &h->hT, sizeof(McTables), hipMemcpyHostToDevice); }

extern "C" int mc_set_run(mc_handle *h, int32_t read_len, double loge_thr, const double *min_cov, const double *min_score, const int32_t *max_aaid, const int32_t *aln_stat)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (read_len < 18 || read_len > 3 * MC_MAXAA) { g_err = "read_len out of range (18..510)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    double t0 = mc_now();
    mc_fill_tables(h->hT, h->H, read_len, loge_thr);
    MC_OT("set_run: tables", t0);
    if (mc_seg_fx_verify(h->hT, nullptr) != 0) { g_err = "internal: the fixed-point SEG tests disagree with the reference arithmetic"; return -1; }
    MC_OT("set_run: seg_fx_verify", t0);
    tables_change(h);                                              // (a lookahead reads d_T, and its frames have this run's pitch)
    memset(&h->hP, 0, sizeof h->hP);
    h->hP.nfam = h->nfam; h->hP.read_len = read_len;
    for (int f = 0; f < h->nfam; f++) { h->hP.min_cov[f] = min_cov[f]; h->hP.min_score[f] = min_score[f]; h->hP.max_aaid[f] = max_aaid[f]; h->hP.aln_stat[f] = aln_stat[f]; }
    HIPCK(run_tables_up(h));
    if (!h->d_segtab) {   // Seg::getprob of every short window, tabulated once (ln n! does not depend on the run)
        std::vector<uint64_t> tab;
        mc_build_segtab(h->hT.lnfac, tab);
        if (h->d_segtab.alloc(tab.size())) return -1;
        HIPCK(hipMemcpy(h->d_segtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    }
    HIPCK(hipMemcpy(h->d_P, &h->hP, sizeof(McClassPars), hipMemcpyHostToDevice));
    const int newFP = ((read_len / 3 + 2) + 3) & ~3;
    if (newFP != h->FP || read_len != h->read_len) h->ctx.cap_reads = 0;   // pools are sized by read length and frame pitch
    h->read_len = read_len; h->FP = newFP; h->run_set = true;
    h->cls_set = false;                                            // (mc_set_run_classes sets it again behind this)
    MC_OT("set_run: segtab, uploads", t0);
    return 0;
}

static void best_materialize(mc_handle *h);
static int ensure_capacity(mc_handle *h, McCtx &c, int64_t nreads)
{
    if (nreads <= c.cap_reads && h->read_len <= c.pool_len) return 0;   // (pools sized for longer reads fit shorter ones: mc_search_varlen)
    if (h->best_from == &c) best_materialize(h);                   // (the best hits of the range before still lie in the pinned buffer that is about to be replaced)
    ahead_drop(h);                                                  // (both frame buffers are about to be freed)
    double t0 = mc_now();
    int64_t cap = nreads;
    if (cap > (1 << 21) - 1) { g_err = "batch larger than 2097151 reads"; return -1; }
    // pool sizes: generous multiples of what shotgun reads produce (75 seed hits, 23 kept HSPs, 5 gapped extensions per 150 bp
    // read of a real genome), scaled with the read length; a batch that still overflows is split by mc_search
    const int64_t L = h->read_len;
    c.cap_reads = 0;                                                // pools are being replaced: nothing is usable until all of them exist
    c.cap_tasks = (uint32_t)std::min<int64_t>(cap * (L + 32) + (1 << 20) + (int64_t)256 * 32 * MC_EN_BLK, 0x7fffffff);
    const int64_t ev_pad = (int64_t)256 * 8 * (MC_EV_BS / 64) * MC_EV_BLK;   // k_eval_seeds hands both pools out in blocks of MC_EV_BLK slots per wave: room for every wave's partly used last block
    c.cap_gaps = (uint32_t)std::min<int64_t>(cap * (L / 8 + 8) + (1 << 18) + ev_pad, (1 << 27) - 2);   // (k_gap_dedupe keeps task index + 1 in 27 bits of a table entry: more tasks than that overflow the pool and the range is split)
    // (round 4: HSPs L / 3 + 8 per read - 58 at 150 bp, where shotgun reads make 23 - instead of L / 2 + 16, rows 16 per read instead of 48:
    // allocating the pools of a 1 M-read batch took 0.8 s, most of the wall time of the reference's default run; a denser batch is split)
    c.cap_hsps = (uint32_t)std::min<int64_t>(cap * (L / 3 + 8) + (1 << 20) + ev_pad, 0x7fffffff);
    c.cap_rows = (uint32_t)std::min<int64_t>(cap * 16 + (1 << 20), 0x7fffffff);
    if (!carve_fits(cap, c.cap_gaps)) { g_err = "internal: the gap task pool is too small for the lists the ordering and finishing stages keep in it"; return -1; }   // (never, for a batch the library accepts: carve_fits)
    if (c.d_frames_base[0].alloc((size_t)cap * 6 * h->FP + 128) || c.d_frames_base[1].alloc((size_t)cap * 6 * h->FP + 128) || c.d_tasks.alloc(c.cap_tasks) ||
        c.d_gaps.alloc(c.cap_gaps) || c.d_hsps.alloc(c.cap_hsps) || c.d_v.alloc(c.cap_hsps) ||
        c.d_tmp.alloc((size_t)c.cap_hsps * 2) || c.d_k64.alloc(c.cap_hsps) || c.d_hkeys.alloc(c.cap_hsps) || c.d_hplace.alloc(c.cap_hsps) || c.d_places.alloc(c.cap_hsps) || c.d_idx.alloc(c.cap_hsps) ||
        c.d_idxo.alloc(c.cap_hsps) || c.d_heads.alloc((size_t)cap + 2) || c.d_scan.alloc((size_t)4100) || c.d_gsz.alloc(c.cap_hsps) || c.d_nv.alloc((size_t)cap + 1) || c.d_rows.alloc(c.cap_rows) ||
        c.d_low.alloc((size_t)cap + 64) || c.d_cand.alloc((size_t)cap + 64) || c.d_nrow.alloc((size_t)cap + 1) || c.d_rowoff.alloc((size_t)cap + 1) || c.d_best.alloc((size_t)cap + 1) || c.d_bestof.alloc((size_t)cap + 1) ||
        c.d_gws_full.alloc((size_t)MC_GAP_THREADS_FULL * MC_GAP_W) || c.d_retry.alloc((size_t)c.cap_gaps * 2 + (size_t)cap + 1) || c.d_retry2.alloc((size_t)c.cap_gaps * 2) || c.d_gleader.alloc((size_t)c.cap_gaps) ||
        c.d_fout.alloc((size_t)c.cap_gaps * 2))
        return -1;
    c.frames_use(h->ahead.cur);
    for (auto &b : c.d_frames_base) HIPCK(hipMemsetAsync(b, MC_INV, 64, c.stream));
    if (c.h_best.alloc((size_t)cap + 1)) return -1;
    c.h_best_cap = (size_t)cap + 1;
    c.cap_reads = cap; c.pool_len = (int)L;
    HIPCK(hipStreamSynchronize(c.stream));
    MC_OT("ensure_capacity (pools)", t0);
    return 0;
}

// the resident read buffer grown to hold nreads reads of the run's length (capacity in bytes: the read length may change between runs)
static int reads_reserve(mc_handle *h, int64_t nreads)
{
    const int64_t need = nreads * (int64_t)h->read_len + 16;
    if (need > h->cap_own) { reads_change(h); if (h->d_reads.alloc((size_t)need)) return -1; h->cap_own = need; }
    return 0;
}

extern "C" int mc_upload(mc_handle *h, const uint8_t *reads, int64_t nreads)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    HIPCK(hipSetDevice(h->device));
    reads_change(h);
    if (reads_reserve(h, nreads)) return -1;
    if (nreads) HIPCK(hipMemcpyAsync(h->d_reads, reads, (size_t)nreads * h->read_len, hipMemcpyHostToDevice, h->ctx.stream));
    HIPCK(hipStreamSynchronize(h->ctx.stream));
    h->reads_dev = h->d_reads; h->nreads = nreads;
    return 0;
}

extern "C" int mc_attach(mc_handle *h, const void *device_reads, int64_t nreads)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    reads_change(h);
    h->reads_dev = (const uint8_t *)device_reads; h->nreads = nreads;
    return 0;
}

// The pipeline of a range, in five stages.  Each stage only ISSUES work on the range's stream and ends with an asynchronous copy
// of the device counters into pinned host memory; the next stage starts by waiting for that copy (stage_wait) and sizes its
// launches from it.
static int stage_wait(McCtx &c) { HIPCK(hipStreamSynchronize(c.stream)); return 0; }
static int counters_to_host(McCtx &c) { HIPCK(hipMemcpyAsync(c.h_c, c.d_counters, sizeof(uint32_t) * C_N, hipMemcpyDeviceToHost, c.stream)); return 0; }

// The cycle counters of the MC_EXP_TIMING build (DESIGN's cycle tables), printed to stderr and cleared: at the end of the translation
// (stage 'a') and of the finishing (stage 'd').  Without that build: nothing.
#ifdef MC_EXP_TIMING
static int exp_timing_dump(mc_handle *h, McCtx &c, char stage)
{
    ahead_drop(h);                                                  // (a lookahead's kernel adds to the same counters)
    if (stage == 'a') {
        HIPCK(hipStreamSynchronize(c.stream));
        unsigned long long acc[12], cnt[12];
        HIPCK(hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_ts_acc), sizeof acc)); HIPCK(hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_ts_cnt), sizeof cnt));
        const char *nm[12] = {"flags", "advance", "numbering", "class-0 rounds", "class-1 rounds", "reduction", "owners", "mask", "staging", "translation", "write-out", ""};
        const double waves = (double)((c.n + MC_TS_READS - 1) / MC_TS_READS) * MC_TS_WAVES;
        for (int k = 0; k < 11; k++) fprintf(stderr, "ts-timing %-15s %9.1f cycles/wave  %8.2f entries/wave  total %8.1f Mcycles\n", nm[k], (double)acc[k] / waves, (double)cnt[k] / waves, acc[k] / 1e6);
        unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_ts_acc), z, sizeof z)); HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_ts_cnt), z, sizeof z));
    } else {
        HIPCK(hipStreamSynchronize(c.stream)); HIPCK(hipStreamSynchronize(c.side));
        unsigned long long acc[8], cnt[8];
        HIPCK(hipMemcpyFromSymbol(acc, HIP_SYMBOL(g_fh_acc), sizeof acc)); HIPCK(hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_fh_cnt), sizeof cnt));
        {
            unsigned long long fr[8];
            HIPCK(hipMemcpyFromSymbol(fr, HIP_SYMBOL(g_fr_acc), sizeof fr));
            const char *fn[7] = {"groups", "items", "std::sort", "threshold, keys", "heap sort", "rows", "classification"};
            for (int k = 0; k < 7; k++) fprintf(stderr, "fr-timing %-17s total %9.1f Mcycles (thread wall time, summed)\n", fn[k], fr[k] / 1e6);
            unsigned long long z8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_fr_acc), z8, sizeof z8));
            HIPCK(hipMemcpyFromSymbol(fr, HIP_SYMBOL(g_fr_acc2), sizeof fr));
            const char *gn[8] = {"-", "sort by frame", "sort by start, stable", "choice", "sum statistics", "copies", "groups (count)", "groups linked (count)"};
            for (int k = 1; k < 8; k++) fprintf(stderr, "fg-timing %-22s %12.1f M\n", gn[k], fr[k] / 1e6);
            HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_fr_acc2), z8, sizeof z8));
        }
        {
            unsigned long long ev[8];
            HIPCK(hipMemcpyFromSymbol(ev, HIP_SYMBOL(g_ev_acc), sizeof ev));
            const char *en[7] = {"loop, records asked", "survivors queued", "X-drop extension", "HSP, marks", "records written", "residue wait + seed", "growth, gate"};
            for (int k = 0; k < 7; k++) fprintf(stderr, "ev-timing %-21s total %9.1f Mcycles (lane 0 of every wave)\n", en[k], ev[k] / 1e6);
            unsigned long long z8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_ev_acc), z8, sizeof z8));
            unsigned long long tr[4];
            HIPCK(hipMemcpyFromSymbol(tr, HIP_SYMBOL(g_ev_turns), sizeof tr));
            fprintf(stderr, "ev-turns forward: %.1f M lane-turns in %.2f M wave-turns = %.1f lanes of 64; backward: %.1f M in %.2f M = %.1f lanes\n", tr[0] / 1e6, tr[1] / 1e6, tr[1] ? (double)tr[0] / (double)tr[1] : 0.0,
                    tr[2] / 1e6, tr[3] / 1e6, tr[3] ? (double)tr[2] / (double)tr[3] : 0.0);
            HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_ev_turns), z8, sizeof tr));
        }
        const char *nm[8] = {"group starts", "groups", "scan, items", "sort", "threshold, ranks", "heap sort", "rows", "other"};
        for (int k = 0; k < 8; k++) fprintf(stderr, "fh-timing %-17s total %9.1f Mcycles %9llu entries\n", nm[k], acc[k] / 1e6, cnt[k]);
        {
            unsigned long long w[12];
            HIPCK(hipMemcpyFromSymbol(w, HIP_SYMBOL(g_fh_worst), sizeof w));
            fprintf(stderr, "fh-worst read: %llu stacked HSPs, %.3f Mcycles:", w[0] & 0xFFFFF, (double)(w[0] >> 20) / 1e6);
            for (int k = 0; k < 8; k++) fprintf(stderr, " %s %.3f", nm[k], (double)w[1 + k] / 1e6);
            fprintf(stderr, "\n");
            unsigned long long z12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_fh_worst), z12, sizeof z12));
        }
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_fh_acc), z, sizeof z)); HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_fh_cnt), z, sizeof z));
    }
    return 0;
}
#else
static int exp_timing_dump(mc_handle *, McCtx &, char) { return 0; }
#endif

// A0: translation + SEG of the n reads at `reads` into the frames of reads at .. at + n - 1 of the frame buffer `into`, on stream st
// between the events e0 and e1.  It reads the reads, d_T and d_segtab and writes nothing but those frames: a running range reads the
// other buffer, d_low and the counters, and A0 may run beside all of it (ahead_issue).
static int stage_a0(mc_handle *h, McCtx &c, hipStream_t st, const uint8_t *reads, uint8_t *into, int64_t at, int64_t n, hipEvent_t e0, hipEvent_t e1)
{
    uint8_t *frames = into + at * 6 * h->FP;                      // (FP is a multiple of 4: the kernel's word stores stay aligned)
    HIPCK(hipEventRecord(e0, st));
    if (mc_translate_launch(h->d_T, h->d_segtab, reads, h->read_len, h->FP, n, frames, st, &c.ts_staged, &c.ts_narrow)) return -1;
    HIPCK(hipEventRecord(e1, st));
    return 0;
}

// A: the counters cleared, then A0 of the reads no lookahead has translated (range_begin: `covered` of them it has, from the range's
// first), then A1: seed enumeration, seed evaluation (gate, growth, ungapped X-drop).  beside_lookahead: range_begin is about to issue
// a lookahead beside the seed kernel, which leaves it room (mc_enumerate_launch)
static int stage_a(mc_handle *h, McCtx &c, int64_t covered, bool beside_lookahead)
{
    const int64_t n = c.n;
    hipStream_t st = c.stream;
    c.ntasks = c.ngaps = c.gpad = c.nh = c.nheads = c.nrows = c.nbest = c.nsegs = 0;
    HIPCK(hipMemsetAsync(c.d_counters, 0, sizeof(uint32_t) * C_N, st));
    HIPCK(hipMemsetAsync(c.d_stats, 0, sizeof(unsigned long long) * S_N, st));
    if (h->best_only) HIPCK(hipMemsetAsync(c.d_cand, 0, (size_t)n, st));
    HIPCK(hipMemsetAsync(c.d_low, 0, (size_t)n, st));
    c.own_a0 = covered < n;
    if (!c.own_a0) HIPCK(hipEventRecord(c.ev[1], st));             // (the seed kernel's interval starts here: the stream has waited for the lookahead)
    else if (stage_a0(h, c, st, c.reads + covered * h->read_len, c.d_frames, covered, n - covered, c.ev[0], c.ev[1])) return -1;
    if (exp_timing_dump(h, c, 'a')) return -1;
    const McRun R = run_of(h);
    const McSeedBufs B = carve_seed(h, c);
    const McSeedKernel kind = !h->fast_enum ? MC_SEED_PLAIN : h->count_traffic ? MC_SEED_COUNTING : MC_SEED_QUEUES;
    if (mc_enumerate_launch(R, B, n, kind, st, beside_lookahead, &c.seed_shape)) return -1;
    HIPCK(hipEventRecord(c.ev[2], st));
    if (mc_eval_seeds_launch(R, B, kind == MC_SEED_QUEUES, st)) return -1;
    HIPCK(hipEventRecord(c.ev[3], st));
    return counters_to_host(c);
}

// B: gapped extension (mc_gap_launch)
static int stage_b(mc_handle *h, McCtx &c)
{
    hipStream_t st = c.stream;
    if (c.h_c[C_OVERFLOW]) { g_err = "seed task / HSP / gap task buffer overflow"; return -2; }
    c.ntasks = c.h_c[C_TASKS];
    const uint32_t ngaps = c.ngaps = c.h_c[C_GAPS];                 // (slots of the pool: the padding of the waves' last blocks included)
    c.gpad = c.h_c[C_GPAD];
    if (ngaps) {
        uint32_t slots = 1u << 16;
        while (slots < 2 * ngaps) slots <<= 1;
        if (slots > c.gtab_slots) { if (c.d_gtab.alloc((size_t)slots)) return -1; c.gtab_slots = slots; }
        // The flank sort borrows the buffers of the HSP ordering (carve_gap).  The pools are sized so that ordinary batches fit
        // (ensure_capacity); a batch dense in gap tasks that does not is an overflow like any other: the range is run again in halves.
        if (2 * (uint64_t)ngaps > c.cap_hsps) { g_err = "gap task pool larger than the sort buffers"; return -2; }
        if (mc_gap_launch(run_of(h), carve_gap(h, c, slots), ngaps, st)) return -1;
    }
    HIPCK(hipEventRecord(c.ev[4], st));
    return counters_to_host(c);
}

// C: HSPs into per-read segments ordered by (subject, hit order); the reads that can print anything (see k_bin_count)
static int stage_c(mc_handle *h, McCtx &c)
{
    hipStream_t st = c.stream;
    if (c.h_c[C_OVERFLOW]) { g_err = "HSP buffer overflow"; return -2; }
    const uint32_t nslots = c.h_c[C_HSPS];                         // used slots of the pool, the padding of the waves' last blocks included
    c.nh_all = nslots - c.h_c[C_HPAD];
    c.nh = c.nh_all;                                               // (best hits only: the reads that can be classified are selected on the device - cand)
    if (c.nh && mc_order_stage_launch(carve_order(h, c), (uint32_t)c.n, nslots, st, fork_of(c), h->best_only)) return -1;
    HIPCK(hipEventRecord(c.ev[5], st));
    return 0;
}

// D: per-read finishing (linking, ranking, cap, classification), rows into m8 order
static int stage_d(mc_handle *h, McCtx &c)
{
    hipStream_t st = c.stream;
    const uint32_t nh = c.nh, nheads = c.nheads = nh ? (uint32_t)c.n : 0u;   // (every read has a segment, most of them empty or unmarked)
    if (nh && mc_finish_launch(run_of(h), carve_finish(c), nheads, nh, c.first_read_id, h->best_only, st, fork_of(c), h->rows_ever ? (hipEvent_t)h->ev_rows : nullptr)) return -1;
    HIPCK(hipEventRecord(c.ev[6], st));
    if (exp_timing_dump(h, c, 'd')) return -1;
    HIPCK(hipMemcpyAsync(c.h_stats, c.d_stats, sizeof(unsigned long long) * S_N, hipMemcpyDeviceToHost, st));
    return counters_to_host(c);
}

// the rows of a range stay on the device: mc_train_library and the class runs, and the abundance counts when nobody asked for the rows
// (mc_set_abundance with mc_set_keep_rows(h, 0): the kernel has read them where they lie)
static bool rows_stay(const mc_handle *h) { return h->rows_stay || (h->ab.active() && !h->keep_rows); }

// E: rows (final order and ABI layout: McRow == mc_row) and best hits into pinned host memory
static int stage_e(mc_handle *h, McCtx &c)
{
    hipStream_t st = c.stream;
    if (c.nrows && !rows_stay(h)) HIPCK(hipMemcpyAsync(h->pin_slot[h->pin_cur], c.d_rows, sizeof(McRow) * c.nrows, hipMemcpyDeviceToHost, h->rows_stream));   // (the range's stream has been waited for: d_rows is final)
    if (c.nbest) HIPCK(hipMemcpyAsync(c.h_best, c.d_best, sizeof(McBestHit) * c.nbest, hipMemcpyDeviceToHost, st));
    return 0;
}

static void rows_wait(mc_handle *h)
{   // the rows of the last run are on their way to the host: wait for them
    if (h->rows_pending) { (void)hipEventSynchronize(h->ev_rows); h->rows_pending = false; }
}

static void stats_add(mc_stats &tot, const mc_stats &s)
{
    tot.reads += s.reads; tot.seed_tasks += s.seed_tasks; tot.gap_tasks += s.gap_tasks; tot.hsps += s.hsps; tot.rows += s.rows;
    tot.reads_with_rows += s.reads_with_rows; tot.classified += s.classified; tot.bucket_lookups += s.bucket_lookups; tot.key_probes += s.key_probes;
    tot.seed_exact_asks += s.seed_exact_asks; tot.seed_wild_asks += s.seed_wild_asks; tot.seed_pair_asks += s.seed_pair_asks; tot.seed_probes += s.seed_probes;
    tot.ms_translate += s.ms_translate; tot.ms_seed += s.ms_seed; tot.ms_eval += s.ms_eval; tot.ms_gapped += s.ms_gapped;
    tot.ms_sort += s.ms_sort; tot.ms_finish += s.ms_finish; tot.ms_total += s.ms_total;
    tot.range_splits += s.range_splits;
}

static int run_range_once(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id);
static void best_materialize(mc_handle *h);

// The results of a run that is made of several ranges: rows (its own vector, or one of the handle's), best hits, for a class run the
// class of every best hit, and the statistics.  take() adds those of the range that ended last; the front of the next range may be
// running meanwhile (range_begin).
struct McResults {
    std::vector<mc_row> own_rows, &rows;                             // (own_rows first: rows may be bound to it)
    std::vector<mc_best_hit> best; std::vector<uint8_t> tag; mc_stats tot;
    bool want_rows, tagged;
    McResults(bool want_rows_, std::vector<mc_row> *rows_ = nullptr, bool tagged_ = false) : rows(rows_ ? *rows_ : own_rows), want_rows(want_rows_), tagged(tagged_) { memset(&tot, 0, sizeof tot); }
    McResults(const McResults &) = delete;
    void take(mc_handle *h, int tag_ = 0)
    {
        if (want_rows) { rows_wait(h); rows.insert(rows.end(), h->res_rows, h->res_rows + h->n_res_rows); }
        best_materialize(h);
        best.insert(best.end(), h->best.begin(), h->best.end());
        if (tagged) tag.insert(tag.end(), h->best.size(), (uint8_t)tag_);
        stats_add(tot, h->stats);
    }
};

// A range whose seed hits / HSPs / rows overflow the pools sized for ordinary shotgun reads (-2 from the pipeline) is run again in
// halves, and their results joined: the caller sees one range either way.
extern "C" int mc_run_range(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id)
{
    if (h && h->pipe_nout) { g_err = "mc_run_range: ranges begun with mc_range_begin() are still in flight"; return -1; }
    int rc = run_range_once(h, first, count, first_read_id);
    if (rc != -2 || count <= 1) return rc;
    h->split_rows.clear();
    McResults R(true, &h->split_rows);
    R.tot.range_splits = 1;
    int64_t off = 0, step = std::max<int64_t>(1, count / 2);
    while (off < count) {
        const int64_t nb = std::min<int64_t>(step, count - off);
        rc = run_range_once(h, first + off, nb, first_read_id + off);
        if (rc == -2 && nb > 1) { step = std::max<int64_t>(1, nb / 2); R.tot.range_splits++; continue; }
        if (rc) return rc;
        R.take(h);
        off += nb;
    }
    h->res_rows = R.rows.data(); h->n_res_rows = (int64_t)R.rows.size(); h->best.swap(R.best); h->best_from = nullptr; h->stats = R.tot;
    return 0;
}

// A range in two halves.  range_begin ISSUES the front of the range (stage A: translation, seeds, seed evaluation - two thirds of
// its time) and returns at once; range_end does everything else: waits for A, issues and waits for B, C + D, sends the rows on their
// way and fetches the best hits.  mc_run_range is one after the other.  Callers with a stream of ranges (run_stream, bench.py) call
// end(i), begin(i + 1) and THEN look at the results of range i: the device works on the next front while the host collects rows
// and best hits (per 2 M reads of 150 bp 0.4 ms to bring the best hits into read order, whatever the caller does with them, and -
// mc_search with rows - the 270 MB of rows to copy out of the pinned buffer).  The next front may overwrite every pool of the
// range before: what the host still reads of it lies in pinned host memory (rows: two buffers in turn; best hits; the counters
// were taken at range_end), and the rows still leaving the device are waited for by stage D (ev_rows).
static int ahead_issue(mc_handle *h, McCtx &c, int64_t first, int64_t count, hipEvent_t behind);
static bool ahead_fits(const mc_handle *h, const McCtx &c, int64_t first, int64_t count);
// predicts: the range issues the lookahead for the range that follows it contiguously in its set (mc_ahead_predict) itself, behind its
// own A1 launches; otherwise its range_end is told the next range, or there is none (mc_run_range).
static int range_begin(mc_handle *h, McCtx &c, int64_t first, int64_t count, int64_t first_read_id, bool predicts)
{
    if (ensure_capacity(h, c, count)) return -1;
    c.reads = h->reads_dev + first * h->read_len; c.n = count; c.first_read_id = first_read_id; c.first = first; c.predicts = predicts;
    // A lookahead that covers the range has written its frames into the other buffer, which becomes the range's; one that does not is
    // over and the current buffer stays.  Either way the range's stream waits for the lookahead's kernel - one lookahead at most is on
    // the device - between two events: the time of that wait is the range's own, the kernel's interval is not (range_end).
    const int64_t covered = mc_ahead_take(h->ahead, ahead_key(h, first, count));   // (reads of the range, from its first; a longer range translates the rest itself)
    c.frames_use(h->ahead.cur);
    c.waited = h->ahead_wait && hipEventQuery(h->ahead_ev[h->ahead_p][1]) != hipSuccess;   // (a kernel that has ended is not waited for: two events on an idle stream would time the host's pause)
    if (c.waited) {
        HIPCK(hipEventRecord(c.ev_wait[0], c.stream));
        HIPCK(hipStreamWaitEvent(c.stream, h->ahead_ev[h->ahead_p][1], 0));
        HIPCK(hipEventRecord(c.ev_wait[1], c.stream));
    }
    h->ahead_wait = false;
    c.ahead_from = covered ? h->ahead_p : -1;
    if (covered) { h->ahead_used++; h->ahead_p ^= 1; }              // (the lookahead behind this range takes the other pair of events)
    // (the range expected next is known before the seed kernel is launched: beside a lookahead the kernel takes another shape.  The
    // shape is chosen on that prediction: a range whose lookahead is then given up - a walk that leaves the order, a mc_debug_stage
    // between two ranges - has run with twelve waves and nothing beside it, about 0.35 ms per 1 M reads slower; its results are the same)
    int64_t next_first = 0;
    const int64_t next_count = predicts && MC_AHEAD_ON ? mc_ahead_predict(first, count, h->nreads, &next_first) : 0;
    int rc = stage_a(h, c, covered, ahead_fits(h, c, next_first, next_count));
    if (rc) { (void)hipStreamSynchronize(c.stream); return rc; }
    c.busy = true;
    if (next_count > 0) {
        if ((rc = ahead_issue(h, c, next_first, next_count, c.ev[1])) != 0) { (void)hipStreamSynchronize(c.stream); c.busy = false; return rc; }
    }
    return 0;
}

// The translation of the range expected next - reads [first, first + count) of the resident set as it is now - beside the running
// range, into the frame buffer that range does not use: no reader of d_frames has to be waited for.  behind: an event of the running
// range's stream the kernel starts behind, or none.  range_begin gives ev[1], the event in front of its seed kernel: the seed kernel,
// launched right behind it on its own queue, is resident first - beside a lookahead of reads up to 191 bp with 12 waves per CU in one
// workgroup, which leave room for eight translation waves instead of six (mc_enumerate_launch), otherwise with 16, the LDS nearly full -
// so the translation gets what is left of the CUs beside it and floods them when the seed kernel's grid runs out, beside k_eval_seeds.
// Holding k_eval_seeds back until the translation has ended was measured and
// lost: the tail takes 2.3 ms per 2 M reads alone, more than the two cost each other.  Without the event the two
// race for the CUs and the step has two speeds; behind the seed kernel's END it finds k_eval_seeds resident, waits for that and runs
// beside the gapped stage, which then takes as much longer as the translation lasts.  A grid BOUNDED to 256 x G one-wave workgroups
// that loop over the blocks was built and measured too, and lost: a wave takes 110 us per block of ten reads however empty its CU is.
// All of it: DESIGN.md 5.5.  No range larger than the pools.
static bool ahead_fits(const mc_handle *h, const McCtx &c, int64_t first, int64_t count)
{
    return count > 0 && count <= c.cap_reads && h->read_len <= c.pool_len && first >= 0 && first + count <= h->nreads && h->reads_dev;
}
static int ahead_issue(mc_handle *h, McCtx &c, int64_t first, int64_t count, hipEvent_t behind)
{
    if (!ahead_fits(h, c, first, count)) return 0;
    ahead_drop(h);                                                  // (nothing to wait for: range_begin has made the range's stream wait for the lookahead before this one)
    if (behind) HIPCK(hipStreamWaitEvent(h->ahead_stream, behind, 0));
    h->ahead_wait = true;                                           // (from here on something may be in the stream)
    if (stage_a0(h, c, h->ahead_stream, h->reads_dev + first * h->read_len, c.frames_of(mc_ahead_target(h->ahead)), 0, count, h->ahead_ev[h->ahead_p][0], h->ahead_ev[h->ahead_p][1])) { ahead_drop(h); return -1; }
    mc_ahead_offer(h->ahead, ahead_key(h, first, count));
    return 0;
}

// the best hits of the range that ended last, in the order classify_reads meets the reads (input order) - made when somebody asks
static void best_materialize(mc_handle *h)
{
    McCtx *c = h->best_from;
    if (!c) return;
    h->best_from = nullptr;
    const uint32_t nb = h->best_count;                             // (taken at range_end: the front of the next range has reset the context's counts since)
    std::sort(c->h_best.get(), c->h_best + nb, [](const McBestHit &x, const McBestHit &y) { return x.read < y.read; });
    h->best.resize(nb);
    for (uint32_t i = 0; i < nb; i++) { const McBestHit &x = c->h_best[i]; mc_best_hit &o = h->best[i]; o.read = x.read; o.family = x.family; o.aln = x.aln; o.target_len = x.target_len; o.bits = x.bits; }
}

static int range_end(mc_handle *h, McCtx &c, int64_t next_first = 0, int64_t next_count = 0)
{
    c.busy = false;
    h->cls_results = false;
    memset(&h->stats, 0, sizeof h->stats);
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr;
    h->stats.reads = c.n;
    int rc = stage_wait(c);
    if (rc == 0) rc = stage_b(h, c);
    // the next range a caller names (run_stream, run_pieces: it is known only here): behind the gapped stage, beside C + D, where it
    // has been since it exists - beside the gapped kernels it costs them what it takes
    if (rc == 0 && MC_AHEAD_ON && !c.predicts) rc = ahead_issue(h, c, next_first, next_count, c.ev[4]);
    if (rc == 0 && (rc = stage_wait(c)) == 0 && (rc = stage_c(h, c)) == 0) rc = stage_d(h, c);   // (C leaves its counts on the device: D is issued behind it)
    if (rc == 0) rc = stage_wait(c);
    if (rc == 0 && c.h_c[C_OVERFLOW]) { g_err = "row buffer overflow"; rc = -2; }
    if (rc) { (void)hipStreamSynchronize(c.stream); ahead_drop(h); return rc; }   // (-2: the caller answers with mc_run_range on this range, whose A0 writes d_frames)
    h->pin_cur ^= 1;                                                // (the other slot may still be receiving the rows of the run before)
    c.nrows = (c.nh && !h->best_only) ? c.h_c[C_ROWS] : 0u; c.nsegs = c.h_c[C_SEGS]; c.nbest = c.h_c[C_BEST];
    // the abundance counts of the range: its rows are final and none of its pools overflowed - a range that did has returned above
    // and counts nothing; the pieces mc_run_range cuts it into come through here one by one, each once
    const bool abund = h->ab.active() && !h->best_only;
    if (abund && h->ab.launch(c.d_rows, std::min(c.nrows, c.cap_rows), c.stream, c.n)) return -1;
    if ((size_t)c.nrows > h->pin_slot_cap[h->pin_cur] && !rows_stay(h)) {   // grow the pinned row buffer
        (void)hipStreamSynchronize(h->rows_stream);                  // (the copy of the run before writes into the other buffer: let it finish before anything is freed)
        const size_t want = (size_t)c.nrows + c.nrows / 4 + 1024;
        McPin<mc_row> nb, ob;                                      // (made before the old one goes, which the move-assignment frees)
        if (nb.alloc(want)) { g_err = "out of pinned host memory for the rows"; return -1; }
        h->pin_slot[h->pin_cur] = std::move(nb); h->pin_slot_cap[h->pin_cur] = want;
        const int other = h->pin_cur ^ 1;                        // the other slot grows with it (pinning 300 MB takes 40 ms: not in the middle of a later run)
        if (h->pin_slot_cap[other] < want && ob.alloc(want) == 0) { h->pin_slot[other] = std::move(ob); h->pin_slot_cap[other] = want; }
    }
    rc = stage_e(h, c);
    if (rc) { (void)hipStreamSynchronize(c.stream); (void)hipStreamSynchronize(h->rows_stream); return rc; }
    if (c.nrows && !rows_stay(h)) { HIPCK(hipEventRecord(h->ev_rows, h->rows_stream)); h->rows_pending = true; h->rows_ever = true; }
    if ((rc = stage_wait(c)) != 0) return rc;
    if (abund) h->ab.range_done(c.n);
    h->res_rows = rows_stay(h) ? nullptr : (const mc_row *)h->pin_slot[h->pin_cur]; h->n_res_rows = rows_stay(h) ? 0 : (int64_t)c.nrows;
    h->best_from = &c; h->best_count = c.nbest;                  // (mc_result_best_hits / whoever needs them: best_materialize)
#ifdef MC_EXP_TIMING
    { const char *nm[6] = {"staging/other", "append", "lookup", "push", "setup", "expand"}; for (int k = 0; k < 6; k++) fprintf(stderr, "timing %-14s %8.3f Mcycles/wave-avg  %10llu entries\n", nm[k], (double)c.h_stats[4 + k] / 4096.0 / 1e6, c.h_stats[10 + k]); }
#endif
    h->stats.bucket_lookups += (int64_t)c.h_stats[S_LOOKUPS]; h->stats.key_probes += (int64_t)c.h_stats[S_KEYPROBES]; h->stats.seed_tasks += (int64_t)c.h_stats[S_TASKS];
    h->stats.seed_exact_asks += (int64_t)c.h_stats[S_EXACT]; h->stats.seed_wild_asks += (int64_t)c.h_stats[S_WILD]; h->stats.seed_pair_asks += (int64_t)c.h_stats[S_PAIRS]; h->stats.seed_probes += (int64_t)c.h_stats[S_PROBES];
    h->stats.gap_tasks += c.ngaps - c.gpad; h->stats.hsps += c.nh_all; h->stats.rows += c.nrows; h->stats.reads_with_rows += c.nsegs;
    // kernel times: HIP events around the stages
    // ms_translate is the range's own stream's: its A0, where it had one, and the time it waited for a lookahead's kernel - so the six
    // stage times add up to the range.  The lookahead's kernel ran in the background of the range before: mc_ahead_kernel_ms.
    const float ms_tr = (c.own_a0 ? ev_ms(c.ev[0], c.ev[1]) : 0.0f) + (c.waited ? ev_ms(c.ev_wait[0], c.ev_wait[1]) : 0.0f);
    h->ahead_ms = c.ahead_from >= 0 ? ev_ms(h->ahead_ev[c.ahead_from][0], h->ahead_ev[c.ahead_from][1]) : 0.0f;
    h->stats.ms_translate += ms_tr; h->stats.ms_seed += ev_ms(c.ev[1], c.ev[2]); h->stats.ms_eval += ev_ms(c.ev[2], c.ev[3]);
    h->stats.ms_gapped += ev_ms(c.ev[3], c.ev[4]); h->stats.ms_sort += ev_ms(c.ev[4], c.ev[5]); h->stats.ms_finish += ev_ms(c.ev[5], c.ev[6]); h->stats.ms_total += ms_tr + ev_ms(c.ev[1], c.ev[6]);
    h->stats.classified = (int64_t)c.nbest;
    return 0;
}

static int range_check(mc_handle *h, int64_t first, int64_t count)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    if (first < 0 || count < 0 || first + count > h->nreads) { g_err = "range outside the resident read set"; return -1; }
    if (count > (1 << 21) - 1) { g_err = "batch larger than 2097151 reads"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return 0;
}

static int run_range_once(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id)
{
    if (range_check(h, first, count)) return -1;
    if (count == 0) { memset(&h->stats, 0, sizeof h->stats); h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr; return 0; }
    McCtx &c = h->ctx;
    const int rc = range_begin(h, c, first, count, first_read_id, false);
    if (rc) return rc;
    return range_end(h, c);
}

// ---- a stream of ranges: the front of the next one issued before the host looks at the results of this one -------------------------
// mc_range_begin() enqueues the front of a range and returns at once; mc_range_end() completes it (results as after mc_run_range).
// end(i), begin(i + 1), results of i, end(i + 1), ... keeps the device busy while the host works on the results.  One range at a
// time is on the device: a second mc_range_begin() before mc_range_end() is refused.  A range that overflows a pool comes back with
// -2 from mc_range_end: it is no longer in flight; run it with mc_run_range (which splits it).
// mc_range_begin() also LOOKS AHEAD: behind the front of its own range it issues the translation of the range it expects next (the one
// that follows contiguously in the resident set: mc_ahead_predict) on a stream of its own, into the frame buffer its own range does
// not use, beside its seed kernel and seed evaluation; run_stream and run_pieces name their next range at its end, and theirs runs
// behind the gapped stage.  An mc_range_begin() of that range (or of a prefix of it, or of a longer one, which translates the rest on
// top) starts with the seed kernel in that buffer, any other waits for the lookahead's kernel and translates itself (range_begin,
// mc_ahead.h).  mc_run_range() issues none.  4.5 % of a step on top of the 2.8 % of the lookahead behind the gapped stage: DESIGN.md 5.5.
// (Round 4 also measured the whole TAIL of a range - ordering, finishing - running beside the whole front of the next, on ordinary
// streams, on streams of their own priority and on streams with CU masks: it does not pay)
// predicts: mc_range_begin itself; run_stream and run_pieces tell range_end their next range instead (range_end_next)
static int range_begin_checked(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id, bool predicts)
{
    if (range_check(h, first, count)) return -1;
    if (count <= 0) { g_err = "mc_range_begin: an empty range"; return -1; }
    if (h->pipe_nout) { g_err = "mc_range_begin: a range is in flight already (mc_range_end first)"; return -1; }
    const int rc = range_begin(h, h->ctx, first, count, first_read_id, predicts);
    if (rc) return rc;
    h->pipe_nout = 1;
    return 0;
}
extern "C" int mc_range_begin(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id) { return range_begin_checked(h, first, count, first_read_id, true); }

// The end of the range in flight, with a lookahead for the range the caller will begin next (count reads from first of the resident
// set as it is NOW; count 0: none).
static int range_end_next(mc_handle *h, int64_t first, int64_t count) { return range_end(h, h->ctx, first, count); }

extern "C" int64_t mc_ranges_translated_ahead(const mc_handle *h) { return h ? h->ahead_used : 0; }
extern "C" float mc_ahead_kernel_ms(const mc_handle *h) { return h ? h->ahead_ms : 0.0f; }

extern "C" int mc_range_end(mc_handle *h)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout == 0) { g_err = "mc_range_end: no range in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    h->pipe_nout = 0;
    return range_end(h, h->ctx);                                   // (its mc_range_begin has issued the lookahead)
}

extern "C" int mc_ranges_in_flight(const mc_handle *h) { return h ? h->pipe_nout : 0; }

// What the stages of the last mc_run_range() left on the device (the per-stage parity tests compare it with the CPU emulation of
// the same per-thread code - SURVEY.md 7.2): 0 the six frames of every read (rows of *record_bytes = FP bytes), 1 the seed kernel's
// hits (McSeedTask, 16 bytes; read = MC_TASK_NONE: padding of a block of the pool), 2 the gap tasks (McGapTask, 28 bytes), 3 the HSP
// pool (McHsp, 48 bytes: the ungapped HSPs of k_eval_seeds and those of the gapped stage).  Returns the bytes there are (copied if
// they fit cap_bytes), -1 on error.
// 4: the counts of the gapped chain (stage B), three uint32 - the distinct flanks (C_ITEMS), those sent to the second window
// (C_RETRY), those sent to full-size rows (C_RETRY2) - from the host copy of the counters that ended the range: only stage_b's
// kernels touch these three, and the block is cleared by the next range's stage A.  Defined for a range that ran unsplit (after a
// split they are the last piece's).
// 5: the form of k_translate_seg the last range launched, one uint32 - 1 reads staged in LDS, 0 read from global memory.  6: its
// instantiation, one uint32 - 1 narrow (frames of at most 63 residues: reads up to 191 bp), 0 wide.  7: waves per workgroup x workgroups
// per CU of the last seed launch, one uint32 (0: k_enumerate, whose grid is per read).
extern "C" int64_t mc_debug_stage(mc_handle *h, int what, void *dst, int64_t cap_bytes, int32_t *record_bytes)
{
    if (!h || !h->run_set || what < 0 || what > 7) { g_err = "mc_debug_stage: bad argument"; return -1; }
    if (h->pipe_nout) { g_err = "mc_debug_stage: ranges are in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    ahead_drop(h);
    const McCtx &c = h->ctx;
    if (what == 4) {
        if (!c.h_c) { g_err = "mc_debug_stage: no range has run"; return -1; }
        const uint32_t v[3] = {c.h_c[C_ITEMS], c.h_c[C_RETRY], c.h_c[C_RETRY2]};
        if (record_bytes) *record_bytes = (int32_t)sizeof(uint32_t);
        if (dst && (int64_t)sizeof v <= cap_bytes) memcpy(dst, v, sizeof v);
        return (int64_t)sizeof v;
    }
    if (what >= 5) {
        int host = -1;                                              // (a host field of McCtx; -1 until a range has run)
        switch (what) {
        case 5: host = c.ts_staged; break;
        case 6: host = c.ts_narrow; break;
        default: host = c.seed_shape; break;
        }
        if (host < 0) { g_err = "mc_debug_stage: no range has run"; return -1; }
        const uint32_t v = (uint32_t)host;
        if (record_bytes) *record_bytes = (int32_t)sizeof v;
        if (dst && (int64_t)sizeof v <= cap_bytes) memcpy(dst, &v, sizeof v);
        return (int64_t)sizeof v;
    }
    const void *src = nullptr; int64_t bytes = 0; int32_t rec = 0;
    if (what == 0) { src = c.d_frames; rec = h->FP; bytes = c.n * 6 * (int64_t)h->FP; }
    else if (what == 1) { src = c.d_tasks; rec = (int32_t)sizeof(McSeedTask); bytes = (int64_t)c.ntasks * rec; }
    else if (what == 2) { src = c.d_gaps; rec = (int32_t)sizeof(McGapTask); bytes = (int64_t)c.ngaps * rec; }
    else { src = c.d_hsps; rec = (int32_t)sizeof(McHsp); bytes = (int64_t)(c.nh_all + (c.h_c ? c.h_c[C_HPAD] : 0u)) * rec; }
    if (record_bytes) *record_bytes = rec;
    if (dst && bytes && bytes <= cap_bytes) { HIPCK(hipStreamSynchronize(c.stream)); HIPCK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost)); }
    return bytes;
}

extern "C" int mc_set_counting(mc_handle *h, int on)
{
    if (!h) { g_err = "null handle"; return -1; }
    ahead_drop(h);
    h->count_traffic = on != 0;
    return 0;
}

extern "C" int mc_run(mc_handle *h, int64_t first_read_id) { return h ? mc_run_range(h, 0, h->nreads, first_read_id) : -1; }

// The streaming form of the pipeline: batches of reads are fetched from a host-side source into pinned staging memory and
// uploaded by a thread of their own (two staging / device buffers in turn) while the calling thread runs the ranges of the batches
// before - upload and search overlap; and the front of batch k + 1 is issued before the results of batch k are collected
// (range_begin / range_end), so that the device does not wait for the host either.
#define MC_STREAM_BATCH 2000000
static int64_t stream_batch()
{   // reads per batch of the streaming pipeline (MC_STREAM_BATCH in the environment: tests deal small batches)
    if (const char *e = getenv("MC_STREAM_BATCH")) { const long long v = atoll(e); if (v >= 1000 && v <= MC_STREAM_BATCH) return (int64_t)v; }
    return MC_STREAM_BATCH;
}
struct McBatchSlot { uint8_t *pin = nullptr, *dev = nullptr; int64_t n = 0, first = 0; int state = 0; /* 0 free, 1 ready, 2 end / error */ int64_t rc = 0; };

// fetch(dst, max, &first) copies the next batch of at most `max` reads into dst, stores the index of its first read and returns
// how many there were (0: the source has ended; < 0: its error).
static int run_stream(mc_handle *h, const std::function<int64_t(uint8_t *, int64_t, int64_t *)> &fetch, int64_t first_read_id, int64_t expect_reads = 0)
{
    HIPCK(hipSetDevice(h->device));
    if (h->pipe_nout) { g_err = "ranges begun with mc_range_begin() are still in flight"; return -1; }
    ahead_drop(h);                                                  // (a lookahead of the caller's ranges: the pools may be replaced, and the resident set is another from here on)
    const int64_t BMAX = MC_STREAM_BATCH, B = stream_batch(), L = h->read_len;
    double t0 = mc_now();
    // The largest batch of this run: a quarter of the reads the caller expects (a power of two between 256 k and 2 M; 2 M when it
    // does not know).  Staging buffers and pools are sized for it ONCE, before the first batch - pinning 2 x 300 MB and allocating
    // (then re-allocating, as the batches grew) the pools of ever larger batches was 1 s of the 1.2 - 2 s of the reference's
    // default run, one run_pipeline of 1 - 2 M reads per process.
    int64_t bmax_run = B;
    if (B == BMAX && expect_reads > 0) { bmax_run = 262144; while (bmax_run < BMAX && bmax_run * 4 < expect_reads) bmax_run <<= 1; bmax_run = std::min(bmax_run, BMAX); }
    const size_t stage_bytes = (size_t)(bmax_run * L + 64);
    if (h->stage_bytes < stage_bytes) {
        h->stage_bytes = 0;                                          // (a failure below leaves no size behind that a later, smaller run could trust)
        for (int k = 0; k < 2; k++) if (h->stage_pin[k].alloc(stage_bytes) || h->stage_dev[k].alloc(stage_bytes)) return -1;
        h->stage_bytes = stage_bytes;
        MC_OT("run_stream: staging buffers", t0);
    }
    if (!h->copy_stream && h->copy_stream.create()) return -1;
    if (expect_reads > 0 && ensure_capacity(h, h->ctx, std::min<int64_t>(bmax_run, expect_reads))) return -1;
    MC_OT("run_stream: pools", t0);
    McBatchSlot slot[2];
    for (int k = 0; k < 2; k++) { slot[k].pin = h->stage_pin[k]; slot[k].dev = h->stage_dev[k]; }
    std::mutex mu; std::condition_variable cv;
    bool abort_up = false;
    std::string up_err;
    std::thread uploader([&] {
        (void)hipSetDevice(h->device);
        int nb = 0;
        for (int k = 0;; k ^= 1) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return slot[k].state == 0 || abort_up; }); if (abort_up) return; }
            int64_t at = 0;
            // The first batches are small - 256 k, 512 k, 1 M reads, then 2 M: the device starts after 4 ms of parsing instead of 33,
            // which is a third of the wall time of the default run (2 M sampled reads); later batches have the full size, where the
            // fixed cost of a range (~1 ms) no longer shows.
            const int64_t want = B == BMAX ? std::min<int64_t>(bmax_run, (int64_t)262144 << std::min(nb, 3)) : B;
            nb++;
            const int64_t n = fetch(slot[k].pin, want, &at);
            int64_t rc = n;
            if (n > 0) {
                hipError_t e = hipMemcpyAsync(slot[k].dev, slot[k].pin, (size_t)(n * L), hipMemcpyHostToDevice, h->copy_stream);
                if (e == hipSuccess) e = hipStreamSynchronize(h->copy_stream);
                if (e != hipSuccess) { up_err = std::string("upload: ") + hipGetErrorString(e); rc = -1; }
            }
            std::unique_lock<std::mutex> lk(mu);
            slot[k].n = n > 0 ? n : 0; slot[k].first = at; slot[k].rc = rc; slot[k].state = rc > 0 ? 1 : 2;
            cv.notify_all();
            if (rc <= 0) return;
        }
    });
    h->all_rows.clear();
    if (h->keep_rows && expect_reads > 0) h->all_rows.reserve((size_t)expect_reads * 2 + 1024);   // (shotgun reads of real genomes: 1.9 rows per read; untouched pages cost nothing)
    McResults R(h->keep_rows, &h->all_rows);
    const uint8_t *saved_reads = h->reads_dev; const int64_t saved_n = h->nreads;
    // the results of the range that ended last -> those of the stream (called while the front of the next batch runs)
    bool pending = false;
    auto collect = [&]() { if (pending) { pending = false; R.take(h); } };
    auto release = [&](int k) { std::unique_lock<std::mutex> lk(mu); slot[k].state = 0; cv.notify_all(); };
    auto reads_at = [&](int k) { reads_change(h); h->reads_dev = slot[k].dev; h->nreads = slot[k].n; };
    // batch `k` is in flight: its range ends (a pool overflow is answered by mc_run_range: smaller ranges); its results are pending.
    // next >= 0: batch `next` is ready and is begun behind this one - the resident set is ITS slot already (the running range took its
    // reads' address at range_begin), and its translation is issued ahead.
    auto end_batch = [&](int k, int next) -> int {
        if (next >= 0) reads_at(next);
        h->pipe_nout = 0;                                            // (mc_range_end, told the next range)
        int r = range_end_next(h, 0, next >= 0 ? slot[next].n : 0);
        if (r == -2) { reads_at(k); r = mc_run_range(h, 0, slot[k].n, first_read_id + slot[k].first); if (next >= 0) reads_at(next); }
        if (r) return r;
        pending = true;
        release(k);                                                  // (the reads of the batch are no longer needed: the uploader may fill the slot)
        return 0;
    };
    int rc = 0, flying = -1;
    for (int k = 0;; k ^= 1) {
        {   // the next batch is not there yet (the source is the slower side): nothing to overlap with - finish the range in flight now
            bool ready;
            { std::unique_lock<std::mutex> lk(mu); ready = slot[k].state != 0; }
            if (!ready && flying >= 0) { if ((rc = end_batch(flying, -1)) != 0) break; flying = -1; collect(); }
        }
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return slot[k].state != 0; }); }
        if (slot[k].state == 2) { if (slot[k].rc < 0) { rc = (int)slot[k].rc; if (!up_err.empty()) g_err = up_err; } break; }
        if (flying >= 0) { if ((rc = end_batch(flying, k)) != 0) break; flying = -1; }
        else reads_at(k);
        if ((rc = range_begin_checked(h, 0, slot[k].n, first_read_id + slot[k].first, false)) != 0) break;
        flying = k;
        collect();                                                   // the batch before, while the front of this one runs
    }
    if (rc == 0 && flying >= 0) { rc = end_batch(flying, -1); flying = -1; }
    if (rc == 0) collect();
    if (h->pipe_nout) { h->pipe_nout = 0; (void)range_end(h, h->ctx); }   // (after an error: nothing stays in flight)
    ahead_drop(h);                                                   // (nor a lookahead that reads a slot: the uploader may be filling it, and the slots outlive this call only as memory)
    { std::unique_lock<std::mutex> lk(mu); abort_up = true; cv.notify_all(); }
    uploader.join();
    reads_change(h);
    h->reads_dev = saved_reads; h->nreads = saved_n;
    if (rc) return rc;
    h->res_rows = R.rows.data(); h->n_res_rows = (int64_t)R.rows.size(); h->best.swap(R.best); h->best_from = nullptr; h->stats = R.tot;
    return 0;
}

void mc_host_copy(uint8_t *dst, const uint8_t *src, size_t bytes);   // (mc_reader.cpp: a batch copied by several threads)
int32_t mc_reader_class_list(const mc_reader *r, int32_t *out);   // (mc_reader.cpp: the classes a reader was opened with; 0: a single-length reader)
extern "C" int mc_search(mc_handle *h, const uint8_t *reads, int64_t nreads, int64_t first_read_id)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    if (nreads < 0 || (nreads > 0 && !reads)) { g_err = "bad argument"; return -1; }
    const int64_t L = h->read_len;
    int64_t at = 0;
    return run_stream(h, [&](uint8_t *dst, int64_t max_reads, int64_t *first) -> int64_t {
        const int64_t n = std::max<int64_t>(0, std::min(max_reads, nreads - at));
        if (n > 0) mc_host_copy(dst, reads + at * L, (size_t)(n * L));
        *first = at; at += n;
        return n;
    }, first_read_id, nreads);
}

// process_seqfile + search_seqs + classify_reads over n_dev GPUs of this process (the library-owned form of the
// multi-GPU path; one process per GPU + RCCL is microbecensus_amd/distributed.py).  The sampler runs once; batches of
// MC_STREAM_BATCH accepted reads are dealt to the devices in the order they ask for them (reads are independent and keep their
// global ids), every device runs the streaming pipeline on a host thread of its own.  Results stay with the handles
// (mc_result_* per handle); the caller sums what it needs - the per-family accumulators are integers.
extern "C" int mc_search_files_multi(mc_handle *const *handles, int32_t n_dev, mc_reader *r, int64_t first_read_id)
{
    if (!handles || n_dev < 1 || !r) { g_err = "bad argument"; return -1; }
    { int32_t cl[MC_CLS_MAX]; if (mc_reader_class_list(r, cl) > 0) { g_err = "mc_search_files_multi: a reader of length classes (one device: mc_search_files)"; return -1; } }
    for (int d = 0; d < n_dev; d++) {
        if (!handles[d] || !handles[d]->run_set) { g_err = "mc_set_run() must be called first on every handle"; return -1; }
        if (mc_reader_read_len(r) != handles[d]->read_len) { g_err = "the reader trims to another length than mc_set_run() was given"; return -1; }
    }
    if (mc_reader_start(r) != 0) { g_err = mc_reader_last_error(); return -1; }
    const int64_t cap_reads = mc_reader_nreads(r);                  // the reads the sampler may deliver at most (args['nreads']): per device, what to size for
    const int64_t expect = cap_reads > 0 && cap_reads < ((int64_t)1 << 40) ? (cap_reads + n_dev - 1) / n_dev : 0;
    std::mutex deal_mu;
    int64_t next = 0;
    bool ended = false;
    std::vector<int> rcs((size_t)n_dev, 0);
    std::vector<std::string> errs((size_t)n_dev);
    auto work = [&](int d) {
        std::string ferr;
        rcs[(size_t)d] = run_stream(handles[d], [&](uint8_t *dst, int64_t max_reads, int64_t *first) -> int64_t {
            int64_t at;
            { std::unique_lock<std::mutex> lk(deal_mu); if (ended) return 0; at = next; next += max_reads; }
            const int64_t n = mc_reader_fetch(r, at, max_reads, dst);
            if (n < 0) ferr = mc_reader_last_error();
            if (n < max_reads) { std::unique_lock<std::mutex> lk(deal_mu); ended = true; }
            *first = at;
            return n;
        }, first_read_id, expect);
        errs[(size_t)d] = !ferr.empty() ? ferr : std::string(rcs[(size_t)d] ? mc_last_error() : "");
    };
    std::vector<std::thread> th;
    for (int d = 1; d < n_dev; d++) th.emplace_back(work, d);
    work(0);
    for (auto &t : th) t.join();
    const int64_t sampled = mc_reader_join(r);
    for (int d = 0; d < n_dev; d++) if (rcs[(size_t)d] == -3) { g_err = errs[(size_t)d]; return -3; }
    if (sampled == -3) { g_err = mc_reader_last_error(); return -3; }
    for (int d = 0; d < n_dev; d++) if (rcs[(size_t)d]) { g_err = errs[(size_t)d]; return rcs[(size_t)d]; }
    if (sampled < 0) { g_err = mc_reader_last_error(); return (int)sampled; }
    return 0;
}

static int search_files_classes(mc_handle *h, mc_reader *r, int64_t first_read_id);
extern "C" int mc_search_files(mc_handle *h, mc_reader *r, int64_t first_read_id)
{
    int32_t cl[MC_CLS_MAX];
    if (h && r && (h->cls_set || mc_reader_class_list(r, cl) > 0)) return search_files_classes(h, r, first_read_id);   // a class run: both sides must hold the same list
    return mc_search_files_multi(&h, 1, r, first_read_id);
}

// ---- the handle borrowed for other read lengths: mc_search_varlen, the class runs, mc_train_library's reference read lengths ---------
// mc_train_library, mc_community_library and the class runs put the handle in a mode of their own (best hits only or not, rows left
// on the device or not); however they return, the caller's mode comes back
struct McModeGuard {
    mc_handle *h; bool best_only, rows_stay;
    McModeGuard(mc_handle *h_, bool best, bool stay) : h(h_), best_only(h_->best_only), rows_stay(h_->rows_stay) { h->best_only = best; h->rows_stay = stay; }
    McModeGuard(const McModeGuard &) = delete;
    ~McModeGuard() { h->best_only = best_only; h->rows_stay = rows_stay; }
};

// The handle borrowed for other read lengths than the run's (and, in a class run, other classification parameters): its read length,
// frame pitch and resident reads are noted here and come back with close(), and so do the run's tables and parameters on the device
// where use() has replaced them - however the borrower returns.
struct McLenBorrow {
    mc_handle *h; int read_len, FP; const uint8_t *reads_dev; int64_t nreads; bool tables = false, pars = false, open = true;
    explicit McLenBorrow(mc_handle *h_) : h(h_), read_len(h_->read_len), FP(h_->FP), reads_dev(h_->reads_dev), nreads(h_->nreads) { ahead_drop(h); }
    McLenBorrow(const McLenBorrow &) = delete;
    ~McLenBorrow() { (void)close(-1); }
    void set_len(int L) { h->read_len = L; h->FP = ((L / 3 + 2) + 3) & ~3; }
    // the pools for the pieces: sized once, for the longest length, and for the larger of the largest piece and what they held before (a
    // fixed-length run after this one then finds its pools in place)
    int pools(int Lmax, int64_t nmax)
    {
        set_len(Lmax);
        return ensure_capacity(h, h->ctx, std::min<int64_t>(std::max(h->ctx.cap_reads, nmax), (1 << 21) - 1));
    }
    // the handle runs reads of L bases from now on: their tables (mc_fill_tables: the query length enters the E-value), read length and
    // frame pitch (the pools were sized for the longest length), and the classification parameters P where some are given
    int use(int L, const McClassPars *P = nullptr)
    {
        if (h->vl_thr != h->hT.loge_thr) { h->vl_tables.clear(); h->vl_thr = h->hT.loge_thr; }
        auto it = h->vl_tables.find(L);
        if (it == h->vl_tables.end()) { it = h->vl_tables.emplace(L, McTables()).first; mc_fill_tables(it->second, h->H, L, h->vl_thr); }
        tables = true;
        tables_change(h);
        HIPCK(hipMemcpy(h->d_T, &it->second, sizeof(McTables), hipMemcpyHostToDevice));
        if (P) { pars = true; HIPCK(hipMemcpy(h->d_P, P, sizeof(McClassPars), hipMemcpyHostToDevice)); }
        set_len(L);
        return 0;
    }
    // rc is what the borrower has come to: it is returned, or - where it is 0 and the run's tables cannot be put back - that error
    int close(int rc = 0)
    {
        if (!open) return rc;
        open = false;
        tables_change(h); reads_change(h);
        h->read_len = read_len; h->FP = FP; h->reads_dev = reads_dev; h->nreads = nreads;
        hipError_t e = tables ? run_tables_up(h) : hipSuccess;
        if (e == hipSuccess && pars) e = hipMemcpy(h->d_P, &h->hP, sizeof(McClassPars), hipMemcpyHostToDevice);
        if (rc == 0 && e != hipSuccess) { g_err = std::string("restoring the run's tables: ") + hipGetErrorString(e); rc = -1; }
        return rc;
    }
};

// The pieces of a sorted batch through the pipeline, each at its length (and, pars != nullptr, with the parameters pars[tag] of its bin),
// its reads at block_of(piece); results into R, a piece's best hits tagged with its bin.  end(j), begin(j + 1), take(j): the front of
// the next piece runs while the host takes the results of this one.  A piece that overflowed a pool is run again in smaller ranges
// while its length is still the handle's.
template <class BlockOf> static int run_pieces(mc_handle *h, McLenBorrow &len, const std::vector<McPiece> &pieces, BlockOf block_of, const McClassPars *pars, McResults &R)
{
    // (a piece of the same bin as the one before it: same length, tables, parameters and reads - the handle stays as it is, and the
    // piece's translation could be issued ahead)
    auto same_bin = [](const McPiece &a, const McPiece &b) { return a.tag == b.tag && a.L == b.L && a.bin_first == b.bin_first && a.bin_n == b.bin_n; };
    auto begin = [&](const McPiece &q, const McPiece *before) -> int {
        if (!before || !same_bin(*before, q)) {
            if (len.use(q.L, pars ? pars + q.tag : nullptr)) return -1;
            reads_change(h);
            h->reads_dev = block_of(q); h->nreads = q.bin_n;
        }
        return range_begin_checked(h, q.first, q.n, q.bin_first + q.first, false);
    };
    int rc = pieces.empty() ? 0 : begin(pieces[0], nullptr);
    for (size_t j = 0; rc == 0 && j < pieces.size(); j++) {
        const McPiece &q = pieces[j];
        const McPiece *nx = j + 1 < pieces.size() ? &pieces[j + 1] : nullptr;
        const bool ahead = nx && same_bin(q, *nx);
        h->pipe_nout = 0;                                            // (mc_range_end, told the next range: the next piece where it is of this bin, else none)
        h->ab.ride_piece(q.tag);                                     // (a class run the counts ride on: the piece's class, for range_end and the ranges of a rerun)
        rc = range_end_next(h, ahead ? nx->first : 0, ahead ? nx->n : 0);
        if (rc == -2) rc = mc_run_range(h, q.first, q.n, q.bin_first + q.first);
        if (rc) break;
        if (nx && (rc = begin(*nx, &q)) != 0) break;
        R.take(h, q.tag);
    }
    if (h->pipe_nout) { h->pipe_nout = 0; (void)range_end(h, h->ctx); }   // (after an error: nothing stays in flight)
    ahead_drop(h);                                                   // (the blocks the pieces were read from are the caller's)
    return rc;
}

// ---- reads of mixed lengths (mc_search_varlen) ---------------------------------------------------------------------------------
// The reads are bucketed by length on the device (k_varlen.h) and the fixed-length pipeline runs once per bucket, with the tables of
// that length (mc_fill_tables: the query length enters the E-value through the length adjustment) and the classification length of
// mc_set_run().  Ranges are numbered by sorted position (bucket start + rank): perm maps them back to the caller's reads.

// Buckets the nreads reads at d_bases / d_off (offsets from 0, on the device) by length: d_sorted receives every bucket's reads back to
// back at its pitch, start[L] the bucket's first sorted position (start[MC_VL_BINS] = nreads), boff[L] its first byte, perm (device)
// the read index of every sorted position.  Every length has been checked to lie in 1 .. 510 before.
static int vl_bucket(McDevBuf &B, hipStream_t st, const uint8_t *d_bases, const int64_t *d_off, int64_t nreads, int64_t total, uint8_t **d_sorted,
                     uint32_t **d_perm, std::vector<uint32_t> &start, std::vector<int64_t> &boff)
{
    const uint32_t ntiles = (uint32_t)((nreads + MC_VL_TILE - 1) / MC_VL_TILE);
    int64_t *d_boff = nullptr; uint32_t *d_cnt = nullptr, *d_start = nullptr;
    if (B.get(d_sorted, (size_t)total + 64) || B.get(&d_boff, MC_VL_BINS) || B.get(&d_cnt, (size_t)MC_VL_BINS * ntiles) || B.get(&d_start, MC_VL_BINS + 1) ||
        B.get(d_perm, (size_t)nreads)) return -1;
    HIPCK(hipMemsetAsync(*d_sorted + total, 0, 64, st));
    k_vl_hist<<<dim3(ntiles), dim3(MC_VL_BS), 0, st>>>(d_off, nreads, ntiles, d_cnt);
    HIPCK(hipGetLastError());
    k_bin_scan<<<dim3(1), dim3(1024), 0, st>>>(d_cnt, (uint32_t)MC_VL_BINS * ntiles, ntiles, MC_VL_BINS, d_start);
    HIPCK(hipGetLastError());
    k_vl_scatter<<<dim3(ntiles), dim3(MC_VL_BS), 0, st>>>(d_off, nreads, ntiles, d_cnt, *d_perm);
    HIPCK(hipGetLastError());
    start.assign(MC_VL_BINS + 1, 0);
    HIPCK(hipMemcpyAsync(start.data(), d_start, start.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (start[MC_VL_BINS] != (uint32_t)nreads) { g_err = "internal: the length buckets do not hold every read"; return -1; }
    boff.assign(MC_VL_BINS, 0);
    for (int L = 1; L < MC_VL_BINS; L++) boff[(size_t)L] = boff[(size_t)L - 1] + (int64_t)(start[(size_t)L] - start[(size_t)L - 1]) * (L - 1);
    HIPCK(hipMemcpyAsync(d_boff, boff.data(), boff.size() * 8, hipMemcpyHostToDevice, st));
    const int64_t waves = MC_VL_BS / 64;                             // (a bounded grid: the kernel strides over the sorted positions)
    k_vl_gather<<<dim3((unsigned)std::min<int64_t>((nreads + waves - 1) / waves, MC_VL_GATHER_BLOCKS)), dim3(MC_VL_BS), 0, st>>>(d_bases, d_off, *d_perm, nreads, d_start, d_boff, *d_sorted);
    HIPCK(hipGetLastError());
    return 0;
}

// the buckets as the piece cutter takes them (mc_pieces.h): bin L - 1 holds the reads of L bases
static std::vector<McBin> vl_bins(const std::vector<uint32_t> &start)
{
    std::vector<McBin> bins;
    for (int L = 1; L < MC_VL_BINS; L++) bins.push_back({L, (int64_t)(start[(size_t)L + 1] - start[(size_t)L]), (int64_t)start[(size_t)L]});
    return bins;
}

static int search_varlen(mc_handle *h, const uint8_t *bases, const int64_t *offsets, int64_t nreads, int64_t first_read_id)
{
    McCtx &c = h->ctx;
    const int64_t total = offsets[nreads] - offsets[0];
    std::vector<int64_t> off((size_t)nreads + 1);
    for (int64_t i = 0; i <= nreads; i++) off[(size_t)i] = offsets[i] - offsets[0];
    McDevBuf B;
    uint8_t *d_bases = nullptr, *d_sorted = nullptr; int64_t *d_off = nullptr; uint32_t *d_perm = nullptr;
    if (B.get(&d_bases, (size_t)total + 64) || B.get(&d_off, (size_t)nreads + 1)) return -1;
    hipStream_t st = c.stream;
    HIPCK(hipMemcpyAsync(d_bases, bases + offsets[0], (size_t)total, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
    std::vector<uint32_t> start; std::vector<int64_t> boff;
    if (vl_bucket(B, st, d_bases, d_off, nreads, total, &d_sorted, &d_perm, start, boff)) { (void)hipStreamSynchronize(st); return -1; }
    std::vector<uint32_t> perm((size_t)nreads);
    HIPCK(hipMemcpyAsync(perm.data(), d_perm, perm.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    const McPieces P = mc_cut_pieces(vl_bins(start), stream_batch());
    McResults R(h->keep_rows);
    int rc = 0;
    if (!P.v.empty()) {
        McLenBorrow len(h);
        if ((rc = len.pools(P.Lmax, P.nmax)) == 0) rc = run_pieces(h, len, P.v, [&](const McPiece &q) { return d_sorted + boff[(size_t)q.L]; }, nullptr, R);
        rows_wait(h);
        rc = len.close(rc);                                          // the run's own tables back
    }
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr;
    if (rc) return rc;
    // results in the caller's order: rows grouped by original read (stable: a read's rows keep RAPsearch2's order), best hits sorted
    std::vector<int64_t> at((size_t)nreads + 1, 0);
    for (const mc_row &r : R.rows) at[(size_t)perm[(size_t)r.query] + 1]++;
    for (int64_t i = 0; i < nreads; i++) at[(size_t)i + 1] += at[(size_t)i];
    std::vector<mc_row> &out = h->all_rows; out.resize(R.rows.size());
    for (const mc_row &r : R.rows) { const uint32_t o = perm[(size_t)r.query]; mc_row &d = out[(size_t)at[o]++]; d = r; d.query = (int32_t)(first_read_id + o); }
    for (mc_best_hit &b : R.best) b.read = (int32_t)(first_read_id + perm[(size_t)b.read]);
    std::sort(R.best.begin(), R.best.end(), [](const mc_best_hit &x, const mc_best_hit &y) { return x.read < y.read; });
    R.tot.reads += P.nshort;
    h->ab.add_searched(P.nshort);                                    // (reads too short to have a frame: searched, no rows - as mc_stats.reads counts them)
    h->res_rows = out.data(); h->n_res_rows = (int64_t)out.size(); h->best.swap(R.best); h->stats = R.tot;
    return 0;
}

extern "C" int mc_search_varlen(mc_handle *h, const uint8_t *bases, const int64_t *offsets, int64_t nreads, int64_t first_read_id)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    if (nreads < 0 || !offsets || (nreads > 0 && !bases)) { g_err = "bad argument"; return -1; }
    if (nreads > 0x7fffffff) { g_err = "more than 2^31 - 1 reads in one call"; return -1; }
    if (h->pipe_nout) { g_err = "ranges begun with mc_range_begin() are still in flight"; return -1; }
    if (h->ab.curve) { g_err = "mc_search_varlen: refused while the curve is on (mc_set_curve, K = " + std::to_string(h->ab.K) + ") - its rows carry the sorted position, not the caller's read id"; return -1; }
    if (h->ab.cboot.on) { g_err = "mc_search_varlen: refused while the coverage bootstrap is on (mc_set_coverage_bootstrap, capacity = " + std::to_string(h->ab.cboot.cap) + ") - its rows carry the sorted position, not the caller's read id"; return -1; }
    if (h->ab.tboot.on) { g_err = "mc_search_varlen: refused while the tie bootstrap is on (mc_set_tie_bootstrap, capacity = " + std::to_string(h->ab.tboot.cap) + ") - its rows carry the sorted position, not the caller's read id"; return -1; }
    if (h->ab.gboot.on) { g_err = "mc_search_varlen: refused while the gene bootstrap is on (mc_set_gene_bootstrap, capacity = " + std::to_string(h->ab.gboot.cap) + ") - its rows carry the sorted position, not the caller's read id"; return -1; }
    bool one = true;
    for (int64_t i = 0; i < nreads; i++) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len <= 0) { g_err = "read " + std::to_string(i) + " is empty (offsets " + std::to_string(offsets[i]) + ", " + std::to_string(offsets[i + 1]) + ")"; return -1; }
        if (len > 3 * MC_MAXAA) { g_err = "read " + std::to_string(i) + " is " + std::to_string(len) + " bases long: longer than 510"; return -1; }
        one = one && len == h->read_len;
    }
    if (one) return mc_search(h, nreads ? bases + offsets[0] : nullptr, nreads, first_read_id);   // every read of the run's length: the fixed path as it is
    HIPCK(hipSetDevice(h->device));
    return search_varlen(h, bases, offsets, nreads, first_read_id);
}

// ---- reads of mixed lengths, each at its length class (mc_set_run_classes, mc_search_classes) -------------------------------------
// A batch of padded rows is sorted into its classes on the device (k_classes.h) and the fixed-length pipeline runs once per non-empty
// class, cut into ranges as search_varlen cuts its buckets: with the tables of that length (McLenBorrow::use) and - unlike there - the
// classification parameters and length of that class.  No m8 rows: the best hits, their classes and the per-class counts.
extern "C" int mc_set_run_classes(mc_handle *h, const int32_t *class_len, int32_t K, double loge_thr, const double *min_cov, const double *min_score,
                                  const int32_t *max_aaid, const int32_t *aln_stat)
{
    if (!h || !class_len || !min_cov || !min_score || !max_aaid || !aln_stat) { g_err = "null argument"; return -1; }
    int32_t bad = 0;
    const int what = mc_classes_check(class_len, K, &bad);
    if (what == 1) { g_err = "mc_set_run_classes: " + std::to_string(bad) + " length classes (1 .. 32 are supported)"; return -1; }
    if (what == 2) { g_err = "mc_set_run_classes: class length " + std::to_string(bad) + " out of range (18 .. 510)"; return -1; }
    if (what == 3) { g_err = "mc_set_run_classes: class length " + std::to_string(bad) + " does not ascend"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_run_classes: ranges begun with mc_range_begin() are still in flight"; return -1; }
    const size_t F = (size_t)h->nfam, top = (size_t)(K - 1) * F;
    // the handle's single-length state is the top class's: tables, pools and the run's E-value threshold come from mc_set_run
    if (mc_set_run(h, class_len[K - 1], loge_thr, min_cov + top, min_score + top, max_aaid + top, aln_stat + top)) return -1;
    h->cls.K = K;
    h->cls_pars.assign((size_t)K, h->hP);
    for (int k = 0; k < K; k++) {
        h->cls.len[k] = class_len[k];
        McClassPars &P = h->cls_pars[(size_t)k];
        P.read_len = class_len[k];
        for (size_t f = 0; f < F; f++) { P.min_cov[f] = min_cov[k * F + f]; P.min_score[f] = min_score[k * F + f]; P.max_aaid[f] = max_aaid[k * F + f]; P.aln_stat[f] = aln_stat[k * F + f]; }
    }
    h->cls_set = true;
    return 0;
}

struct McClSorted { uint8_t *d_sorted = nullptr; uint32_t *d_perm = nullptr; std::vector<uint32_t> start; McClGather G; float ms[2] = {0, 0}; };

// Sorts the n rows at d_rows (pitch stride, MC_CL_SLACK readable bytes behind them) into the classes of C: S.d_sorted receives every
// class's trimmed reads back to back, class k from byte S.G.word0[k] * 16; S.start[k] is the class's first sorted position
// (start[K]: the rows without a class, start[K + 1] = n), S.d_perm the row index of every sorted position.  ms (ev != nullptr: four
// events): [0] lengths, classes, scan and scatter, [1] the gather.
static int cl_prologue(McDevBuf &B, hipStream_t st, const uint8_t *d_rows, int64_t n, int stride, const McClasses &C, McClSorted &S, hipEvent_t *ev = nullptr)
{
    const uint32_t ntiles = (uint32_t)((n + MC_CL_TILE - 1) / MC_CL_TILE), nbins = (uint32_t)C.K + 1;
    uint8_t *d_cls = nullptr; uint32_t *d_cnt = nullptr, *d_start = nullptr;
    if (B.get(&d_cls, (size_t)n) || B.get(&d_cnt, (size_t)nbins * ntiles) || B.get(&d_start, nbins + 1) || B.get(&S.d_perm, (size_t)n)) return -1;
    if (ev) HIPCK(hipEventRecord(ev[0], st));
    k_cl_hist<<<dim3(ntiles), dim3(MC_CL_BS), 0, st>>>(d_rows, n, stride, C, mc_cl_lanes(stride), ntiles, d_cls, d_cnt);
    HIPCK(hipGetLastError());
    k_bin_scan<<<dim3(1), dim3(1024), 0, st>>>(d_cnt, nbins * ntiles, ntiles, nbins, d_start);
    HIPCK(hipGetLastError());
    k_cl_scatter<<<dim3(ntiles), dim3(MC_CL_BS), 0, st>>>(d_cls, n, ntiles, nbins, d_cnt, S.d_perm);
    HIPCK(hipGetLastError());
    if (ev) HIPCK(hipEventRecord(ev[1], st));
    S.start.assign(nbins + 1, 0);
    HIPCK(hipMemcpyAsync(S.start.data(), d_start, S.start.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (S.start[nbins] != (uint32_t)n) { g_err = "internal: the length classes do not hold every row"; return -1; }
    memset(&S.G, 0, sizeof S.G);
    S.G.K = C.K;
    for (int k = 0; k < C.K; k++) {
        S.G.first[k] = S.start[(size_t)k]; S.G.cnt[k] = S.start[(size_t)k + 1] - S.start[(size_t)k];
        S.G.word0[k + 1] = S.G.word0[k] + ((int64_t)S.G.cnt[k] * C.len[k] + 15) / 16;
    }
    const int64_t W = S.G.word0[C.K];
    if (B.get(&S.d_sorted, (size_t)W * 16 + MC_CL_SLACK)) return -1;
    HIPCK(hipMemsetAsync(S.d_sorted + W * 16, 0, MC_CL_SLACK, st));
    if (ev) HIPCK(hipEventRecord(ev[2], st));
    if (W) {
        k_cl_gather<<<dim3((unsigned)std::min<int64_t>((W + MC_CL_BS - 1) / MC_CL_BS, MC_CL_GATHER_BLOCKS)), dim3(MC_CL_BS), 0, st>>>(d_rows, stride, S.d_perm, C, S.G, S.d_sorted);
        HIPCK(hipGetLastError());
    }
    if (ev) {
        HIPCK(hipEventRecord(ev[3], st));
        HIPCK(hipEventSynchronize(ev[3]));
        S.ms[0] = ev_ms(ev[0], ev[1]); S.ms[1] = ev_ms(ev[2], ev[3]);
    }
    return 0;
}

// one batch of rows, resident at d_rows: its best hits (global read ids, tagged with their class) are added to R, its counts to reads
static int classes_batch(mc_handle *h, const uint8_t *d_rows, int64_t n, int64_t first_read_id, McResults &R, int64_t *reads)
{
    McCtx &c = h->ctx;
    const McClasses &C = h->cls;
    hipStream_t st = c.stream;
    McDevBuf B; McClSorted S;
    if (cl_prologue(B, st, d_rows, n, mc_class_stride(C), C, S)) { (void)hipStreamSynchronize(st); return -1; }
    const int64_t nclassed = (int64_t)S.start[(size_t)C.K];
    std::vector<uint32_t> perm((size_t)nclassed);
    if (nclassed) HIPCK(hipMemcpyAsync(perm.data(), S.d_perm, perm.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    std::vector<McBin> bins;
    for (int k = 0; k < C.K; k++) bins.push_back({C.len[k], (int64_t)S.G.cnt[k], (int64_t)S.G.first[k]});
    const McPieces P = mc_cut_pieces(bins, stream_batch());            // (P.nshort is 0 here: mc_classes_check admits no class under 18 bases)
    for (int k = 0; k <= C.K; k++) reads[k] += (int64_t)(S.start[(size_t)k + 1] - S.start[(size_t)k]);
    R.tot.reads += n - nclassed;
    // the counts ride (mc_set_abundance_classes): the owner holds the batch's id map, S.d_perm and the batch's first id, while the
    // pieces run - every piece's range_end launches the counting kernels on its rows - and lets go of it however this returns
    struct Ride { McAbundance &ab; ~Ride() { ab.ride_end(); } } ride{h->ab};
    if (h->ab.ride_begin(S.d_perm, first_read_id, C.K, st) || h->ab.rows_below(n - nclassed, st)) return -1;
    if (P.v.empty()) return 0;
    const size_t best0 = R.best.size();
    int rc;
    {
        McModeGuard mode(h, h->ab.classes ? false : h->best_only, true);   // (a class run hands out no rows: they stay on the device; under the counts they are made)
        McLenBorrow len(h);
        if ((rc = len.pools(P.Lmax, P.nmax)) == 0)
            rc = run_pieces(h, len, P.v, [&](const McPiece &q) { return S.d_sorted + S.G.word0[q.tag] * 16; }, h->cls_pars.data(), R);
        rc = len.close(rc);                                          // the top class's tables and parameters back
    }
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr;
    if (rc) return rc;
    // sorted positions -> global read ids, ascending (the batches follow each other in read order)
    std::vector<mc_best_hit> &best = R.best; std::vector<uint8_t> &cls = R.tag;
    const size_t nb = best.size() - best0;
    std::vector<std::pair<mc_best_hit, uint8_t>> tmp(nb);
    for (size_t i = 0; i < nb; i++) {
        tmp[i] = {best[best0 + i], cls[best0 + i]};
        tmp[i].first.read = (int32_t)(first_read_id + perm[(size_t)tmp[i].first.read]);
    }
    std::sort(tmp.begin(), tmp.end(), [](const std::pair<mc_best_hit, uint8_t> &x, const std::pair<mc_best_hit, uint8_t> &y) { return x.first.read < y.first.read; });
    for (size_t i = 0; i < nb; i++) { best[best0 + i] = tmp[i].first; cls[best0 + i] = tmp[i].second; }
    return 0;
}

// fetch(dst, max, &first): as run_stream's, rows of the class stride.  The batches are uploaded and searched one after another (the
// sampler of a class reader runs on its own thread beside them).
static int classes_stream(mc_handle *h, const std::function<int64_t(uint8_t *, int64_t, int64_t *)> &fetch, int64_t first_read_id, int64_t expect_reads)
{
    HIPCK(hipSetDevice(h->device));
    const int64_t B = std::max<int64_t>(1, expect_reads > 0 ? std::min(stream_batch(), expect_reads) : stream_batch()), stride = mc_class_stride(h->cls);   // (expect_reads: the most the source can deliver)
    McDevBuf buf;
    uint8_t *d_rows = nullptr; McPin<uint8_t> pin;
    McResults R(false, nullptr, true);                               // (no rows; every best hit tagged with its class)
    int64_t reads[MC_CL_BINS] = {};
    int rc = 0;
    int64_t cap = 0;
    for (;;) {
        int64_t at = 0;
        if (!pin && pin.alloc((size_t)(B * stride))) { g_err = "out of pinned host memory for the rows"; rc = -1; break; }
        const int64_t n = fetch(pin, B, &at);
        if (n < 0) { rc = (int)n; break; }
        if (n == 0) break;
        if (n > cap) { if (buf.get(&d_rows, (size_t)(n * stride) + MC_CL_SLACK)) { rc = -1; break; } cap = n; }   // (the first batch is the largest)
        if (hipMemcpyAsync(d_rows, pin, (size_t)(n * stride), hipMemcpyHostToDevice, h->ctx.stream) != hipSuccess ||
            hipMemsetAsync(d_rows + n * stride, 0, MC_CL_SLACK, h->ctx.stream) != hipSuccess || hipStreamSynchronize(h->ctx.stream) != hipSuccess) { g_err = "upload of the rows failed"; rc = -1; break; }
        if ((rc = classes_batch(h, d_rows, n, first_read_id + at, R, reads)) != 0) break;
        if (n < B) break;
    }
    pin.reset();
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr; h->best_cls.clear();
    if (rc) return rc;
    h->best.swap(R.best); h->best_cls.swap(R.tag); h->stats = R.tot;
    memcpy(h->cls_reads, reads, sizeof h->cls_reads);
    h->cls_results = true;
    return 0;
}

static int classes_ready(mc_handle *h, const char *who)
{
    if (!h || !h->run_set || !h->cls_set) { g_err = std::string(who) + ": mc_set_run_classes() must be called first"; return -1; }
    if (h->pipe_nout) { g_err = std::string(who) + ": ranges begun with mc_range_begin() are still in flight"; return -1; }
    if (h->ab.active() && !h->ab.classes) { g_err = std::string(who) + ": a class run is refused while abundance counting is on (mc_set_abundance)"; return -1; }
    return 0;                                                        // (mc_set_abundance_classes: the counts ride on the class run)
}

extern "C" int mc_search_classes(mc_handle *h, const uint8_t *rows, int64_t nreads, int32_t stride, int64_t first_read_id)
{
    if (classes_ready(h, "mc_search_classes")) return -1;
    if (nreads < 0 || (nreads > 0 && !rows)) { g_err = "bad argument"; return -1; }
    if (nreads > 0x7fffffff) { g_err = "more than 2^31 - 1 reads in one call"; return -1; }
    if (stride != mc_class_stride(h->cls)) { g_err = "mc_search_classes: stride " + std::to_string(stride) + " is not the top class length " + std::to_string(mc_class_stride(h->cls)); return -1; }
    int64_t at = 0;
    return classes_stream(h, [&](uint8_t *dst, int64_t max_reads, int64_t *first) -> int64_t {
        const int64_t n = std::max<int64_t>(0, std::min(max_reads, nreads - at));
        if (n > 0) mc_host_copy(dst, rows + at * stride, (size_t)(n * stride));
        *first = at; at += n;
        return n;
    }, first_read_id, nreads);
}

static int search_files_classes(mc_handle *h, mc_reader *r, int64_t first_read_id)
{
    if (classes_ready(h, "mc_search_files")) return -1;
    int32_t rl[MC_CLS_MAX];
    const int32_t rk = mc_reader_class_list(r, rl);
    if (rk != h->cls.K || memcmp(rl, h->cls.len, sizeof(int32_t) * (size_t)rk) != 0) { g_err = "mc_search_files: the reader's length classes are not those of mc_set_run_classes()"; return -1; }
    if (mc_reader_start(r) != 0) { g_err = mc_reader_last_error(); return -1; }
    int64_t at = 0;
    std::string ferr;
    const int rc = classes_stream(h, [&](uint8_t *dst, int64_t max_reads, int64_t *first) -> int64_t {
        const int64_t n = mc_reader_fetch(r, at, max_reads, dst);
        if (n < 0) ferr = mc_reader_last_error();
        *first = at; if (n > 0) at += n;
        return n;
    }, first_read_id, mc_reader_nreads(r));
    const std::string err = !ferr.empty() ? ferr : std::string(rc ? mc_last_error() : "");
    const int64_t sampled = mc_reader_join(r);
    if (rc == -3) { g_err = err; return -3; }
    if (sampled == -3) { g_err = mc_reader_last_error(); return -3; }
    if (rc) { g_err = err; return rc; }
    if (sampled < 0) { g_err = mc_reader_last_error(); return (int)sampled; }
    return 0;
}

extern "C" int64_t mc_result_best_classes(mc_handle *h, const uint8_t **cls)
{
    if (!h || !cls) return -1;
    if (!h->cls_results) { g_err = "mc_result_best_classes: the last run was not a class run"; return -1; }
    *cls = h->best_cls.data();
    return (int64_t)h->best_cls.size();
}

extern "C" int mc_result_class_reads(mc_handle *h, int64_t *out)
{
    if (!h || !out) { g_err = "null argument"; return -1; }
    if (!h->cls_results) { g_err = "mc_result_class_reads: the last run was not a class run"; return -1; }
    for (int k = 0; k <= h->cls.K; k++) out[k] = h->cls_reads[k];
    return 0;
}

// Test and timing aid: the prologue alone on nreads host rows with the class list of mc_set_run_classes().  perm (nreads values),
// start (K + 2), word0 (K + 1: each class's first 16-byte word of the sorted bytes) and, where they fit sorted_cap, the sorted bytes
// (word0[K] * 16) are copied out; ms[0] lengths + classes + scan + scatter, ms[1] the gather (HIP events).  Returns word0[K] * 16.
extern "C" int64_t mc_debug_classes_prologue(mc_handle *h, const uint8_t *rows, int64_t nreads, int32_t stride, uint32_t *perm, uint32_t *start, int64_t *word0,
                                             uint8_t *sorted, int64_t sorted_cap, float *ms)
{
    if (classes_ready(h, "mc_debug_classes_prologue")) return -1;
    if (nreads < 1 || nreads > (1 << 21) - 1 || !rows) { g_err = "mc_debug_classes_prologue: 1 .. 2097151 rows"; return -1; }
    if (stride != mc_class_stride(h->cls)) { g_err = "mc_debug_classes_prologue: stride " + std::to_string(stride) + " is not the top class length"; return -1; }
    HIPCK(hipSetDevice(h->device));
    hipStream_t st = h->ctx.stream;
    McDevBuf B; McClSorted S;
    uint8_t *d_rows = nullptr;
    const size_t bytes = (size_t)nreads * stride;
    if (B.get(&d_rows, bytes + MC_CL_SLACK)) return -1;
    HIPCK(hipMemcpyAsync(d_rows, rows, bytes, hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(d_rows + bytes, 0, MC_CL_SLACK, st));
    McEvents ev;
    if (ev.make(4)) { g_err = "mc_debug_classes_prologue: cannot create events"; (void)hipStreamSynchronize(st); return -1; }
    if (cl_prologue(B, st, d_rows, nreads, stride, h->cls, S, ev.e.data())) { (void)hipStreamSynchronize(st); return -1; }
    const int64_t nbytes = S.G.word0[h->cls.K] * 16;
    if (perm) HIPCK(hipMemcpyAsync(perm, S.d_perm, (size_t)nreads * 4, hipMemcpyDeviceToHost, st));
    if (sorted && nbytes && nbytes <= sorted_cap) HIPCK(hipMemcpyAsync(sorted, S.d_sorted, (size_t)nbytes, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (start) memcpy(start, S.start.data(), S.start.size() * 4);
    if (word0) memcpy(word0, S.G.word0, sizeof(int64_t) * (size_t)(h->cls.K + 1));
    if (ms) { ms[0] = S.ms[0]; ms[1] = S.ms[1]; }
    return nbytes;
}

// bin nk = reads whose best row passes exactly the first nk (ascending) cut-offs: cut-off j (ascending) counts the bins nk > j
static void grid_counts(const std::vector<unsigned long long> &bins, size_t nbins, int ncp, int n_score, int nfam, const std::vector<int> &order,
                        int64_t *count_hits, int64_t *count_aln, double *count_cov)
{
    const double *bcov = (const double *)(bins.data() + 2 * nbins);
    for (int c = 0; c < ncp; c++)
        for (int f = 0; f < nfam; f++) {
            unsigned long long sh = 0, sa = 0; double sc = 0.0;
            for (int j = n_score - 1; j >= 0; j--) {
                const size_t o = ((size_t)c * (MC_GRID_MAXS + 1) + (size_t)(j + 1)) * (size_t)nfam + (size_t)f;
                sh += bins[o]; sa += bins[nbins + o]; sc += bcov[o];
                const size_t out = ((size_t)c * n_score + (size_t)order[(size_t)j]) * (size_t)nfam + (size_t)f;
                count_hits[out] = (int64_t)sh; count_aln[out] = (int64_t)sa; count_cov[out] = sc;
            }
        }
}

// the grid's parameters, cut-offs in ascending order (order[j]: the caller's index of the j-th smallest)
static int grid_pars(const mc_handle *h, const double *aln_covs, int32_t n_cov, const int32_t *max_pids, int32_t n_pid, const double *min_scores, int32_t n_score,
                     McGridPars &G, std::vector<int> &order)
{
    if (n_cov < 1 || n_cov > MC_GRID_MAXC || n_pid < 1 || n_pid > MC_GRID_MAXP || n_score < 1 || n_score > MC_GRID_MAXS) { g_err = "grid larger than 8 x 8 x 64"; return -1; }
    if (!aln_covs || !max_pids || !min_scores) { g_err = "null argument"; return -1; }
    // (NaN breaks the strict weak ordering std::sort needs; infinities are refused with it: no grid of the training workflow has one)
    for (int i = 0; i < n_cov; i++) if (!std::isfinite(aln_covs[i])) { g_err = "aln_covs[" + std::to_string(i) + "] is not finite"; return -1; }
    for (int i = 0; i < n_score; i++) if (!std::isfinite(min_scores[i])) { g_err = "min_scores[" + std::to_string(i) + "] is not finite"; return -1; }
    memset(&G, 0, sizeof G);
    G.read_len = h->read_len; G.n_cov = n_cov; G.n_pid = n_pid; G.n_score = n_score; G.nfam = h->nfam;
    for (int i = 0; i < n_cov; i++) G.cov[i] = aln_covs[i];
    for (int i = 0; i < n_pid; i++) G.pid[i] = max_pids[i];
    order.resize((size_t)n_score);
    for (int i = 0; i < n_score; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return min_scores[a] < min_scores[b]; });
    for (int i = 0; i < n_score; i++) G.score[i] = min_scores[order[(size_t)i]];
    return 0;
}

extern "C" int mc_grid_classify(mc_handle *h, const double *aln_covs, int32_t n_cov, const int32_t *max_pids, int32_t n_pid, const double *min_scores, int32_t n_score,
                                int64_t *count_hits, int64_t *count_aln, double *count_cov)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    if (!count_hits || !count_aln || !count_cov) { g_err = "null argument"; return -1; }
    McGridPars G; std::vector<int> order;
    if (grid_pars(h, aln_covs, n_cov, max_pids, n_pid, min_scores, n_score, G, order)) return -1;
    HIPCK(hipSetDevice(h->device));
    const int nfam = h->nfam;
    const size_t nbins = (size_t)n_cov * n_pid * (MC_GRID_MAXS + 1) * nfam;
    const size_t nout = (size_t)n_cov * n_pid * n_score * nfam;
    memset(count_hits, 0, nout * 8); memset(count_aln, 0, nout * 8); memset(count_cov, 0, nout * 8);
    const int64_t nrows = h->n_res_rows;
    if (nrows == 0) return 0;
    rows_wait(h);
    McDevBuf buf;
    McRow *d_rows = nullptr; unsigned long long *d_bins = nullptr;
    if (buf.get(&d_rows, (size_t)nrows) || buf.get(&d_bins, nbins * 3)) return -1;
    hipStream_t st = h->ctx.stream;
    HIPCK(hipMemcpyAsync(d_rows, h->res_rows, (size_t)nrows * sizeof(McRow), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(d_bins, 0, nbins * 24, st));
    k_grid_classify<<<dim3((unsigned)((nrows + 127) / 128)), dim3(128), 0, st>>>(G, dev_index(h), h->d_fam, d_rows, nrows, d_bins, d_bins + nbins, (double *)(d_bins + 2 * nbins));
    std::vector<unsigned long long> bins(nbins * 3);
    HIPCK(hipMemcpyAsync(bins.data(), d_bins, nbins * 24, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    grid_counts(bins, nbins, n_cov * n_pid, n_score, nfam, order, count_hits, count_aln, count_cov);
    return 0;
}

// The hit tiles of mc_bootstrap(): about 4096 waves over the grid (hit tiles x replicate tiles of 64), at least 32 hits per tile, at
// most 1024 tiles - a function of (n, B) alone, so a call's cov sums are the same on every run.
static int boot_tiles(int64_t n, int32_t B)
{
    const int64_t rep_tiles = (B + MC_BOOT_LANES - 1) / MC_BOOT_LANES;
    int64_t g = std::min<int64_t>(1024, std::max<int64_t>(32, 4096 / rep_tiles));
    g = std::min<int64_t>(g, (n + 31) / 32);
    return (int)std::max<int64_t>(1, g);
}

extern "C" int mc_bootstrap(mc_handle *h, const mc_best_hit *best, int64_t n, const int32_t *family_stat, int32_t nfam, int32_t B, uint64_t seed,
                            int64_t *sums_i64, double *sums_f64)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!family_stat || !sums_i64 || !sums_f64 || (n > 0 && !best)) { g_err = "null argument"; return -1; }
    if (nfam < 1 || nfam > 32) { g_err = "mc_bootstrap: 1 to 32 families"; return -1; }
    if (B < 1 || B > (1 << 16)) { g_err = "mc_bootstrap: 1 to 65536 replicates"; return -1; }      // (the tiles' partial sums: at most 32 x 33 x B x 8 bytes there)
    if (n < 0 || n > 0x7fffffffll) { g_err = "mc_bootstrap: bad number of best hits"; return -1; }
    McBootPars P; memset(&P, 0, sizeof(P));
    P.nfam = nfam; P.B = B; P.seed = seed;
    for (int f = 0; f < nfam; f++) {
        if (family_stat[f] != MC_BOOT_HITS && family_stat[f] != MC_BOOT_COV && family_stat[f] != MC_BOOT_ALN) { g_err = "mc_bootstrap: aln_stat must be 0 (hits), 1 (cov) or 2 (aln)"; return -1; }
        P.stats |= (uint64_t)family_stat[f] << (2 * f);
    }
    for (int64_t i = 0; i < n; i++)      // (the family indexes the kernel's LDS array)
        if (best[i].family < 0 || best[i].family >= nfam || best[i].read < 0 || best[i].aln < 0 || best[i].target_len < 1) { g_err = "mc_bootstrap: a best hit with a family outside 0 .. nfam - 1, a negative read id or alignment length, or no target length"; return -1; }
    const size_t rows = (size_t)nfam + 1;
    memset(sums_i64, 0, (size_t)B * rows * 8); memset(sums_f64, 0, (size_t)B * (size_t)nfam * 8);
    h->boot_ms = 0;
    if (n == 0) return 0;
    HIPCK(hipSetDevice(h->device));
    const int ntiles = boot_tiles(n, B);
    const int64_t per_tile = (n + ntiles - 1) / ntiles;
    mc_best_hit *d_hits = nullptr; unsigned long long *d_part = nullptr, *d_out = nullptr;
    McDevBuf buf; McEvents ev;
    const size_t nout = (size_t)B * (rows + (size_t)nfam);
    if (buf.get(&d_hits, (size_t)n) || buf.get(&d_part, (size_t)ntiles * rows * (size_t)B) || buf.get(&d_out, nout) || ev.make(2)) return -1;
    hipEvent_t e0 = ev[0], e1 = ev[1];
    hipStream_t st = h->ctx.stream;
    HIPCK(hipMemcpyAsync(d_hits, best, (size_t)n * sizeof(mc_best_hit), hipMemcpyHostToDevice, st));
    HIPCK(hipEventRecord(e0, st));
    k_bootstrap<<<dim3((unsigned)ntiles, (unsigned)((B + MC_BOOT_LANES - 1) / MC_BOOT_LANES)), dim3(MC_BOOT_LANES), 0, st>>>(P, d_hits, n, per_tile, d_part);
    long long *d_i64 = (long long *)d_out; double *d_f64 = (double *)(d_out + (size_t)B * rows);
    k_bootstrap_reduce<<<dim3((unsigned)(((size_t)B * rows + 255) / 256)), dim3(256), 0, st>>>(P, ntiles, d_part, d_i64, d_f64);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(e1, st));
    HIPCK(hipMemcpyAsync(sums_i64, d_i64, (size_t)B * rows * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(sums_f64, d_f64, (size_t)B * (size_t)nfam * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipEventElapsedTime(&h->boot_ms, e0, e1));
    return 0;
}

extern "C" float mc_bootstrap_ms(const mc_handle *h) { return h ? h->boot_ms : 0.0f; }

// ---- the fit of the per-family weights (k_wfit.h; csrc/mc_wfit.h states it) -------------------------------------------------------
// The launch shape of k_wfit_eval for a table of N x F: whether the table is staged in LDS, the waves of a block, the words of LDS a
// wave keeps its errors in, and the dynamic LDS of a block.
struct WfitShape { bool tab_lds; int waves, err_words; size_t lds_bytes; };
static WfitShape wfit_shape(int N, int F)
{
    WfitShape s;
    const size_t tab = (size_t)(F + 2) * (size_t)N * 8;
    s.err_words = (N + 63) / 64 > MC_WFIT_REG_ROUNDS ? N : 0;
    const size_t per_wave = (size_t)s.err_words * 8 + 16;
    s.tab_lds = tab <= MC_WFIT_TAB_LDS && tab + per_wave <= MC_WFIT_LDS_MAX;
    const size_t room = MC_WFIT_LDS_MAX - (s.tab_lds ? tab : 0);
    s.waves = (int)std::max<size_t>(1, std::min<size_t>(MC_WFIT_MAX_WAVES, room / per_wave));
    s.lds_bytes = (s.tab_lds ? tab : 0) + (size_t)s.waves * per_wave;
    return s;
}

// checks the table and makes the device layout of k_wfit.h from it: tab[F + 2][N], alive
static int wfit_table(const char *who, const double *pred, const double *truth, int32_t N, int32_t F, std::vector<double> &tab, uint32_t &alive)
{
    if (F < 1 || F > MC_WFIT_MAX_F) { g_err = std::string(who) + ": 1 to 32 families"; return -1; }
    if (N < 1 || N > MC_WFIT_MAX_N) { g_err = std::string(who) + ": 1 to " + std::to_string(MC_WFIT_MAX_N) + " libraries"; return -1; }
    for (int n = 0; n < N; n++) if (!(truth[n] > 0.0) || std::isinf(truth[n])) { g_err = std::string(who) + ": a true size that is not a positive finite number"; return -1; }
    for (size_t i = 0; i < (size_t)N * F; i++) if (std::isinf(pred[i])) { g_err = std::string(who) + ": an infinite prediction (NaN stands for NA)"; return -1; }
    std::vector<double> pm((size_t)N * F);
    std::vector<uint32_t> keep(N);
    alive = mc_wfit_mask(pred, N, F, pm.data(), keep.data());
    tab.assign((size_t)(F + 2) * N, 0.0);
    for (int n = 0; n < N; n++) {
        for (int f = 0; f < F; f++) tab[(size_t)f * N + n] = pm[(size_t)n * F + f];
        tab[(size_t)F * N + n] = truth[n];
        const uint64_t kb = keep[n];
        memcpy(&tab[(size_t)(F + 1) * N + n], &kb, 8);
    }
    return 0;
}

static void wfit_launch_eval(const WfitShape &sh, int nblocks, hipStream_t st, const McWfitPars &P, const double *d_tab, const McWfitState *d_state, int32_t gen, const double *d_w,
                             double *d_out, unsigned long long *d_best)
{
    if (sh.tab_lds) k_wfit_eval<true><<<dim3((unsigned)nblocks), dim3((unsigned)sh.waves * 64), sh.lds_bytes, st>>>(P, d_tab, d_state, gen, sh.err_words, d_w, d_out, d_best);
    else k_wfit_eval<false><<<dim3((unsigned)nblocks), dim3((unsigned)sh.waves * 64), sh.lds_bytes, st>>>(P, d_tab, d_state, gen, sh.err_words, d_w, d_out, d_best);
}

extern "C" int mc_fit_weights(mc_handle *h, const double *pred, const double *truth, int32_t N, int32_t F, uint64_t seed, int32_t read_len, int32_t C, int32_t G,
                              double *weights, double *trace)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!pred || !truth || !weights || !trace) { g_err = "null argument"; return -1; }
    if (C < 0 || C > MC_WFIT_MAX_C) { g_err = "mc_fit_weights: 0 (the default) to 65536 candidates"; return -1; }
    if (G < -1 || G > MC_WFIT_MAX_G) { g_err = "mc_fit_weights: -1 (the default) to 4096 generations"; return -1; }
    if (C == 0) C = MC_WFIT_C;
    if (G == -1) G = MC_WFIT_G;
    std::vector<double> tab;
    uint32_t alive = 0;
    if (wfit_table("mc_fit_weights", pred, truth, N, F, tab, alive) != 0) return -1;
    h->wfit_ms = 0;
    HIPCK(hipSetDevice(h->device));
    const WfitShape sh = wfit_shape(N, F);
    const int nblocks = (int)std::min<int64_t>(2048, ((int64_t)C + sh.waves - 1) / sh.waves);
    McWfitPars P; memset(&P, 0, sizeof(P));
    P.N = N; P.F = F; P.C = C; P.alive = alive; P.seed = seed; P.L = (uint64_t)(int64_t)read_len;
    McWfitState S0; memset(&S0, 0, sizeof(S0));
    for (int f = 0; f < F; f++) S0.w[f] = 1.0 / (double)F;
    S0.sigma = MC_WFIT_SIGMA0;
    double *d_tab = nullptr, *d_trace = nullptr; McWfitState *d_state = nullptr; unsigned long long *d_best = nullptr;
    McDevBuf buf; McEvents ev;
    const size_t trace_bytes = 3 * (size_t)(G + 1) * 8;
    if (buf.get(&d_tab, tab.size()) || buf.get(&d_trace, trace_bytes / 8) || buf.get(&d_state, 1) || buf.get(&d_best, (size_t)nblocks * 2) || ev.make(2)) return -1;
    hipEvent_t e0 = ev[0], e1 = ev[1];
    hipStream_t st = h->ctx.stream;
    HIPCK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_state, &S0, sizeof(S0), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(d_trace, 0, trace_bytes, st));
    HIPCK(hipEventRecord(e0, st));
    McWfitPars P1 = P; P1.C = 1;                                   // the start: candidate 0 alone
    wfit_launch_eval(sh, 1, st, P1, d_tab, d_state, -1, nullptr, nullptr, d_best);
    k_wfit_update<<<dim3(1), dim3(256), 0, st>>>(P1, d_state, -1, 1, d_best, d_trace);
    for (int g = 0; g < G; g++) {                                  // every generation enqueued; the host takes no part between them
        wfit_launch_eval(sh, nblocks, st, P, d_tab, d_state, g, nullptr, nullptr, d_best);
        k_wfit_update<<<dim3(1), dim3(256), 0, st>>>(P, d_state, g, nblocks, d_best, d_trace);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(e1, st));
    McWfitState S1;
    HIPCK(hipMemcpyAsync(&S1, d_state, sizeof(S1), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(trace, d_trace, trace_bytes, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipEventElapsedTime(&h->wfit_ms, e0, e1));
    for (int f = 0; f < F; f++) weights[f] = S1.w[f];
    return 0;
}

extern "C" int mc_weights_mue(mc_handle *h, const double *pred, const double *truth, int32_t N, int32_t F, const double *w, int32_t K, double *out)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!pred || !truth || (K > 0 && (!w || !out))) { g_err = "null argument"; return -1; }
    if (K < 0 || K > (1 << 24)) { g_err = "mc_weights_mue: 0 to 16777216 weight vectors"; return -1; }
    std::vector<double> tab;
    uint32_t alive = 0;
    if (wfit_table("mc_weights_mue", pred, truth, N, F, tab, alive) != 0) return -1;
    for (size_t i = 0; i < (size_t)K * F; i++) if (!(w[i] >= 0.0 && w[i] <= 1.0)) { g_err = "mc_weights_mue: a weight outside [0, 1]"; return -1; }
    h->wfit_ms = 0;
    if (K == 0) return 0;
    HIPCK(hipSetDevice(h->device));
    const WfitShape sh = wfit_shape(N, F);
    const int nblocks = (int)std::min<int64_t>(4096, ((int64_t)K + sh.waves - 1) / sh.waves);
    McWfitPars P; memset(&P, 0, sizeof(P));
    P.N = N; P.F = F; P.C = K; P.alive = alive;
    double *d_tab = nullptr, *d_w = nullptr, *d_out = nullptr;
    McDevBuf buf; McEvents ev;
    if (buf.get(&d_tab, tab.size()) || buf.get(&d_w, (size_t)K * F) || buf.get(&d_out, (size_t)K) || ev.make(2)) return -1;
    hipEvent_t e0 = ev[0], e1 = ev[1];
    hipStream_t st = h->ctx.stream;
    HIPCK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(d_w, w, (size_t)K * F * 8, hipMemcpyHostToDevice, st));
    HIPCK(hipEventRecord(e0, st));
    wfit_launch_eval(sh, nblocks, st, P, d_tab, nullptr, 0, d_w, d_out, nullptr);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(e1, st));
    HIPCK(hipMemcpyAsync(out, d_out, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipEventElapsedTime(&h->wfit_ms, e0, e1));
    return 0;
}

extern "C" float mc_fit_weights_ms(const mc_handle *h) { return h ? h->wfit_ms : 0.0f; }

extern "C" int mc_set_keep_rows(mc_handle *h, int keep)
{
    if (!h) { g_err = "null handle"; return -1; }
    h->keep_rows = keep != 0;
    return 0;
}

extern "C" int mc_set_best_hits_only(mc_handle *h, int on)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (on && h->ab.active()) { g_err = "mc_set_best_hits_only: refused while abundance counting is on - it needs every m8 row of a read (mc_set_abundance)"; return -1; }
    h->best_only = on != 0;
    return 0;
}

// ---- per-gene read counts for RPKG, coverage breadth and depth, the tie accounting (k_abundance.h, k_coverage.h and k_ties.h state the
// rules) - the counters live in the handle's McAbundance (mc_abund.h) and accumulate over every range that completes (range_end) until
// they are reset.  Here: the arguments are checked, the device is set, the owner is called.
extern "C" int mc_set_abundance(mc_handle *h, int on, int32_t min_ident, int32_t min_aln, double min_bits, double max_loge)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_abundance: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (!on) return h->ab.set_counts(false, McAbundPars());
    if (min_ident < 0 || min_ident > 100) { g_err = "mc_set_abundance: min_ident " + std::to_string(min_ident) + " is not a percent from 0 to 100"; return -1; }
    if (min_aln < 0) { g_err = "mc_set_abundance: min_aln " + std::to_string(min_aln) + " is negative"; return -1; }
    if (min_bits != min_bits) { g_err = "mc_set_abundance: min_bits is NaN"; return -1; }
    if (max_loge != max_loge) { g_err = "mc_set_abundance: max_loge is NaN"; return -1; }
    if (h->best_only) { g_err = "mc_set_abundance: best hits only is on (mc_set_best_hits_only) - abundance needs every m8 row of a read"; return -1; }
    McAbundPars A; A.min_ident = min_ident; A.min_aln = min_aln; A.min_bits = min_bits; A.max_loge = max_loge;
    return h->ab.set_counts(true, A);
}

extern "C" int mc_abundance_reset(mc_handle *h)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.on) { g_err = "mc_abundance_reset: abundance counting is off (mc_set_abundance)"; return -1; }
    if (h->pipe_nout) { g_err = "mc_abundance_reset: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.reset();
}

extern "C" int mc_abundance_read(mc_handle *h, int64_t *reads, int64_t *aligned, int64_t *searched, int64_t *assigned)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.on) { g_err = "mc_abundance_read: abundance counting is off (mc_set_abundance)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_counts(reads, aligned, searched, assigned);
}

extern "C" int mc_set_coverage(mc_handle *h, int on)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_coverage: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (on && !h->ab.on) { g_err = "mc_set_coverage: abundance counting is off (mc_set_abundance) - coverage is that of the reads it counts"; return -1; }
    return h->ab.set_coverage(on != 0);
}

extern "C" int mc_coverage_read(mc_handle *h, int64_t *covered, int64_t *spanned, int64_t *max_depth)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.cov) { g_err = "mc_coverage_read: coverage is off (mc_set_coverage)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_figures(false, covered, spanned, max_depth);
}

extern "C" int mc_coverage_depth(mc_handle *h, uint32_t *depth, int64_t n)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.cov) { g_err = "mc_coverage_depth: coverage is off (mc_set_coverage)"; return -1; }
    if (n != (int64_t)h->ab.nres || !depth) { g_err = "mc_coverage_depth: the array holds " + std::to_string(n) + " values, the database " + std::to_string(h->ab.nres) + " residues"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_depth(depth);
}

extern "C" int mc_set_ties(mc_handle *h, int on, const int32_t *group_of, int32_t ngroups)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_ties: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (!on) return h->ab.set_ties(false, nullptr, 0);
    if (!h->ab.on) { g_err = "mc_set_ties: abundance counting is off (mc_set_abundance) - the ties are those of the reads it counts"; return -1; }
    if (ngroups < 0) { g_err = "mc_set_ties: ngroups " + std::to_string(ngroups) + " is negative"; return -1; }
    if (ngroups > 0 && !group_of) { g_err = "mc_set_ties: " + std::to_string(ngroups) + " groups and a NULL group map"; return -1; }
    if (ngroups == 0) group_of = nullptr;
    for (size_t s = 0; group_of && s < (size_t)h->ab.nseq; s++)                       // (the genes under a fold, mc_set_gene_fold)
        if (group_of[s] < 0 || group_of[s] >= ngroups) { g_err = "mc_set_ties: group_of[" + std::to_string(s) + "] = " + std::to_string(group_of[s]) + " lies outside 0 .. " + std::to_string(ngroups - 1); return -1; }
    return h->ab.set_ties(true, group_of, ngroups);
}

extern "C" int mc_ties_read(mc_handle *h, int64_t *candidates, int64_t *unique, uint64_t *share, int64_t *group_unique, int64_t *ambiguous, int64_t *group_ambiguous)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.ties) { g_err = "mc_ties_read: ties are off (mc_set_ties)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_ties(candidates, unique, share, group_unique, ambiguous, group_ambiguous);
}

extern "C" int mc_ties_coverage_read(mc_handle *h, int64_t *covered_any, int64_t *spanned_any, int64_t *max_depth_any)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.ties) { g_err = "mc_ties_coverage_read: ties are off (mc_set_ties)"; return -1; }
    if (!h->ab.cov) { g_err = "mc_ties_coverage_read: coverage is off (mc_set_coverage)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_figures(true, covered_any, spanned_any, max_depth_any);
}

// the lower median and the truncated sum of every gene's depth (mc_depthstats.h), of the depth or (any != 0) of the any-depth: one selection kernel
extern "C" int mc_depth_stats(mc_handle *h, int32_t keep_percent, int any, int64_t *median, int64_t *trimmed_sum, int64_t *low, int64_t *high)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_depth_stats: a range begun with mc_range_begin() is still in flight (keep_percent = " + std::to_string(keep_percent) + ")"; return -1; }
    if (!mc_ds_keep_ok(keep_percent)) { g_err = "mc_depth_stats: keep_percent " + std::to_string(keep_percent) + " is not a percent from 1 to 100"; return -1; }
    if (!h->ab.cov) { g_err = "mc_depth_stats: coverage is off (mc_set_coverage) - the depths are its difference array's (keep_percent = " + std::to_string(keep_percent) + ")"; return -1; }
    if (any && !h->ab.ties) { g_err = "mc_depth_stats: any = " + std::to_string(any) + " while ties are off (mc_set_ties) - the any-depth is theirs"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_depth_stats(any != 0, keep_percent, median, trimmed_sum, low, high);
}
// the selection kernels' time over the reads since the last zeroing
extern "C" float mc_depth_stats_ms(const mc_handle *h) { return h ? h->ab.dstat_ms : 0.0f; }

// the rarefaction curve: K points (ascending, each >= 1) turn it on and zero every counter; K == 0 turns it off
extern "C" int mc_set_curve(mc_handle *h, int32_t K, const int64_t *points)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_curve: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (K == 0) return h->ab.set_curve(0, nullptr);
    if (h->ab.classes) { g_err = "mc_set_curve: refused while the counts may ride on class runs (mc_set_abundance_classes) - a prefix of mixed lengths has no one length (K = " + std::to_string(K) + ")"; return -1; }
    if (K < 0 || K > MC_CURVE_MAXK) { g_err = "mc_set_curve: K " + std::to_string(K) + " is not a number of points from 0 to " + std::to_string(MC_CURVE_MAXK); return -1; }
    if (!points) { g_err = "mc_set_curve: " + std::to_string(K) + " points and a NULL array"; return -1; }
    if (!h->ab.on) { g_err = "mc_set_curve: abundance counting is off (mc_set_abundance) - the curve is that of the reads it counts (K = " + std::to_string(K) + ")"; return -1; }
    unsigned long long pts[MC_CURVE_MAXK];
    for (int32_t k = 0; k < K; k++) {
        if (points[k] < 1) { g_err = "mc_set_curve: point " + std::to_string(k) + " is " + std::to_string(points[k]) + ": below 1"; return -1; }
        if (k && points[k] < points[k - 1]) { g_err = "mc_set_curve: point " + std::to_string(k) + " is " + std::to_string(points[k]) + ": below the point before it, " + std::to_string(points[k - 1]); return -1; }
        pts[k] = (unsigned long long)points[k];
    }
    return h->ab.set_curve(K, pts);
}

// reads, aligned, covered (or NULL): K x nseq values, point by point; assigned: K values; beyond: the reads behind the last point
extern "C" int mc_curve_read(mc_handle *h, int64_t *reads, int64_t *aligned, int64_t *covered, int64_t *assigned, int64_t *beyond)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.curve) { g_err = "mc_curve_read: the curve is off (mc_set_curve)"; return -1; }
    if (covered && !h->ab.cov) { g_err = "mc_curve_read: covered asked for with coverage off (mc_set_coverage; K = " + std::to_string(h->ab.K) + ")"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_curve(reads, aligned, covered, assigned, beyond);
}

// the number of points the curve is on with; 0: off
extern "C" int32_t mc_curve_k(const mc_handle *h) { return h && h->ab.curve ? h->ab.K : 0; }

// k_curve's time over the completed ranges plus the scans' at the reads, since the last zeroing
extern "C" float mc_curve_ms(const mc_handle *h) { return h ? h->ab.curve_ms + h->ab.cscan_ms : 0.0f; }

// the bootstrap of the counts: a list of `capacity` entries turns it on and zeroes every counter; capacity == 0 turns it off
extern "C" int mc_set_gene_bootstrap(mc_handle *h, int64_t capacity)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_gene_bootstrap: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (capacity == 0) return h->ab.set_gene_bootstrap(0);
    if (capacity < 0 || capacity > 0x7fffffffll) { g_err = "mc_set_gene_bootstrap: capacity " + std::to_string(capacity) + " is not a number of reads from 0 to 2^31 - 1"; return -1; }
    if (!h->ab.on) { g_err = "mc_set_gene_bootstrap: abundance counting is off (mc_set_abundance) - the replicates are those of the reads it counts (capacity = " + std::to_string(capacity) + ")"; return -1; }
    return h->ab.set_gene_bootstrap(capacity);
}

// counts (or NULL): nseq x B replicate counts; stats: nseq x 6 doubles (mc_geneboot.h); dropped: the assigned reads that did not fit
extern "C" int mc_gene_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const double *scale, int64_t *counts, double *stats, int64_t *dropped)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.gboot.on) { g_err = "mc_gene_bootstrap: the gene bootstrap is off (mc_set_gene_bootstrap)"; return -1; }
    if (B < 1 || B > MC_GB_MAXB) { g_err = "mc_gene_bootstrap: B " + std::to_string(B) + " is not a number of replicates from 1 to " + std::to_string(MC_GB_MAXB); return -1; }
    if (!scale || !stats) { g_err = "mc_gene_bootstrap: B = " + std::to_string(B) + " and a NULL scale or stats array"; return -1; }
    if (h->pipe_nout) { g_err = "mc_gene_bootstrap: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_gene_bootstrap(B, seed, scale, counts, stats, dropped);
}

// the bootstrap of the groups table (mc_groupboot.h): counts (or NULL): ngroups x B group replicate counts; stats: ngroups x 6 doubles
extern "C" int mc_group_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const double *scale, const int32_t *group_of, int32_t ngroups, const double *gene_kb, int64_t *counts,
                                  double *stats, int64_t *dropped)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.gboot.on) { g_err = "mc_group_bootstrap: the gene bootstrap is off (mc_set_gene_bootstrap)"; return -1; }
    if (B < 1 || B > MC_GB_MAXB) { g_err = "mc_group_bootstrap: B " + std::to_string(B) + " is not a number of replicates from 1 to " + std::to_string(MC_GB_MAXB); return -1; }
    if (!scale || !stats || !group_of || !gene_kb) { g_err = "mc_group_bootstrap: B = " + std::to_string(B) + " and a NULL scale, group_of, gene_kb or stats array"; return -1; }
    const int32_t nseq = h->ab.nseq;
    if (ngroups < 1 || ngroups > nseq) { g_err = "mc_group_bootstrap: ngroups " + std::to_string(ngroups) + " is not a number of groups from 1 to " + std::to_string(nseq) + ", the genes"; return -1; }
    for (int32_t s = 0; s < nseq; s++) {
        if (group_of[s] < 0 || group_of[s] >= ngroups) { g_err = "mc_group_bootstrap: group_of[" + std::to_string(s) + "] = " + std::to_string(group_of[s]) + " is not a group from 0 to " + std::to_string(ngroups - 1); return -1; }
        if (!(gene_kb[s] > 0.0 && gene_kb[s] <= 1.7976931348623157e308)) { g_err = "mc_group_bootstrap: gene_kb[" + std::to_string(s) + "] = " + std::to_string(gene_kb[s]) + " is not a finite number > 0"; return -1; }
    }
    if (h->pipe_nout) { g_err = "mc_group_bootstrap: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_group_bootstrap(B, seed, scale, group_of, ngroups, gene_kb, counts, stats, dropped);
}

// the bootstrap of the tie shares (mc_tieboot.h; it extends mc_set_gene_bootstrap from the counts to the shares of mc_set_ties): a list of
// `capacity` entries turns it on and zeroes every counter; capacity == 0 turns it off
extern "C" int mc_set_tie_bootstrap(mc_handle *h, int64_t capacity)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_tie_bootstrap: a range begun with mc_range_begin() is still in flight (capacity = " + std::to_string(capacity) + ")"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (capacity == 0) return h->ab.set_tie_bootstrap(0);
    if (capacity < 0 || capacity > (int64_t)MC_TB_MAXCAP) { g_err = "mc_set_tie_bootstrap: capacity " + std::to_string(capacity) + " is not a number of entries from 0 to 2^27"; return -1; }
    if (!h->ab.ties) { g_err = "mc_set_tie_bootstrap: ties are off (mc_set_ties) - the entries are the tied sets it counts (capacity = " + std::to_string(capacity) + ")"; return -1; }
    if (!h->ab.gboot.on) { g_err = "mc_set_tie_bootstrap: the gene bootstrap is off (mc_set_gene_bootstrap) - the replicates are its replicates (capacity = " + std::to_string(capacity) + ")"; return -1; }
    return h->ab.set_tie_bootstrap(capacity);
}

// shares (or NULL): nseq x B replicate shares in units of 2^-32; stats: nseq x 6 doubles (mc_tieboot.h); dropped: the entries that did not fit
extern "C" int mc_tie_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const double *scale, uint64_t *shares, double *stats, int64_t *dropped)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.tboot.on) { g_err = "mc_tie_bootstrap: the tie bootstrap is off (mc_set_tie_bootstrap)"; return -1; }
    if (B < 1 || B > MC_GB_MAXB) { g_err = "mc_tie_bootstrap: B " + std::to_string(B) + " is not a number of replicates from 1 to " + std::to_string(MC_GB_MAXB); return -1; }
    if (!scale || !stats) { g_err = "mc_tie_bootstrap: B = " + std::to_string(B) + " and a NULL scale or stats array"; return -1; }
    if (h->pipe_nout) { g_err = "mc_tie_bootstrap: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_tie_bootstrap(B, seed, scale, shares, stats, dropped);
}

// the bootstrap of the coverage columns (mc_covboot.h): a list of `capacity` entries turns it on and zeroes every counter; capacity == 0 turns it off
extern "C" int mc_set_coverage_bootstrap(mc_handle *h, int64_t capacity)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_coverage_bootstrap: a range begun with mc_range_begin() is still in flight (capacity = " + std::to_string(capacity) + ")"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (capacity == 0) return h->ab.set_coverage_bootstrap(0);
    if (capacity < 0 || capacity > (int64_t)MC_CB_MAXCAP) { g_err = "mc_set_coverage_bootstrap: capacity " + std::to_string(capacity) + " is not a number of entries from 0 to 2^31 - 1"; return -1; }
    if (!h->ab.active()) { g_err = "mc_set_coverage_bootstrap: the counts are off (mc_set_abundance) - the entries are the reads they assign (capacity = " + std::to_string(capacity) + ")"; return -1; }
    if (!h->ab.cov) { g_err = "mc_set_coverage_bootstrap: coverage is off (mc_set_coverage) - the entries are the spans it marks (capacity = " + std::to_string(capacity) + ")"; return -1; }
    return h->ab.set_coverage_bootstrap(capacity);
}

// need (or NULL): nseq values, none 0; covered (or NULL): nseq x B covered residues; stats: nseq x 6 doubles (mc_covboot.h); detected (or NULL;
// only with need): nseq counts; dropped: the assigned reads that did not fit
extern "C" int mc_coverage_bootstrap(mc_handle *h, int32_t B, uint64_t seed, const uint32_t *need, int64_t *covered, double *stats, int64_t *detected, int64_t *dropped)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.cboot.on) { g_err = "mc_coverage_bootstrap: the coverage bootstrap is off (mc_set_coverage_bootstrap)"; return -1; }
    if (B < 1 || B > MC_GB_MAXB) { g_err = "mc_coverage_bootstrap: B " + std::to_string(B) + " is not a number of replicates from 1 to " + std::to_string(MC_GB_MAXB); return -1; }
    if (!stats) { g_err = "mc_coverage_bootstrap: B = " + std::to_string(B) + " and a NULL stats array"; return -1; }
    if (detected && !need) { g_err = "mc_coverage_bootstrap: detected without need (B = " + std::to_string(B) + ") - a replicate detects a gene that covers need[g] residues"; return -1; }
    for (int32_t s = 0; need && s < h->ab.nseq; s++)
        if (need[s] == 0) { g_err = "mc_coverage_bootstrap: need[" + std::to_string(s) + "] = 0 - every replicate would detect the gene; the least is 1"; return -1; }
    if (h->pipe_nout) { g_err = "mc_coverage_bootstrap: a range begun with mc_range_begin() is still in flight"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_coverage_bootstrap(B, seed, need, covered, stats, detected, dropped);
}

// the counts on class runs: mc_search_classes and mc_search_files on a class reader are no longer refused, every piece adds to the
// counts and to the per-class table (k_abund_classes.h), and the gene bootstrap takes the read ids through the batch's id map
extern "C" int mc_set_abundance_classes(mc_handle *h, int on)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_abundance_classes: a range begun with mc_range_begin() is still in flight (on = " + std::to_string(on) + ")"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (!on) return h->ab.set_classes(false);
    if (!h->ab.on) { g_err = "mc_set_abundance_classes: abundance counting is off (mc_set_abundance) - the classes are those of the reads it counts (on = " + std::to_string(on) + ")"; return -1; }
    if (h->ab.curve) { g_err = "mc_set_abundance_classes: refused while the curve is on (mc_set_curve, K = " + std::to_string(h->ab.K) + ") - a prefix of mixed lengths has no one length (on = " + std::to_string(on) + ")"; return -1; }
    return h->ab.set_classes(true);
}

// the identity of the assigned reads (mc_identity.h): a histogram of the best rows' identities and three sums per gene; on zeroes every counter
extern "C" int mc_set_identity(mc_handle *h, int on)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_identity: a range begun with mc_range_begin() is still in flight (on = " + std::to_string(on) + ")"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (on && !h->ab.on) { g_err = "mc_set_identity: abundance counting is off (mc_set_abundance) - the identities are those of the reads it counts (on = " + std::to_string(on) + ")"; return -1; }
    return h->ab.set_identity(on != 0);
}

// levels: nlevels of them, 0 .. MC_ID_LEVELS, each 0 .. 100, strictly ascending; every output array holds nseq values (ge: nseq x nlevels) or is NULL
extern "C" int mc_identity_read(mc_handle *h, const int32_t *levels, int32_t nlevels, int64_t *matched, int64_t *mismatched, int64_t *gap_opens, int32_t *ident_min, int32_t *ident_median,
                                int32_t *ident_max, int64_t *ge)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.ident) { g_err = "mc_identity_read: the identity is off (mc_set_identity)"; return -1; }
    if (nlevels < 0 || nlevels > MC_ID_LEVELS) { g_err = "mc_identity_read: nlevels " + std::to_string(nlevels) + " is not a number of levels from 0 to " + std::to_string(MC_ID_LEVELS); return -1; }
    if (nlevels > 0 && !levels) { g_err = "mc_identity_read: " + std::to_string(nlevels) + " levels and a NULL array"; return -1; }
    const int bad = mc_id_bad_level(levels, nlevels);
    if (bad >= 0) {
        g_err = "mc_identity_read: level " + std::to_string(bad) + " is " + std::to_string(levels[bad]) +
                (levels[bad] < 0 || levels[bad] > 100 ? ": not a percent from 0 to 100" : ": not above the level before it, " + std::to_string(levels[bad - 1]));
        return -1;
    }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_identity(levels, nlevels, matched, mismatched, gap_opens, ident_min, ident_median, ident_max, nlevels ? ge : nullptr);
}

// hist: nseq x MC_ID_BINS counters, gene by gene
extern "C" int mc_identity_hist(mc_handle *h, uint32_t *hist)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.ident) { g_err = "mc_identity_hist: the identity is off (mc_set_identity)"; return -1; }
    if (!hist) { g_err = "mc_identity_hist: a NULL array for " + std::to_string(h->ab.nseq) + " genes"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_identity_hist(hist);
}
// k_identity's time over the completed ranges, and the scans' of the reads, since the last zeroing
extern "C" float mc_identity_ms(const mc_handle *h) { return h ? h->ab.ident_ms : 0.0f; }
extern "C" float mc_identity_scan_ms(const mc_handle *h) { return h ? h->ab.iscan_ms : 0.0f; }

// ---- the gene fold (mc_fold.h): the index holds the segments of long genes, every abundance table the genes.  seg_gene[s], seg_off[s]: the
// gene and the offset in it of segment s of the index, gene_len[g]: the residues of gene g.  Checked here against the index's own segment
// lengths - every value that is refused is named - and handed to the owner as records (mc_fold_seg's lo and hi from the same facts).
// ngenes == 0: off.  From here on every size the abundance ABI speaks of (mc_abundance_count and the arrays of the readers) is the genes'.
extern "C" int mc_set_gene_fold(mc_handle *h, int32_t ngenes, const int32_t *seg_gene, const int32_t *seg_off, const int32_t *gene_len)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_set_gene_fold: a range begun with mc_range_begin() is still in flight (ngenes = " + std::to_string(ngenes) + ")"; return -1; }
    HIPCK(hipSetDevice(h->device));
    const int32_t nseq = h->H.nseq;
    const auto refuse_sizes = [&](int32_t ng, size_t nr) {
        g_err = "mc_set_gene_fold: abundance counting is on with tables of " + std::to_string(h->ab.nseq) + " sequences and " + std::to_string(h->ab.nres) + " residues, the fold asks for " +
                std::to_string(ng) + " and " + std::to_string(nr) + " (mc_set_abundance off first)";
        return -1;
    };
    if (ngenes == 0) {
        if (h->ab.on && !h->ab.fold_keeps_sizes(0, 0)) return refuse_sizes(nseq, (size_t)h->H.nres);
        return h->ab.set_fold(0, nullptr, nullptr);
    }
    if (ngenes < 0 || ngenes > nseq) { g_err = "mc_set_gene_fold: ngenes " + std::to_string(ngenes) + " is not a number of genes from 0 to the index's " + std::to_string(nseq) + " sequences"; return -1; }
    if (!seg_gene || !seg_off || !gene_len) { g_err = "mc_set_gene_fold: " + std::to_string(ngenes) + " genes and a NULL map"; return -1; }
    std::vector<McFoldSeg> seg((size_t)nseq); std::vector<uint32_t> goff((size_t)ngenes + 1, 0u);
    uint64_t at = 0;
    for (int32_t g = 0; g < ngenes; g++) {
        if (gene_len[g] < 1 || gene_len[g] > MC_FOLD_MAX_GENE) { g_err = "mc_set_gene_fold: gene_len[" + std::to_string(g) + "] = " + std::to_string(gene_len[g]) + " lies outside 1 .. " + std::to_string(MC_FOLD_MAX_GENE); return -1; }
        goff[(size_t)g] = (uint32_t)at; at += (uint64_t)gene_len[g];
        if (at + (uint64_t)g + 1 > 0xFFFFFFFFull) { g_err = "mc_set_gene_fold: the coverage offsets pass 2^32 at gene " + std::to_string(g) + " (" + std::to_string(at) + " residues)"; return -1; }
    }
    goff[(size_t)ngenes] = (uint32_t)at;
    // the map ascends gene by gene, every gene has its segments; a gene's offsets are j * S with one step S for all, every segment but a
    // gene's last has one length L > S, and the last is the first that reaches gene_len
    int32_t L = 0, S = 0;                                            // (what the first gene of more than one segment says; 0, 0: no gene is split)
    for (int32_t s = 1; s < nseq && S == 0; s++)
        if (seg_gene[s] == seg_gene[s - 1]) { S = seg_off[s]; L = (int32_t)(h->H.off[(size_t)s] - h->H.off[(size_t)s - 1]); }
    for (int32_t s = 0, g = -1, j = 0; s < nseq; s++, j++) {
        const int32_t len = (int32_t)(h->H.off[(size_t)s + 1] - h->H.off[(size_t)s]);
        if (seg_gene[s] != g) {
            if (seg_gene[s] != g + 1) { g_err = "mc_set_gene_fold: seg_gene[" + std::to_string(s) + "] = " + std::to_string(seg_gene[s]) + " behind gene " + std::to_string(g) + ": the map does not ascend gene by gene"; return -1; }
            g++; j = 0;
            if (g >= ngenes) { g_err = "mc_set_gene_fold: seg_gene[" + std::to_string(s) + "] = " + std::to_string(seg_gene[s]) + " lies outside 0 .. " + std::to_string(ngenes - 1); return -1; }
        }
        const bool last = s + 1 == nseq || seg_gene[s + 1] != g;
        if (seg_off[s] < 0 || (j == 0 && seg_off[s] != 0) || (j > 0 && (S <= 0 || seg_off[s] != j * S))) {
            g_err = "mc_set_gene_fold: seg_off[" + std::to_string(s) + "] = " + std::to_string(seg_off[s]) + " is not " + std::to_string(j) + " steps of " + std::to_string(S) + " into gene " + std::to_string(g); return -1;
        }
        const int64_t end = (int64_t)seg_off[s] + len;
        if (last ? end != gene_len[g] : (end >= gene_len[g] || len != L || L <= S)) {
            g_err = "mc_set_gene_fold: segment " + std::to_string(s) + " of " + std::to_string(len) + " residues at seg_off " + std::to_string(seg_off[s]) + " does not fit gene " + std::to_string(g) + " of gene_len " +
                    std::to_string(gene_len[g]) + (last ? ": the last segment ends at " + std::to_string(end) : ": an inner segment has " + std::to_string(L) + " residues, more than the step " + std::to_string(S) + ", and ends before the gene does");
            return -1;
        }
        seg[(size_t)s].gene = g; seg[(size_t)s].off = seg_off[s]; seg[(size_t)s].lo = j > 0 ? 0 : -1; seg[(size_t)s].hi = last ? -1 : len - 1;
        if (last && s + 1 == nseq && g != ngenes - 1) { g_err = "mc_set_gene_fold: the map ends at gene " + std::to_string(g) + " of " + std::to_string(ngenes); return -1; }
    }
    if (h->ab.on && !h->ab.fold_keeps_sizes(ngenes, (size_t)at)) return refuse_sizes(ngenes, (size_t)at);
    return h->ab.set_fold(ngenes, seg.data(), goff.data());
}

// ngenes: the genes of the fold, 0: off; edge_rows: the rows that touched an interior segment edge since the last zeroing (mc_fold.h: the
// witness that the overlap was wide enough); ms: k_fold's time over the completed ranges since then.  Any of the three may be NULL
extern "C" int mc_gene_fold_stats(mc_handle *h, int32_t *ngenes, int64_t *edge_rows, float *ms)
{
    if (!h) { g_err = "null handle"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (ngenes) *ngenes = h->ab.fold ? h->ab.nseq : 0;
    if (ms) *ms = h->ab.fold_ms;
    return h->ab.read_fold(edge_rows);
}

// the sequences and residues every abundance table is sized by: the index's, or the genes' under a fold
extern "C" int32_t mc_abundance_count(const mc_handle *h) { return h ? h->ab.nseq : -1; }
extern "C" int64_t mc_abundance_residues(const mc_handle *h) { return h ? (int64_t)h->ab.nres : -1; }

// rows[k], assigned[k] of class k = 0 .. n - 2 and, at n - 1, the rows below the lowest class; n: the classes of mc_set_run_classes + 1
extern "C" int mc_abundance_classes_read(mc_handle *h, int64_t *rows, int64_t *assigned, int32_t n)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (!h->ab.classes) { g_err = "mc_abundance_classes_read: the counts do not ride on class runs (mc_set_abundance_classes)"; return -1; }
    if (!h->cls_set || n != h->cls.K + 1) { g_err = "mc_abundance_classes_read: the arrays hold " + std::to_string(n) + " values, the run has " + std::to_string(h->cls_set ? h->cls.K : 0) + " classes and the rows below them (mc_set_run_classes)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    return h->ab.read_classes(rows, assigned, n);
}
extern "C" float mc_abundance_classes_ms(const mc_handle *h) { return h ? h->ab.cls_ms : 0.0f; }

// k_geneboot_collect's time over the completed ranges plus the reads' kernels, since the last zeroing
extern "C" float mc_gene_bootstrap_ms(const mc_handle *h) { return h ? h->ab.gboot.collect_ms + h->ab.gboot.read_ms : 0.0f; }
// k_tieboot_collect's time over the completed ranges plus the tie reads' kernels, since the last zeroing; the two parts (either may be NULL)
extern "C" float mc_tie_bootstrap_ms(const mc_handle *h) { return h ? h->ab.tboot.collect_ms + h->ab.tboot.read_ms : 0.0f; }
extern "C" void mc_tie_bootstrap_kernels_ms(const mc_handle *h, float *collect_ms, float *read_ms)
{
    if (collect_ms) *collect_ms = h ? h->ab.tboot.collect_ms : 0.0f;
    if (read_ms) *read_ms = h ? h->ab.tboot.read_ms : 0.0f;
}
// k_covboot_collect's time over the completed ranges plus the coverage reads' kernels, since the last zeroing; the two parts (either may be NULL)
extern "C" float mc_coverage_bootstrap_ms(const mc_handle *h) { return h ? h->ab.cboot.collect_ms + h->ab.cboot.read_ms : 0.0f; }
extern "C" void mc_coverage_bootstrap_kernels_ms(const mc_handle *h, float *collect_ms, float *read_ms)
{
    if (collect_ms) *collect_ms = h ? h->ab.cboot.collect_ms : 0.0f;
    if (read_ms) *read_ms = h ? h->ab.cboot.read_ms : 0.0f;
}
// the group reads' kernels since the last zeroing: k_groupboot_values and k_groupboot_summary, and the kernels of a mat a group read had to make
extern "C" float mc_group_bootstrap_ms(const mc_handle *h) { return h ? h->ab.grp_ms : 0.0f; }
// the two kernels' shares of it (either may be NULL)
extern "C" void mc_group_bootstrap_kernels_ms(const mc_handle *h, float *values_ms, float *summary_ms)
{
    if (values_ms) *values_ms = h ? h->ab.grp_values_ms : 0.0f;
    if (summary_ms) *summary_ms = h ? h->ab.grp_summary_ms : 0.0f;
}
extern "C" float mc_abundance_ms(const mc_handle *h) { return h ? h->ab.ms : 0.0f; }
extern "C" float mc_coverage_ms(const mc_handle *h) { return h ? h->ab.cov_ms : 0.0f; }
extern "C" float mc_ties_ms(const mc_handle *h) { return h ? h->ab.ties_ms : 0.0f; }

extern "C" int64_t mc_result_rows(mc_handle *h, const mc_row **rows) { if (!h) return -1; rows_wait(h); *rows = h->res_rows; return h->n_res_rows; }
extern "C" int64_t mc_result_best_hits(mc_handle *h, const mc_best_hit **hits) { if (!h) return -1; best_materialize(h); *hits = h->best.data(); return (int64_t)h->best.size(); }
extern "C" int mc_result_stats(mc_handle *h, mc_stats *out) { if (!h) return -1; *out = h->stats; return 0; }

static int write_m8(mc_handle *h, const char *path, int append, const char *const *query_names, int64_t n_names, int64_t first_read_id)
{
    if (!h) { g_err = "null handle"; return -1; }
    rows_wait(h);
    FILE *f = fopen(path, append ? "a" : "w");
    if (!f) { g_err = std::string("cannot open ") + path; return -1; }
    setvbuf(f, nullptr, _IOFBF, 1 << 22);
    for (int64_t i = 0; i < h->n_res_rows; i++) {
        const mc_row &r = h->res_rows[i];
        if (query_names) {
            const int64_t k = (int64_t)r.query - first_read_id;
            if (k < 0 || k >= n_names) { fclose(f); g_err = "a row's query id lies outside the names given"; return -1; }
            fprintf(f, "%s", query_names[k]);
        } else fprintf(f, "%d", r.query);
        fprintf(f, "\t%s\t%g\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%g\t%g\n", h->H.names[r.subject].c_str(), r.ident, r.alnlen, r.mismatch, r.gapopen, r.qstart, r.qend,
                r.sstart, r.send, r.loge, r.bits);
    }
    fclose(f);
    return 0;
}
extern "C" int mc_write_m8(mc_handle *h, const char *path, int append) { return write_m8(h, path, append, nullptr, 0, 0); }
extern "C" int mc_write_m8_named(mc_handle *h, const char *path, int append, const char *const *query_names, int64_t n_names, int64_t first_read_id)
{
    if (!query_names) { g_err = "null names"; return -1; }
    return write_m8(h, path, append, query_names, n_names, first_read_id);
}

// ------------------------------------------------------------------------------------------------
// training and mock communities: device-resident sources of reads, simulated libraries, the fused library passes
// ------------------------------------------------------------------------------------------------
// What a genome and a community share: the bases and contig offsets in HBM, the library kind with its error thresholds, and the
// table of valid starts (made by either for the span at hand).  `noun` names the source in error messages.
struct McSimSource {
    const char *noun;
    int device = 0, ncontig = 0;
    std::vector<int64_t> off;                                       // contig offsets (host)
    McDevBuf mem;                                                   // owns every device buffer of the source
    uint8_t *d_bases = nullptr; int64_t *d_off = nullptr, *d_vstart = nullptr;
    int span = 0;                                                   // the span (read length or insert) the tables of valid starts were made for
    mc_library lib = {0, 0, MC_ERR_NONE, 0.0};                      // mc_*_set_library's kind; d_thr: its error thresholds (mc_simlib.h)
    uint64_t *d_thr = nullptr;
    explicit McSimSource(const char *n) : noun(n) {}
    std::string fn(const char *what) const { return "mc_" + std::string(noun) + "_" + what; }
};
struct mc_genome : McSimSource {
    int read_lengths = MC_SIM_LEN_FIXED;                            // mc_genome_set_read_lengths
    mc_genome() : McSimSource("genome") {}
    McGenomePlacer placer() const { return {d_off, d_vstart, ncontig}; }
};
struct mc_community : McSimSource {
    int M = 0;
    std::vector<int64_t> copies;                                    // copies per member (host)
    std::vector<int32_t> mfirst;                                    // member m holds contigs mfirst[m] .. mfirst[m + 1] - 1
    int64_t *d_total = nullptr; uint64_t *d_cum = nullptr; int32_t *d_mfirst = nullptr;
    unsigned long long *d_counts = nullptr;                         // reads per member of the pass under way
    std::vector<int64_t> member_reads;                              // ... of the last simulate / library call
    mc_community() : McSimSource("community") {}
    McCommPlacer placer() const { return {d_cum, d_total, d_mfirst, d_vstart, d_off, M, M <= MC_COMM_LDS_M ? 1 : 0, d_counts, nullptr, nullptr, nullptr}; }
};
static_assert(MC_ERR_NONE == MC_SIM_ERR_NONE && MC_ERR_UNIFORM == MC_SIM_ERR_UNIFORM && MC_ERR_ILLUMINA == MC_SIM_ERR_ILLUMINA, "one numbering of the error models");
static bool default_library(const mc_library &l) { return !l.paired_end && l.error_model == MC_ERR_NONE; }

// the checks of mc_*_open that need no device ...
static int source_args(const McSimSource &s, const uint8_t *bases, const int64_t *contig_off, int32_t ncontig)
{
    if (!bases || !contig_off || ncontig < 1) { g_err = s.fn("open") + ": bad argument"; return -1; }
    if (contig_off[0] != 0) { g_err = s.fn("open") + ": contig_off[0] must be 0"; return -1; }
    for (int i = 0; i < ncontig; i++) if (contig_off[i + 1] < contig_off[i]) { g_err = s.fn("open") + ": contig offsets must not decrease"; return -1; }
    return 0;
}
// ... and the device's: the bases (64 bytes of slack behind them) and the offsets to it, room for the valid starts and the thresholds
static int source_open(McSimSource &s, const uint8_t *bases, const int64_t *contig_off, int32_t ncontig, int32_t device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_err = "no HIP device visible"; return -1; }
    if (device < 0 || device >= ndev) { g_err = s.fn("open") + ": no such device"; return -1; }
    if (hipSetDevice(device) != hipSuccess) { g_err = "hipSetDevice failed"; return -1; }
    s.device = device; s.ncontig = ncontig; s.off.assign(contig_off, contig_off + ncontig + 1);
    const size_t nb = (size_t)contig_off[ncontig];
    if (s.mem.get(&s.d_bases, nb + 64) || s.mem.get(&s.d_off, (size_t)ncontig + 1) || s.mem.get(&s.d_vstart, (size_t)ncontig + 1) || s.mem.get(&s.d_thr, MC_SIM_NTHR) ||
        hipMemcpy(s.d_bases, bases, nb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s.d_off, contig_off, sizeof(int64_t) * (ncontig + 1), hipMemcpyHostToDevice) != hipSuccess) {
        g_err = s.fn("open") + ": out of device memory";
        return -1;
    }
    return 0;
}
template <class S> static void source_close(S *s) { if (s) { (void)hipSetDevice(s->device); delete s; } }

extern "C" mc_genome *mc_genome_open(const uint8_t *bases, const int64_t *contig_off, int32_t ncontig, int32_t device)
{
    mc_genome *g = new mc_genome();
    if (source_args(*g, bases, contig_off, ncontig) || source_open(*g, bases, contig_off, ncontig, device)) { mc_genome_close(g); return nullptr; }
    return g;
}
extern "C" void mc_genome_close(mc_genome *g) { source_close(g); }

static int set_library(McSimSource *s, const char *fn, const mc_library *lib)
{
    if (!s) { g_err = std::string(fn) + ": bad argument"; return -1; }
    const mc_library l = lib ? *lib : mc_library{0, 0, MC_ERR_NONE, 0.0};
    if (l.error_model != MC_ERR_NONE && l.error_model != MC_ERR_UNIFORM && l.error_model != MC_ERR_ILLUMINA) { g_err = "unknown error model " + std::to_string(l.error_model); return -1; }
    if (!(l.error_rate >= 0.0 && l.error_rate <= 1.0)) { g_err = "error rate " + std::to_string(l.error_rate) + " outside [0, 1]"; return -1; }
    int64_t longest = 0;
    for (int c = 0; c < s->ncontig; c++) longest = std::max(longest, s->off[(size_t)c + 1] - s->off[(size_t)c]);
    if (l.paired_end && l.insert < 1) { g_err = "a paired-end library needs a positive insert"; return -1; }
    if (l.paired_end && l.insert > longest) { g_err = "the " + std::string(s->noun) + " has no contig of at least the insert (" + std::to_string(l.insert) + " bp)"; return -1; }
    uint64_t thr[MC_SIM_NTHR];
    mc_sim_thresholds(l.error_model, l.error_rate, thr);
    HIPCK(hipSetDevice(s->device));
    HIPCK(hipMemcpy(s->d_thr, thr, sizeof thr, hipMemcpyHostToDevice));
    s->lib = l;
    return 0;
}
extern "C" int mc_genome_set_library(mc_genome *g, const mc_library *lib) { return set_library(g, "mc_genome_set_library", lib); }
extern "C" int mc_community_set_library(mc_community *c, const mc_library *lib) { return set_library(c, "mc_community_set_library", lib); }

// The span of a fragment for reads of L bases: the insert of a paired-end library, else L.  Returns it when the source's tables have to
// be made for it, 0 when they stand, -1 for an insert shorter than the read.  no_contig(): what a source without a start of that span says.
static int span_to_make(const McSimSource &s, int L)
{
    if (s.lib.paired_end && s.lib.insert < L) { g_err = "the insert (" + std::to_string(s.lib.insert) + ") is shorter than the read length (" + std::to_string(L) + ")"; return -1; }
    const int span = s.lib.paired_end ? s.lib.insert : L;
    return s.span == span ? 0 : span;
}
static int no_contig(const McSimSource &s, int span)
{
    g_err = "the " + std::string(s.noun) + " has no contig of at least the " + std::string(s.lib.paired_end ? "insert" : "read length") + " (" + std::to_string(span) + " bp)";
    return -1;
}

// the valid starts of every contig for reads of L bases (prefix sums); refuses a genome without a contig of the span
static int source_for_len(mc_genome *g, int L)
{
    const int span = span_to_make(*g, L);
    if (span <= 0) return span;
    std::vector<int64_t> vs((size_t)g->ncontig + 1, 0);
    for (int c = 0; c < g->ncontig; c++) vs[(size_t)c + 1] = vs[(size_t)c] + std::max<int64_t>(0, g->off[(size_t)c + 1] - g->off[(size_t)c] - span + 1);
    if (vs.back() == 0) return no_contig(*g, span);
    HIPCK(hipMemcpy(g->d_vstart, vs.data(), sizeof(int64_t) * vs.size(), hipMemcpyHostToDevice));
    g->span = span;
    return 0;
}
// the member table for reads of L bases; refuses a community none of whose members has a contig of the span, and a universe of 2^62 or more
static int source_for_len(mc_community *c, int L)
{
    const int span = span_to_make(*c, L);
    if (span <= 0) return span;
    std::vector<int64_t> vs((size_t)c->ncontig), total((size_t)c->M);
    std::vector<uint64_t> cum((size_t)c->M + 1);
    const int bad = mc_sim_member_table(c->off.data(), c->mfirst.data(), c->copies.data(), c->M, span, vs.data(), total.data(), cum.data());
    if (bad == 1) return no_contig(*c, span);
    if (bad) { g_err = "the community's universe (the sum of copies x valid starts) does not stay below 2^62"; return -1; }
    HIPCK(hipMemcpy(c->d_vstart, vs.data(), sizeof(int64_t) * vs.size(), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_total, total.data(), sizeof(int64_t) * total.size(), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->d_cum, cum.data(), sizeof(uint64_t) * cum.size(), hipMemcpyHostToDevice));
    c->span = span;
    return 0;
}

// what the simulate entry points do first: the read length's range, the source's device, its tables for that length
template <class S> static int simulate_begin(S *s, int read_len)
{
    if (read_len < 18 || read_len > 3 * MC_MAXAA) { g_err = "read_len out of range (18..510)"; return -1; }
    HIPCK(hipSetDevice(s->device));
    return source_for_len(s, read_len);
}

static uint64_t sim_key(uint64_t seed, uint64_t library_id) { return mc_mix64(seed ^ mc_mix64(library_id)); }
static McSimKind sim_kind(const McSimSource &s, int L) { return McSimKind{L, s.lib.paired_end ? 1 : 0, s.lib.paired_end ? s.lib.insert : L, s.lib.error_model != MC_ERR_NONE ? 1 : 0}; }

// reads [first, first + n) of the source's library into dst (device), on st
template <class S> static int launch_simulate(const S *s, int L, uint64_t key, int64_t first, int64_t n, uint8_t *dst, hipStream_t st)
{
    if (n <= 0) return 0;
    const auto place = s->placer();
    if (default_library(s->lib)) {
        k_sim_copy<<<dim3((unsigned)((n + 255) / 256)), dim3(256), place.lds_bytes(), st>>>(s->d_bases, place, L, key, first, n, dst);
    } else {
        const size_t lds = (size_t)64 * L + sizeof(uint64_t) * MC_SIM_NTHR + place.lds_bytes();
        k_sim_walk<<<dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st>>>(s->d_bases, place, sim_kind(*s, L), s->d_thr, key, mc_mix64(key ^ MC_SIM_EKEY), first, n, dst);
    }
    HIPCK(hipGetLastError());
    return 0;
}

// reads [first, first + n) to the host, in ranges of the streaming batch size, as the fused passes make them
template <class S> static int simulate_to_host(const S *s, int L, int64_t first, int64_t n, uint64_t key, uint8_t *dst_host, const char *fn)
{
    const int64_t B = std::min<int64_t>(n, stream_batch());
    McDevBuf buf;
    uint8_t *d = nullptr;
    if (buf.get(&d, (size_t)(B * L))) return -1;
    for (int64_t at = 0; at < n; at += B) {
        const int64_t cnt = std::min(B, n - at);
        if (launch_simulate(s, L, key, first + at, cnt, d, nullptr)) return -1;
        if (hipMemcpy(dst_host + at * L, d, (size_t)(cnt * L), hipMemcpyDeviceToHost) != hipSuccess) { g_err = std::string(fn) + ": copy failed"; return -1; }
    }
    return 0;
}

static_assert(MC_READLEN_FIXED == MC_SIM_LEN_FIXED && MC_READLEN_REFERENCE == MC_SIM_LEN_REFERENCE, "one numbering of the read-length modes");
extern "C" int mc_genome_set_read_lengths(mc_genome *g, int32_t mode)
{
    if (!g) { g_err = "mc_genome_set_read_lengths: bad argument"; return -1; }
    if (mode != MC_READLEN_FIXED && mode != MC_READLEN_REFERENCE) { g_err = "unknown read-length mode " + std::to_string(mode); return -1; }
    g->read_lengths = mode;
    return 0;
}

// Reads [first, first + n) of the reference read-length mode into d_dst (n x min(2L, 510) bytes + 64 of room), their offsets (from
// 0) into d_roff (n + 1), in two passes: lengths (d_lens, n), checked on the host (a read over 510 bases is refused, named), scanned on
// the device, then the reads.  *total: their bases.
static int simulate_var(const mc_genome *g, int L, uint64_t key, int64_t first, int64_t n, uint32_t *d_lens, int64_t *d_roff, uint8_t *d_dst, hipStream_t st,
                        int64_t *total)
{
    *total = 0;
    if (n <= 0) return 0;
    const McSimKind kind = sim_kind(*g, L);
    const McGenomePlacer place = g->placer();
    const uint64_t ekey = mc_mix64(key ^ MC_SIM_EKEY);
    const dim3 grid((unsigned)((n + 63) / 64));
    k_simulate_var<<<grid, dim3(64), 0, st>>>(g->d_bases, place, kind, g->d_thr, key, ekey, first, n, d_lens, nullptr, nullptr);
    HIPCK(hipGetLastError());
    std::vector<uint32_t> lens((size_t)n);
    HIPCK(hipMemcpyAsync(lens.data(), d_lens, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    int64_t sum = 0;
    for (int64_t k = 0; k < n; k++) {
        if (lens[(size_t)k] > 3 * MC_MAXAA) {
            g_err = "read " + std::to_string(first + k) + " of the library is " + std::to_string(lens[(size_t)k]) + " bases long (read length " + std::to_string(L) +
                    " plus its insertions): longer than 510";
            return -1;
        }
        sum += lens[(size_t)k];
    }
    k_sim_scan<<<dim3(1), dim3(1024), 0, st>>>(d_lens, n, d_roff);
    HIPCK(hipGetLastError());
    k_simulate_var<<<grid, dim3(64), 0, st>>>(g->d_bases, place, kind, g->d_thr, key, ekey, first, n, nullptr, d_roff, d_dst);
    HIPCK(hipGetLastError());
    *total = sum;
    return 0;
}

extern "C" int64_t mc_simulate_varlen(mc_genome *g, int32_t read_len, int64_t first, int64_t n, uint64_t seed, uint64_t library_id, uint8_t *dst_host,
                                      int64_t dst_cap, int64_t *offsets)
{
    if (!g || first < 0 || n < 0 || !offsets) { g_err = "mc_simulate_varlen: bad argument"; return -1; }
    if (simulate_begin(g, read_len)) return -1;
    offsets[0] = 0;
    if (n == 0) return 0;
    const int64_t B = std::min<int64_t>(n, stream_batch()), W = std::min(2 * read_len, 3 * MC_MAXAA);
    McDevBuf buf;
    uint8_t *d = nullptr; uint32_t *d_lens = nullptr; int64_t *d_roff = nullptr;
    if (buf.get(&d, (size_t)(B * W + 64)) || buf.get(&d_lens, (size_t)B) || buf.get(&d_roff, (size_t)B + 1)) return -1;
    const uint64_t key = sim_key(seed, library_id);
    int64_t at_byte = 0;
    for (int64_t at = 0; at < n; at += B) {                          // ranges of the streaming batch size, as mc_train_library makes them
        const int64_t cnt = std::min(B, n - at);
        int64_t total = 0;
        if (simulate_var(g, read_len, key, first + at, cnt, d_lens, d_roff, d, nullptr, &total)) return -1;
        std::vector<int64_t> ro((size_t)cnt + 1);
        HIPCK(hipMemcpy(ro.data(), d_roff, ro.size() * 8, hipMemcpyDeviceToHost));
        for (int64_t k = 1; k <= cnt; k++) offsets[at + k] = at_byte + ro[(size_t)k];
        if (dst_host && at_byte + total <= dst_cap) HIPCK(hipMemcpy(dst_host + at_byte, d, (size_t)total, hipMemcpyDeviceToHost));
        at_byte += total;
    }
    return at_byte;
}

extern "C" int mc_simulate(mc_genome *g, int32_t read_len, int64_t first, int64_t n, uint64_t seed, uint64_t library_id, uint8_t *dst_host)
{
    if (!g || first < 0 || n < 0 || (n > 0 && !dst_host)) { g_err = "mc_simulate: bad argument"; return -1; }
    if (simulate_begin(g, read_len)) return -1;
    if (n == 0) return 0;
    return simulate_to_host(g, read_len, first, n, sim_key(seed, library_id), dst_host, "mc_simulate");
}

// one range of the resident reads through the pipeline with its rows left on the device, then the grid over those rows into the
// bins; a range that overflows a pool is run in halves (the grid's bins do not care how the reads were cut)
static int train_range(mc_handle *h, int64_t first, int64_t count, int64_t first_read_id, const McGridPars &G, unsigned long long *d_bins, size_t nbins,
                       hipEvent_t e0, hipEvent_t e1, mc_stats &tot)
{
    if (count <= 0) return 0;
    McCtx &c = h->ctx;
    int rc = range_begin(h, c, first, count, first_read_id, false);
    if (rc == 0) rc = range_end(h, c);
    if (rc == -2 && count > 1) {
        tot.range_splits++;
        const int64_t a = count / 2;
        if ((rc = train_range(h, first, a, first_read_id, G, d_bins, nbins, e0, e1, tot)) != 0) return rc;
        return train_range(h, first + a, count - a, first_read_id + a, G, d_bins, nbins, e0, e1, tot);
    }
    if (rc) return rc;
    stats_add(tot, h->stats);
    const int64_t nrows = (int64_t)c.nrows;
    HIPCK(hipEventRecord(e0, c.stream));
    if (nrows) k_grid_classify<<<dim3((unsigned)((nrows + 127) / 128)), dim3(128), 0, c.stream>>>(G, dev_index(h), h->d_fam, c.d_rows, nrows, d_bins, d_bins + nbins, (double *)(d_bins + 2 * nbins));
    HIPCK(hipEventRecord(e1, c.stream));
    HIPCK(hipEventSynchronize(e1));
    h->train_ms[2] += ev_ms(e0, e1);
    return 0;
}

// one range of a library into the resident read buffer, between the events ev[0] and ev[1] on the handle's stream
template <class S> static int simulate_resident(mc_handle *h, const S *s, uint64_t key, int64_t at, int64_t cnt, const McEvents &ev)
{
    hipStream_t st = h->ctx.stream;
    reads_change(h);
    if (hipEventRecord(ev[0], st) != hipSuccess || launch_simulate(s, h->read_len, key, at, cnt, h->d_reads, st) || hipEventRecord(ev[1], st) != hipSuccess) return -1;
    h->reads_dev = h->d_reads; h->nreads = cnt;
    return 0;
}

extern "C" int mc_train_library(mc_handle *h, mc_genome *g, int64_t nreads, uint64_t seed, uint64_t library_id, const double *aln_covs, int32_t n_cov,
                                const int32_t *max_pids, int32_t n_pid, const double *min_scores, int32_t n_score, int64_t *count_hits, int64_t *count_aln, double *count_cov)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    if (!g || nreads < 0 || !count_hits || !count_aln || !count_cov) { g_err = "mc_train_library: bad argument"; return -1; }
    if (g->lib.paired_end && (nreads & 1)) { g_err = "a paired-end library has an even number of reads (" + std::to_string(nreads) + " given)"; return -1; }
    if (g->device != h->device) { g_err = "mc_train_library: the genome lies on another device than the handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_train_library: ranges begun with mc_range_begin() are still in flight"; return -1; }
    ahead_drop(h);                                                  // (the resident reads are about to be simulated over)
    if (h->ab.active()) { g_err = "mc_train_library: refused while abundance counting is on (mc_set_abundance)"; return -1; }
    McGridPars G; std::vector<int> order;
    if (grid_pars(h, aln_covs, n_cov, max_pids, n_pid, min_scores, n_score, G, order)) return -1;
    HIPCK(hipSetDevice(h->device));
    const int L = h->read_len;
    if (source_for_len(g, L)) return -1;
    const int nfam = h->nfam;
    const size_t nbins = (size_t)n_cov * n_pid * (MC_GRID_MAXS + 1) * nfam;
    const size_t nout = (size_t)n_cov * n_pid * n_score * nfam;
    memset(count_hits, 0, nout * 8); memset(count_aln, 0, nout * 8); memset(count_cov, 0, nout * 8);
    h->train_ms[0] = h->train_ms[1] = h->train_ms[2] = 0.f;
    mc_stats tot; memset(&tot, 0, sizeof tot);
    if (nreads == 0) { h->stats = tot; return 0; }
    const int64_t B = std::min<int64_t>(nreads, stream_batch());
    const bool ref = g->read_lengths == MC_SIM_LEN_REFERENCE;
    h->train_bases = 0;
    // the resident read buffer (mc_upload's) holds one range at a time: the simulator writes it, the search reads it
    if (!ref && (reads_reserve(h, B) || ensure_capacity(h, h->ctx, B))) return -1;
    // the reference read-length mode: reads of L + ins - del bases (two passes), bucketed by length, each bucket searched at its length
    // and grid-classified into the same bins (a read lies in one bucket: its best survivor is the one of the whole library)
    McDevBuf vb;
    uint8_t *d_sim = nullptr; uint32_t *d_lens = nullptr; int64_t *d_roff = nullptr;
    if (ref && (vb.get(&d_sim, (size_t)(B * std::min(2 * L, 3 * MC_MAXAA) + 64)) || vb.get(&d_lens, (size_t)B) || vb.get(&d_roff, (size_t)B + 1))) return -1;
    unsigned long long *d_bins = nullptr;
    if (vb.get(&d_bins, nbins * 3)) { g_err = "out of device memory"; return -1; }
    McEvents ev;
    if (ev.make(4)) return -1;
    hipStream_t st = h->ctx.stream;
    McModeGuard mode(h, false, true);                                // (the grid needs every row of a read)
    int rc = hipMemsetAsync(d_bins, 0, nbins * 24, st) == hipSuccess ? 0 : -1;
    if (rc) g_err = "hipMemsetAsync failed";
    const uint64_t key = sim_key(seed, library_id);
    for (int64_t at = 0; at < nreads && rc == 0 && !ref; at += B) {
        const int64_t cnt = std::min(B, nreads - at);
        if (simulate_resident(h, g, key, at, cnt, ev)) { rc = -1; break; }
        rc = train_range(h, 0, cnt, at, G, d_bins, nbins, ev[2], ev[3], tot);
        if (rc) break;
        h->train_ms[0] += ev_ms(ev[0], ev[1]);
        h->train_bases += cnt * L;
    }
    if (ref) {
        McLenBorrow len(h);
        for (int64_t at = 0; at < nreads && rc == 0; at += B) {
            const int64_t cnt = std::min(B, nreads - at);
            int64_t bases = 0;
            if (hipEventRecord(ev[0], st) != hipSuccess || simulate_var(g, L, key, at, cnt, d_lens, d_roff, d_sim, st, &bases)) { rc = -1; break; }
            McDevBuf bb;
            uint8_t *d_sorted = nullptr; uint32_t *d_perm = nullptr;
            std::vector<uint32_t> start; std::vector<int64_t> boff;
            if (vl_bucket(bb, st, d_sim, d_roff, cnt, bases, &d_sorted, &d_perm, start, boff) || hipEventRecord(ev[1], st) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess) { rc = -1; break; }
            h->train_ms[0] += ev_ms(ev[0], ev[1]);
            h->train_bases += bases;
            const McPieces P = mc_cut_pieces(vl_bins(start), B);
            tot.reads += P.nshort;
            if (!P.v.empty() && (rc = len.pools(P.Lmax, P.nmax)) != 0) break;
            // a plain loop, not run_pieces: the grid reads a piece's rows where they lie, before the next front may overwrite them
            for (const McPiece &q : P.v) {
                if ((rc = len.use(q.L)) != 0) break;
                reads_change(h);
                h->reads_dev = d_sorted + boff[(size_t)q.L]; h->nreads = q.bin_n;
                if ((rc = train_range(h, q.first, q.n, at + q.bin_first + q.first, G, d_bins, nbins, ev[2], ev[3], tot)) != 0) break;
            }
            (void)hipStreamSynchronize(st);                          // (the bucket buffers are freed at the end of the range)
        }
        rc = len.close(rc);                                          // the run's own length and tables back
        reads_change(h);
        h->reads_dev = nullptr; h->nreads = 0;                       // (the buckets the handle read from are gone)
    }
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr;
    std::vector<unsigned long long> bins(nbins * 3);
    if (rc == 0 && (hipMemcpyAsync(bins.data(), d_bins, nbins * 24, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) { g_err = "mc_train_library: copy of the bins failed"; rc = -1; }
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    grid_counts(bins, nbins, n_cov * n_pid, n_score, nfam, order, count_hits, count_aln, count_cov);
    h->stats = tot; h->train_ms[1] = tot.ms_total;
    return 0;
}

extern "C" int64_t mc_train_library_bases(const mc_handle *h) { if (!h) { g_err = "null handle"; return -1; } return h->train_bases; }

extern "C" int mc_train_times(const mc_handle *h, float *ms)
{
    if (!h || !ms) { g_err = "null argument"; return -1; }
    for (int k = 0; k < 3; k++) ms[k] = h->train_ms[k];
    return 0;
}

// ------------------------------------------------------------------------------------------------
// mock communities: M genomes with copies each, resident in HBM; their libraries (k_community.h's placer), the fused library pass
// ------------------------------------------------------------------------------------------------
static int community_open(mc_community *c, const uint8_t *bases, const int64_t *contig_off, int32_t ncontig, const int32_t *member_first_contig, const int64_t *copies,
                          int32_t M, int32_t device)
{
    if (!bases || !contig_off || ncontig < 1 || !member_first_contig || !copies) { g_err = "mc_community_open: bad argument"; return -1; }
    if (M < 1 || M > MC_SIM_MAX_MEMBERS) { g_err = "mc_community_open: " + std::to_string(M) + " members (1 .. " + std::to_string(MC_SIM_MAX_MEMBERS) + ")"; return -1; }
    if (source_args(*c, bases, contig_off, ncontig)) return -1;
    if (member_first_contig[0] != 0 || member_first_contig[M] != ncontig) { g_err = "mc_community_open: member_first_contig must run from 0 to ncontig"; return -1; }
    for (int m = 0; m < M; m++) {
        if (member_first_contig[m + 1] <= member_first_contig[m]) { g_err = "mc_community_open: member " + std::to_string(m) + " has no contig"; return -1; }
        if (copies[m] < 1 || copies[m] > MC_SIM_MAX_COPIES) { g_err = "mc_community_open: member " + std::to_string(m) + " has " + std::to_string(copies[m]) + " copies (1 .. " + std::to_string(MC_SIM_MAX_COPIES) + ")"; return -1; }
    }
    if (source_open(*c, bases, contig_off, ncontig, device)) return -1;
    c->M = M; c->copies.assign(copies, copies + M); c->mfirst.assign(member_first_contig, member_first_contig + M + 1);
    c->member_reads.assign((size_t)M, 0);
    if (c->mem.get(&c->d_total, (size_t)M) || c->mem.get(&c->d_cum, (size_t)M + 1) || c->mem.get(&c->d_mfirst, (size_t)M + 1) || c->mem.get(&c->d_counts, (size_t)M) ||
        hipMemcpy(c->d_mfirst, member_first_contig, sizeof(int32_t) * (M + 1), hipMemcpyHostToDevice) != hipSuccess) {
        g_err = "mc_community_open: out of device memory";
        return -1;
    }
    return 0;
}
extern "C" mc_community *mc_community_open(const uint8_t *bases, const int64_t *contig_off, int32_t ncontig, const int32_t *member_first_contig, const int64_t *copies,
                                           int32_t M, int32_t device)
{
    mc_community *c = new mc_community();
    if (community_open(c, bases, contig_off, ncontig, member_first_contig, copies, M, device)) { mc_community_close(c); return nullptr; }
    return c;
}
extern "C" void mc_community_close(mc_community *c) { source_close(c); }

// the device's counts cleared before a pass (on st), and to the host when it has ended (everything on `st` waited for)
static int community_counts_reset(mc_community *c, hipStream_t st) { HIPCK(hipMemsetAsync(c->d_counts, 0, sizeof(unsigned long long) * c->M, st)); return 0; }
static int community_counts(mc_community *c, hipStream_t st)
{
    std::vector<unsigned long long> v((size_t)c->M);
    HIPCK(hipMemcpyAsync(v.data(), c->d_counts, sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int m = 0; m < c->M; m++) c->member_reads[(size_t)m] = (int64_t)v[(size_t)m];
    return 0;
}

extern "C" int mc_community_simulate(mc_community *c, int32_t read_len, int64_t first, int64_t n, uint64_t seed, uint64_t library_id, uint8_t *dst_host)
{
    if (!c || first < 0 || n < 0 || (n > 0 && !dst_host)) { g_err = "mc_community_simulate: bad argument"; return -1; }
    if (simulate_begin(c, read_len)) return -1;
    std::fill(c->member_reads.begin(), c->member_reads.end(), 0);
    if (n == 0) return 0;
    if (community_counts_reset(c, nullptr) || simulate_to_host(c, read_len, first, n, sim_key(seed, library_id), dst_host, "mc_community_simulate")) return -1;
    return community_counts(c, nullptr);
}

extern "C" int mc_community_member_reads(mc_community *c, int64_t *out)
{
    if (!c || !out) { g_err = "mc_community_member_reads: bad argument"; return -1; }
    memcpy(out, c->member_reads.data(), sizeof(int64_t) * (size_t)c->M);
    return 0;
}

// The fused pass: every range is simulated into the resident read buffer and searched from there (mc_run_range: a range that
// overflows a pool is run in smaller pieces) with best hits only; the best hits of the ranges are joined in read order - where
// mc_search() on the same reads ends.
extern "C" int mc_community_library(mc_handle *h, mc_community *c, int64_t nreads, uint64_t seed, uint64_t library_id)
{
    if (!h || !h->run_set) { g_err = "mc_set_run() must be called first"; return -1; }
    if (!c || nreads < 0) { g_err = "mc_community_library: bad argument"; return -1; }
    if (nreads > 0x7fffffff) { g_err = "mc_community_library: more than 2^31 - 1 reads"; return -1; }
    if (c->lib.paired_end && (nreads & 1)) { g_err = "a paired-end library has an even number of reads (" + std::to_string(nreads) + " given)"; return -1; }
    if (c->device != h->device) { g_err = "mc_community_library: the community lies on another device than the handle"; return -1; }
    if (h->pipe_nout) { g_err = "mc_community_library: ranges begun with mc_range_begin() are still in flight"; return -1; }
    ahead_drop(h);                                                  // (the resident reads are about to be simulated over)
    if (h->ab.active()) { g_err = "mc_community_library: refused while abundance counting is on (it runs best hits only; mc_set_abundance)"; return -1; }
    HIPCK(hipSetDevice(h->device));
    if (source_for_len(c, h->read_len)) return -1;
    std::fill(c->member_reads.begin(), c->member_reads.end(), 0);
    h->comm_ms[0] = h->comm_ms[1] = 0.f;
    mc_stats tot; memset(&tot, 0, sizeof tot);
    std::vector<mc_best_hit> all_best;
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.clear(); h->best_from = nullptr;
    if (nreads == 0) { h->stats = tot; return 0; }
    const int64_t B = std::min<int64_t>(nreads, stream_batch());
    if (reads_reserve(h, B) || ensure_capacity(h, h->ctx, B)) return -1;   // the resident read buffer (mc_upload's) holds one range at a time
    McEvents ev;
    if (ev.make(2)) return -1;
    hipStream_t st = h->ctx.stream;
    McModeGuard mode(h, true, h->rows_stay);
    int rc = community_counts_reset(c, st);
    const uint64_t key = sim_key(seed, library_id);
    for (int64_t at = 0; at < nreads && rc == 0; at += B) {
        const int64_t cnt = std::min(B, nreads - at);
        if (simulate_resident(h, c, key, at, cnt, ev)) { rc = -1; break; }
        if ((rc = mc_run_range(h, 0, cnt, at)) != 0) break;
        h->comm_ms[0] += ev_ms(ev[0], ev[1]);
        best_materialize(h);
        all_best.insert(all_best.end(), h->best.begin(), h->best.end());
        stats_add(tot, h->stats);
    }
    if (rc == 0) rc = community_counts(c, st); else (void)hipStreamSynchronize(st);
    if (rc) return rc;
    h->res_rows = nullptr; h->n_res_rows = 0; h->best.swap(all_best); h->best_from = nullptr; h->stats = tot;
    h->comm_ms[1] = tot.ms_total;
    return 0;
}

extern "C" int mc_community_times(const mc_handle *h, float *ms)
{
    if (!h || !ms) { g_err = "null argument"; return -1; }
    ms[0] = h->comm_ms[0]; ms[1] = h->comm_ms[1];
    return 0;
}
