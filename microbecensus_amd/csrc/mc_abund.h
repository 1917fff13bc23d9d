// mc_abund.h - the one owner of the per-gene counts (mc_set_abundance), the coverage depth (mc_set_coverage), the tie accounting
// (mc_set_ties), the rarefaction curve (mc_set_curve), the three list bootstraps - of the counts (mc_set_gene_bootstrap), of the tie
// shares (mc_set_tie_bootstrap) and of the coverage columns (mc_set_coverage_bootstrap): one McBootList each - the identity of the
// assigned reads (mc_set_identity) and the counts on class runs (mc_set_abundance_classes): where their tables lie, how their kernels
// are launched on the rows of a range, and which buffer exists when.
// With a gene fold (mc_set_gene_fold, mc_fold.h) it also owns the fold of a range's rows from segments onto genes (k_fold.h), in front of everything else.
// k_abundance.h, k_coverage.h, k_ties.h, k_curve.h, k_geneboot.h, k_tieboot.h, k_covboot.h, k_groupboot.h, k_identity.h, k_depthstats.h and k_abund_classes.h state the rules and hold the kernels; mc_hip.hip keeps the C ABI as thin wrappers (arguments,
// hipSetDevice, a call here) and the harnesses of tests/emul/ launch through mc_abund_launch like range_end, and through mc_geneboot_launch,
// mc_tieboot_launch, mc_covboot_launch, mc_groupboot_launch, mc_identity_launch and mc_depthstats_launch like the reads.
#pragma once
#include "k_abundance.h"
#include "k_coverage.h"
#include "k_ties.h"
#include "k_curve.h"
#include "k_geneboot.h"
#include "k_tieboot.h"
#include "k_covboot.h"
#include "k_groupboot.h"
#include "k_abund_classes.h"
#include "k_fold.h"
#include "k_identity.h"
#include "k_depthstats.h"
#include "mc_owned.h"

// ---- Layout: every size and offset of the four tables (k_ties.h, k_coverage.h and k_curve.h, "Layout", say what the slots hold) -----------------
// A pair table, (nseq + 1) x 2 counters: the count table ([s]: reads, aligned; [nseq][0]: assigned) and the head of the tie table
// ([s]: candidates, unique; [nseq]: ambiguous, group_ambiguous), which goes on in the SAME buffer with nseq shares and ngroups
// group_unique.  A difference array: every gene's residues and its sentinel.
static inline size_t mc_pair_slots(size_t nseq) { return 2 * (nseq + 1); }
static inline size_t mc_pair_at(size_t s) { return 2 * s; }
static inline size_t mc_tie_share_at(size_t nseq) { return mc_pair_slots(nseq); }
static inline size_t mc_tie_group_at(size_t nseq) { return mc_tie_share_at(nseq) + nseq; }
static inline size_t mc_tie_slots(size_t nseq, size_t ngroups) { return mc_tie_group_at(nseq) + ngroups; }
static inline size_t mc_diff_slots(size_t nres, size_t nseq) { return nres + nseq; }
// The curve's bin table, (K + 1) x nseq pairs, and the output of its scan: K x nseq triples and K + 1 totals (k_curve.h, "Layout")
static inline size_t mc_curve_bin_slots(size_t K, size_t nseq) { return 2 * (K + 1) * nseq; }
static inline size_t mc_curve_tot_at(size_t K, size_t nseq) { return 3 * K * nseq; }
static inline size_t mc_curve_out_slots(size_t K, size_t nseq) { return mc_curve_tot_at(K, nseq) + K + 1; }

// ---- Launch -------------------------------------------------------------------------------------------------------------------
// raw device pointers of one launch; null: that part is off.  off: the index's residue offsets (nseq + 1); counts: the count table;
// diff: the depth's difference array (coverage); ties, group_of: the tie table, the group map; diff_any: the any-depth's (coverage and ties)
struct McAbundBufs { int32_t nseq; const uint32_t *off; unsigned long long *counts; uint32_t *diff; unsigned long long *ties; const int32_t *group_of; uint32_t *diff_any; };
// the curve's part of a launch (null: the curve is off).  pts: the K points on the device; bins: the bin table; first: every residue's
// lowest covering id, or null while coverage is off; ev: recorded behind k_curve
struct McCurveBufs { int32_t K; const unsigned long long *pts; unsigned long long *bins; uint32_t *first; hipEvent_t ev; };
// a list bootstrap's part of a launch (null: it is off), for the entry E of the gene (McGbEntry), tie (McTbEntry) or coverage bootstrap
// (McCbEntry; the launch's B.off gives the genes' residues).  list: `capacity` entries; cur: the cursor and `dropped` (mc_boot_put,
// k_geneboot.h); ev: recorded behind the collect kernel
template <class E> struct McBootBufs { E *list; unsigned long long capacity; unsigned long long *cur; hipEvent_t ev; };
using McGeneBootBufs = McBootBufs<McGbEntry>; using McTieBootBufs = McBootBufs<McTbEntry>; using McCovBootBufs = McBootBufs<McCbEntry>;
// the identity's part of a launch (null: it is off).  hist: nseq x MC_ID_STRIDE counters; sums: nseq records (mc_identity.h, "Layout"); ev: recorded
// behind k_identity
struct McIdentBufs { uint32_t *hist; McIdSums *sums; hipEvent_t ev; };
// the class ride of a launch (null: the rows are no piece of a class run).  map: the ids of the batch (k_geneboot.h); tab: the per-class
// table of K classes (k_abund_classes.h); k, nreads: the piece's class and reads; ev: recorded behind k_abund_class_add
struct McClassRide { McIdMap map; unsigned long long *tab; int32_t K, k; unsigned long long nreads; hipEvent_t ev; };

// The kernels of a range's final rows (ascending read id), in `st`: the counting kernel - k_abundance_cov INSTEAD of k_abundance while
// coverage is on, the marks ride with the counts - between ev[0] and ev[1]; with ties k_ties behind it on the same rows where they
// lie, and ev[2] behind that; with the curve k_curve behind those on the same rows, and its event behind that.  The events are recorded
// with nr == 0 too: whoever reads the times need not know.  Without the curve (C null) nothing more is issued than before it existed;
// with the gene bootstrap k_geneboot_collect behind all of those on the same rows, and its event behind that - without it (G null) nothing.
// With a class ride (R not null: the rows are a piece of a class run, mc_set_abundance_classes) k_geneboot_collect_mapped runs INSTEAD of
// k_geneboot_collect and takes every id through R->map, and k_abund_class_add runs behind everything, with nr == 0 too (a piece without
// rows has reads), and R->ev behind it.  Without one (R null) nothing more is issued and the kernels are the fixed-length runs'.
// With the tie bootstrap (T not null) k_tieboot_collect runs behind the gene bootstrap's kernel on the same rows - with a class ride it
// takes every id through R->map, without one the map it is handed has a null perm - and T->ev behind it; without it (T null) nothing.
// With the coverage bootstrap (V not null; B.off is there: coverage is on) k_covboot_collect runs behind the tie bootstrap's kernel on the same
// rows, its ids taken as k_tieboot_collect takes them, and V->ev behind it; without it (V null) nothing.
// With the identity (I not null) k_identity runs behind the coverage bootstrap's kernel on the same rows - its tables are per gene, it takes no
// read id - and I->ev behind it, in front of k_abund_class_add; without it (I null) nothing.
static int mc_abund_launch(const McAbundPars &A, const McAbundBufs &B, const McRow *rows, uint32_t nr, hipStream_t st, const hipEvent_t (&ev)[3], const McCurveBufs *C = nullptr,
                           const McGeneBootBufs *G = nullptr, const McClassRide *R = nullptr, const McTieBootBufs *T = nullptr, const McCovBootBufs *V = nullptr,
                           const McIdentBufs *I = nullptr)
{
    const dim3 grid((nr + 255) / 256), block(256);
    HIPCK(hipEventRecord(ev[0], st));
    if (nr && B.diff) k_abundance_cov<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, B.counts, B.off, B.diff);
    else if (nr) k_abundance<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, B.counts);
    HIPCK(hipEventRecord(ev[1], st));
    if (B.ties) {
        if (nr) k_ties<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, B.ties, B.ties + mc_tie_share_at(B.nseq), B.group_of, B.group_of ? B.ties + mc_tie_group_at(B.nseq) : nullptr,
                                               B.diff_any ? B.off : nullptr, B.diff_any);
        HIPCK(hipEventRecord(ev[2], st));
    }
    if (C) {
        if (nr) k_curve<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, C->pts, C->K, C->bins, B.off, C->first);
        HIPCK(hipEventRecord(C->ev, st));
    }
    if (G) {
        if (nr && R) k_geneboot_collect_mapped<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, G->list, G->capacity, G->cur, R->map);
        else if (nr) k_geneboot_collect<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, G->list, G->capacity, G->cur);
        HIPCK(hipEventRecord(G->ev, st));
    }
    if (T) {
        const McIdMap own = {nullptr, 0};
        if (nr) k_tieboot_collect<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, T->list, T->capacity, T->cur, R ? R->map : own);
        HIPCK(hipEventRecord(T->ev, st));
    }
    if (V) {
        const McIdMap own = {nullptr, 0};
        if (nr) k_covboot_collect<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, B.off, V->list, V->capacity, V->cur, R ? R->map : own);
        HIPCK(hipEventRecord(V->ev, st));
    }
    if (I) {
        if (nr) k_identity<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, I->hist, I->sums);
        HIPCK(hipEventRecord(I->ev, st));
    }
    if (!R) return 0;
    k_abund_class_add<<<dim3(1), dim3(64), 0, st>>>(R->tab, R->K, R->k, R->nreads, B.counts + mc_pair_at((size_t)B.nseq));
    HIPCK(hipEventRecord(R->ev, st));
    return 0;
}

// A list bootstrap's read: raw device pointers of one read.  list: the n collected entries; cursor: nseq slots, every gene's first slot in
// the grouped list; idx: nseq compact indices; sorted: n entries; mat: ngenes x B counters - the gene bootstrap's replicate counts, the tie
// bootstrap's shares in units of 2^-32 (both zeroed), the coverage bootstrap's covered residues; scale: B doubles, m of them used (the
// tie bootstrap's: scale x 2^-32, mc_tb_scale; the coverage bootstrap's: B ones, m == B); out: ngenes x 6 doubles.  mc_gb_plan makes cursor
// and idx on the host from a pair table - the count table, or the head of the tie table (`candidates` where the other holds `reads`).
template <class E> struct McBootRead { int32_t nseq, ngenes; long long n; const E *list; uint32_t *cursor; const int32_t *idx; E *sorted; unsigned long long *mat;
                                       const double *scale; int32_t B, m; uint64_t seed; double *out; };
using McGeneBootRead = McBootRead<McGbEntry>; using McTieBootRead = McBootRead<McTbEntry>;
// start[s]: the exclusive scan of reads[s]; idx[s]: the compact index of a gene with reads, -1 of one without.  Returns the genes with reads
static int32_t mc_gb_plan(const unsigned long long *tab, int32_t nseq, uint32_t *start, int32_t *idx, unsigned long long *total)
{
    unsigned long long at = 0; int32_t ng = 0;
    for (int32_t s = 0; s < nseq; s++) { const unsigned long long r = tab[mc_pair_at((size_t)s)]; start[s] = (uint32_t)at; idx[s] = r ? ng++ : -1; at += r; }
    *total = at;
    return ng;
}
// the kernels of an entry type (the coverage bootstrap has no sums: k_covboot_cover takes their place, mc_covboot_launch)
template <class E> struct McBootKernels;
template <> struct McBootKernels<McGbEntry> { static constexpr auto scatter = k_geneboot_scatter; static constexpr auto sums = k_geneboot_sums; };
template <> struct McBootKernels<McTbEntry> { static constexpr auto scatter = k_tieboot_scatter; static constexpr auto sums = k_tieboot_sums; };
template <> struct McBootKernels<McCbEntry> { static constexpr auto scatter = k_covboot_scatter; };
// The kernels of a read between ev[0] and ev[1], in `st`: the entry type's scatter with n > 0, what `middle` issues on the grouped list,
// and k_geneboot_summary on R.mat and R.scale with ngenes > 0
template <class E, class Middle> static int mc_boot_read_launch(const McBootRead<E> &R, hipStream_t st, const hipEvent_t (&ev)[2], Middle middle)
{
    HIPCK(hipEventRecord(ev[0], st));
    if (R.n > 0) McBootKernels<E>::scatter<<<dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st>>>(R.list, R.n, R.nseq, R.cursor, R.idx, R.sorted);
    middle();
    if (R.ngenes > 0) k_geneboot_summary<<<dim3((unsigned)R.ngenes), dim3(MC_GB_THREADS), 0, st>>>(R.mat, R.scale, R.B, R.m, R.out);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(ev[1], st));
    return 0;
}
// The gene and the tie bootstrap's read: the middle is the entry type's sums, with n > 0
template <class E> static int mc_boot_launch(const McBootRead<E> &R, hipStream_t st, const hipEvent_t (&ev)[2])
{
    return mc_boot_read_launch(R, st, ev, [&] {
        if (R.n <= 0) return;
        const long long per = mc_gb_per_tile(R.n, R.B);
        McBootKernels<E>::sums<<<dim3((unsigned)((R.n + per - 1) / per), (unsigned)((R.B + MC_GB_LANES - 1) / MC_GB_LANES)), dim3(MC_GB_LANES), 0, st>>>(R.sorted, R.n, per, R.B, R.seed, (uint32_t)R.ngenes, R.mat);
    });
}
static int mc_geneboot_launch(const McGeneBootRead &R, hipStream_t st, const hipEvent_t (&ev)[2]) { return mc_boot_launch(R, st, ev); }
static int mc_tieboot_launch(const McTieBootRead &R, hipStream_t st, const hipEvent_t (&ev)[2]) { return mc_boot_launch(R, st, ev); }
// The coverage bootstrap's read (mc_covboot.h): the fields of McBootRead (ones: its scales, B doubles of 1.0 - every replicate is used) and
// genes: the ngenes genes with reads - slice, residues, need (0: no detection) - made on the host; det: ngenes counts, zeroed, or null
struct McCovBootRead { int32_t nseq, ngenes; long long n; const McCbEntry *list; uint32_t *cursor; const int32_t *idx; McCbEntry *sorted; const McCbGene *genes; unsigned long long *mat;
                       unsigned long long *det; const double *ones; int32_t B; uint64_t seed; double *out; };
// the middle is the cover kernel, with ngenes > 0
static int mc_covboot_launch(const McCovBootRead &R, hipStream_t st, const hipEvent_t (&ev)[2])
{
    const McBootRead<McCbEntry> L = {R.nseq, R.ngenes, R.n, R.list, R.cursor, R.idx, R.sorted, R.mat, R.ones, R.B, R.B, R.seed, R.out};
    return mc_boot_read_launch(L, st, ev, [&] {
        if (R.ngenes > 0) k_covboot_cover<<<dim3((unsigned)R.ngenes, (unsigned)((R.B + MC_GB_LANES - 1) / MC_GB_LANES)), dim3(MC_GB_LANES), 0, st>>>(R.sorted, R.genes, R.B, R.seed, R.mat, R.det);
    });
}

// The group bootstrap's read (mc_groupboot.h): raw device pointers of one mc_group_bootstrap, behind a read that left mat.  mat: ngenes x B
// replicate counts; start, member, kb: the CSR of the ngrp groups with reads, made by mc_grb_plan on the host; val: ngrp x B doubles;
// cnt: ngrp x B counts, or null; scale: B doubles, m of them used; out: ngrp x 6 doubles
struct McGroupBootRead { int32_t ngenes, ngrp; const unsigned long long *mat; const uint32_t *start; const uint32_t *member; const double *kb; double *val; unsigned long long *cnt;
                         const double *scale; int32_t B, m; double *out; };
// The two kernels of a read between ev[0] and ev[1], in `st`, and ev[2] between them; with ngrp == 0 only the events
static int mc_groupboot_launch(const McGroupBootRead &R, hipStream_t st, const hipEvent_t (&ev)[3])
{
    HIPCK(hipEventRecord(ev[0], st));
    if (R.ngrp > 0) k_groupboot_values<<<dim3((unsigned)R.ngrp, (unsigned)((R.B + MC_GB_LANES - 1) / MC_GB_LANES)), dim3(MC_GB_LANES), 0, st>>>(R.mat, (uint32_t)R.ngenes, R.B, R.scale, R.start, R.member, R.kb, R.val, R.cnt);
    HIPCK(hipEventRecord(ev[2], st));
    if (R.ngrp > 0) k_groupboot_summary<<<dim3((unsigned)R.ngrp), dim3(MC_GB_THREADS), 0, st>>>(R.val, R.scale, R.B, R.m, R.out);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(ev[1], st));
    return 0;
}

// The identity's read (mc_identity.h): raw device pointers of one mc_identity_read.  hist: nseq x MC_ID_STRIDE counters; level: nlevels checked
// levels; out: nseq x (3 + nlevels) values
struct McIdentRead { int32_t nseq; const uint32_t *hist; const int32_t *level; int32_t nlevels; long long *out; };
// The scan between ev[0] and ev[1], in `st`; with nseq == 0 only the events
static int mc_identity_launch(const McIdentRead &R, hipStream_t st, const hipEvent_t (&ev)[2])
{
    HIPCK(hipEventRecord(ev[0], st));
    if (R.nseq > 0) k_identity_scan<<<dim3(((unsigned)R.nseq + 3) / 4), dim3(256), 0, st>>>(R.hist, R.nseq, R.level, R.nlevels, R.out);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(ev[1], st));
    return 0;
}

// The depth statistics' read (mc_depthstats.h): raw device pointers of one mc_depth_stats.  tab: the pair table that says which genes have reads -
// the count table, or the head of the tie table for the any-depth; off: the genes' residue offsets; diff: that depth's difference array; P: the
// percent kept, 1 .. 100, checked by the caller; out: nseq x MC_DS_NOUT values
struct McDepthRead { const unsigned long long *tab; const uint32_t *off; const uint32_t *diff; int32_t nseq, P; unsigned long long *out; };
// The selection between ev[0] and ev[1], in `st`, a workgroup per gene; with nseq == 0 only the events
static int mc_depthstats_launch(const McDepthRead &R, hipStream_t st, const hipEvent_t (&ev)[2])
{
    HIPCK(hipEventRecord(ev[0], st));
    if (R.nseq > 0) k_depth_select<<<dim3((unsigned)R.nseq), dim3(MC_DS_THREADS), 0, st>>>(R.tab, R.off, R.diff, R.nseq, R.P, R.out);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(ev[1], st));
    return 0;
}

// ---- A list bootstrap's state -------------------------------------------------------------------------------------------------
template <class Tp> static int fit_one(McDev<Tp> &d, bool want, size_t n) { if (!want) d.reset(); return want && !d ? d.alloc(n) : 0; }
static int fit_one(McEvent &e, bool want) { if (!want) e.reset(); return want && !e ? e.create() : 0; }

// The nouns of a read's two refusals: what the list holds, and which pair table sizes its slices and what that table counts
struct McBootWords { const char *entries, *table, *counted, *tail; };
static const McBootWords MC_BOOT_OF_READS = {"assigned reads", "count", "assigned reads", ""}, MC_BOOT_OF_TIES = {"entries", "tie", "candidates", " entries"};
// What the prologue of a read learns on the host: the pair table, every gene's first slot and compact index (mc_gb_plan), the genes with
// entries, the used replicates and the entries of the list
struct McBootPlan { std::vector<unsigned long long> tab; std::vector<uint32_t> start; std::vector<int32_t> idx; int32_t ng = 0, m = 0; long long n = 0; };

// The read's epilogue, from the compact rows of the genes (or groups) with entries to one row each, idx.size() of them: the ng x 6 doubles
// of d_out into stats, a row without a compact index getting `empty` ..
static int mc_boot_stats(const std::vector<int32_t> &idx, int32_t ng, const double *d_out, double empty, double *stats)
{
    std::vector<double> out((size_t)MC_GB_NOUT * (size_t)ng);
    if (ng) HIPCK(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < idx.size(); s++)
        for (int k = 0; k < MC_GB_NOUT; k++) stats[MC_GB_NOUT * s + k] = idx[s] >= 0 ? out[(size_t)MC_GB_NOUT * (size_t)idx[s] + k] : empty;
    return 0;
}
// .. and the ng x B counters of d_mat into rows, a row without a compact index getting zeros
template <class T> static int mc_boot_rows(const std::vector<int32_t> &idx, int32_t ng, int32_t B, const unsigned long long *d_mat, T *rows)
{
    const size_t need = (size_t)ng * (size_t)B;
    std::vector<unsigned long long> mat(need);
    if (need) HIPCK(hipMemcpy(mat.data(), d_mat, need * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < idx.size(); s++)
        for (size_t b = 0; b < (size_t)B; b++) rows[s * (size_t)B + b] = idx[s] >= 0 ? (T)mat[(size_t)idx[s] * (size_t)B + b] : 0;
    return 0;
}

// What the gene, the tie and the coverage bootstrap each hold, for their entry E: the switch and the list's capacity; the list, its cursor
// and dropped counter, the grouped list, the genes' cursors and compact indices, the scales, the output; the matrix and what it holds;
// the event behind the collect kernel and the two around the kernels of a read; the collect kernel's and the reads' time since the last
// zeroing.
template <class E> struct McBootList {
    bool on = false; int64_t cap = 0;
    McDev<E> d_list, d_sorted; McDev<unsigned long long> d_cur, d_mat; McDev<uint32_t> d_cursor; McDev<int32_t> d_idx; McDev<double> d_scale, d_out;
    size_t mat_slots = 0;                                          // what d_mat holds: a read grows it to ngenes x B
    McEvent ev, ev_read[2];
    float collect_ms = 0, read_ms = 0;
    operator bool() const { return on; }

    // its part of THE BUFFER RULE (McAbundance::fit): the switch is `want`; the buffers exist while it is on, the matrix once a read has sized it
    int fit(bool want, size_t ns)
    {
        on = want;
        if (!on) { cap = 0; collect_ms = read_ms = 0.f; d_mat.reset(); mat_slots = 0; }
        return fit_one(d_list, on, (size_t)cap) || fit_one(d_sorted, on, (size_t)cap) || fit_one(d_cur, on, 2) || fit_one(d_cursor, on, ns) || fit_one(d_idx, on, ns) ||
               fit_one(d_scale, on, MC_GB_MAXB) || fit_one(d_out, on, (size_t)MC_GB_NOUT * ns) || fit_one(ev, on) || fit_one(ev_read[0], on) || fit_one(ev_read[1], on);
    }
    int reset()                                                    // an empty list
    {
        if (d_cur) HIPCK(hipMemset(d_cur, 0, sizeof(unsigned long long) * 2));
        collect_ms = read_ms = 0.f;
        return 0;
    }
    McBootBufs<E> bufs() const { return {d_list, (unsigned long long)cap, d_cur, ev}; }
    // A read's prologue on the host, under the caller's name `who`: the cursor (dropped: what did not fit the list - not zero: an error that
    // names it, and nothing else is done), the pair table d_tab of nseq genes, mc_gb_plan (table and list disagree: an error), and the B
    // scales, which go to the device.  setter: the switch's function, for the message
    int plan(const char *who, const char *setter, const McBootWords &W, const unsigned long long *d_tab, int32_t nseq, int32_t B, const double *scale, McBootPlan &P, int64_t *dropped)
    {
        const size_t ns = (size_t)nseq;
        unsigned long long cur[2];
        HIPCK(hipMemcpy(cur, d_cur, sizeof cur, hipMemcpyDeviceToHost));
        if (dropped) *dropped = (int64_t)cur[1];
        if (cur[1] || cur[0] > (unsigned long long)cap) {
            g_err = std::string(who) + ": " + std::to_string(cur[1]) + " " + W.entries + " did not fit the list of " + std::to_string(cap) + " entries (" + setter + "): dropped, no replicate is whole";
            return -1;
        }
        P.tab.resize(mc_pair_slots(ns)); P.start.resize(ns); P.idx.resize(ns);
        HIPCK(hipMemcpy(P.tab.data(), d_tab, P.tab.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long total = 0;
        P.ng = mc_gb_plan(P.tab.data(), nseq, P.start.data(), P.idx.data(), &total);
        if (total != cur[0]) { g_err = std::string(who) + ": the " + W.table + " table holds " + std::to_string(total) + " " + W.counted + ", the list " + std::to_string(cur[0]) + W.tail; return -1; }
        P.n = (long long)cur[0]; P.m = 0;
        for (int32_t b = 0; b < B; b++) P.m += mc_gb_used(scale[b]) ? 1 : 0;
        HIPCK(hipMemcpy(d_scale, scale, sizeof(double) * (size_t)B, hipMemcpyHostToDevice));
        return 0;
    }
    // .. and on the device: the matrix grown to ng x B, the genes' cursors and compact indices uploaded, the matrix zeroed in stream 0
    // (zero; the cover kernel writes every counter).  What the kernels of the read take is returned in R
    int stage(const McBootPlan &P, int32_t nseq, int32_t B, uint64_t seed, bool zero, McBootRead<E> &R)
    {
        const size_t ns = (size_t)nseq, need = (size_t)P.ng * (size_t)B;
        if (need > mat_slots) { mat_slots = 0; if (d_mat.alloc(need)) return -1; mat_slots = need; }
        HIPCK(hipMemcpy(d_cursor, P.start.data(), sizeof(uint32_t) * ns, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_idx, P.idx.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice));
        if (zero && need) HIPCK(hipMemsetAsync(d_mat, 0, sizeof(unsigned long long) * need, 0));
        R = {nseq, P.ng, P.n, d_list, d_cursor, d_idx, d_sorted, d_mat, d_scale, B, P.m, seed, d_out};
        return 0;
    }
    // the read's kernels, issued between ev_read[0] and ev_read[1], are waited for and their time is added to `ms`
    int finish(float &ms)
    {
        HIPCK(hipEventSynchronize(ev_read[1]));
        ms += ev_ms(ev_read[0], ev_read[1]);
        return 0;
    }
};

// ---- Owner --------------------------------------------------------------------------------------------------------------------
// The nine switches and everything that hangs on them.  THE BUFFER RULE, kept by fit() and by nobody else:
//     the count table, its two events                              exist while   counts are on
//     the difference array, the scan's output, its two events                    coverage is on
//     the depth statistics' output, its two events                               coverage is on
//     the tie table, its event                                                   ties are on
//     the group map                                                              ties are on with ngroups > 0
//     the any-depth's difference array                                           coverage and ties are on
//     the curve's points, bin table, scan output, its three events                the curve is on
//     the curve's first ids                                                       the curve and coverage are on
//     a list bootstrap's buffers and three events (McBootList::fit)               it is on; its matrix once a read has sized it
//     the coverage bootstrap's gene records and need's counts                     the coverage bootstrap is on
//     the group bootstrap's CSR, gene_kb, output and its three events; its values and counts   the gene bootstrap is on and a group read has sized them
//     the per-class table (k_abund_classes.h), its event                          the counts may ride on class runs
//     the identity's histogram, sum records, scan output, levels, its three events   the identity is on
//     the segment records, the genes' offsets, the edge counter, its two events   a gene fold is set (set_fold; with the counts on or off)
//     the folded rows                                                             a gene fold is set and a range has sized them (launch grows them)
// Coverage, ties, the curve, the gene bootstrap, the class ride and the identity are on only while the counts are; the tie bootstrap only while ties AND the gene
// bootstrap are (either going off, or being set anew, takes it with it); the coverage bootstrap only while coverage is (it is independent of the gene
// bootstrap: a list, a seed and a B of its own).  Every switch that goes on, and reset(), zeroes ALL
// counters, both difference arrays, the curve's bins (and refills its first ids with 0xFF), the cursor and dropped counter of the three bootstraps' lists
// (empty lists), the per-class table, the identity's histogram and sums, `searched` and the times: counts, depth, ties, curve, bootstrap, classes and identity describe the same reads.  A switch that goes off
// frees its buffers and zeroes nothing of the others; the counts going off take the others with them.
struct McAbundance {
    int32_t nseq = 0; size_t nres = 0; const uint32_t *off = nullptr;   // the database: bind(), once the index is on the device
    bool on = false, cov = false, ties = false, curve = false; int32_t ngroups = 0, K = 0;
    McAbundPars pars = {};
    McDev<unsigned long long> d_counts, d_covout, d_ties, d_pts, d_bins, d_curveout; McDev<uint32_t> d_diff, d_diff_any, d_first; McDev<int32_t> d_group;
    McEvent ev_count[2], ev_cov[2], ev_ties;                       // around the counting kernel of a range; around a scan; behind k_ties
    McEvent ev_curve, ev_cscan[2];                                 // behind k_curve; around a scan of the curve
    float curve_ms = 0, cscan_ms = 0;                              // k_curve's, the curve scans' time since the last zeroing
    McBootList<McGbEntry> gboot;                                   // the gene bootstrap (mc_geneboot.h)
    // what gboot.d_mat holds, so that a group read may take it over from the read before it: the replicates, the seed and the entries of the read that
    // made it; gmat_n < 0: nothing - no read yet, or a range, a reset or a switch since (launch, reset, fit)
    int32_t gmat_B = 0; uint64_t gmat_seed = 0; long long gmat_n = -1;
    McBootList<McTbEntry> tboot;                                   // the tie bootstrap (mc_tieboot.h)
    McBootList<McCbEntry> cboot;                                   // the coverage bootstrap (mc_covboot.h); its scales are B ones
    McDev<McCbGene> d_cgene; McDev<unsigned long long> d_cdet;     // its genes with reads, and how many replicates reach need
    // the names the unit harnesses of tests/emul/ read the owner's lists and the gene reads' time by
    McDev<McGbEntry> &d_glist = gboot.d_list; McDev<unsigned long long> &d_gcur = gboot.d_cur; McDev<McCbEntry> &d_clist = cboot.d_list; float &gread_ms = gboot.read_ms;
    // the group bootstrap (mc_groupboot.h): the CSR of the groups with reads, the members' gene_kb, the replicate values and counts, the output
    McDev<uint32_t> d_grstart, d_grmember; McDev<double> d_grkb, d_grval, d_grout; McDev<unsigned long long> d_grcnt;
    size_t grval_slots = 0, grcnt_slots = 0;                       // what d_grval, d_grcnt hold: a group read grows them to ngrp x B
    McEvent ev_grp[3];                                             // around the two kernels of a group read, and between them
    float grp_ms = 0, grp_values_ms = 0, grp_summary_ms = 0;       // the group reads' time since the last zeroing (with the mat they had to make), and the two kernels'
    bool classes = false;                                          // mc_set_abundance_classes: the counts may ride on class runs
    McDev<unsigned long long> d_cls; McEvent ev_cls; float cls_ms = 0;   // the per-class table; behind k_abund_class_add; its time since the last zeroing
    // the identity (mc_identity.h): the switch, the histogram, the sum records, the scan's output and levels
    bool ident = false;
    McDev<uint32_t> d_idhist; McDev<McIdSums> d_idsums; McDev<long long> d_idout; McDev<int32_t> d_idlev;
    McEvent ev_ident, ev_iscan[2];                                 // behind k_identity; around a scan
    float ident_ms = 0, iscan_ms = 0;                              // k_identity's, the scans' time since the last zeroing
    McIdMap map = {nullptr, 0}; int32_t map_K = 0, piece_k = 0;    // held while a batch's pieces run (ride_begin .. ride_end): its ids, its classes; the class of the piece that ends next
    int64_t searched = 0;                                          // the reads of the completed ranges
    // the gene fold (mc_set_gene_fold, mc_fold.h): while it is set nseq, nres and off above are the GENES' - every table, scan and reader is
    // in gene space - and ix_* keep what bind() was given, the segments of the index
    int32_t ix_nseq = 0; size_t ix_nres = 0; const uint32_t *ix_off = nullptr;
    bool fold = false; size_t folded_cap = 0;                      // folded_cap: the rows d_folded holds
    McDev<McFoldSeg> d_seg; McDev<uint32_t> d_goff; McDev<McRow> d_folded; McDev<unsigned long long> d_edge;
    McEvent ev_fold[2]; float fold_ms = 0;                          // around k_fold of a range; its time since the last zeroing
    float ms = 0, cov_ms = 0, ties_ms = 0;                         // the counting kernels', the scans', k_ties' time since the last zeroing
    McDev<unsigned long long> d_dsout; McEvent ev_ds[2]; float dstat_ms = 0;   // the depth statistics (mc_depthstats.h): the selection's output; around a read; the reads' time since the last zeroing

    void bind(int32_t nseq_, size_t nres_, const uint32_t *d_off) { nseq = ix_nseq = nseq_; nres = ix_nres = nres_; off = ix_off = d_off; }
    bool active() const { return on; }

    // ---- the switches ----
    int set_counts(bool to, const McAbundPars &A) { if (to) pars = A; return turn(on, to); }
    int set_coverage(bool to) { return turn(cov, to); }
    // group_of: nseq groups below ng, or null with ng == 0.  On while on: the tie state anew (a map of another size)
    int set_ties(bool to, const int32_t *group_of, int32_t ng)
    {
        (void)turn(ties, false);
        if (!to) return 0;
        ngroups = ng;
        if (turn(ties, true)) return -1;
        if (ng > 0 && mc_owned_ck(hipMemcpy(d_group, group_of, sizeof(int32_t) * (size_t)nseq, hipMemcpyHostToDevice), "hipMemcpy(d_tgroup, group_of)")) { (void)turn(ties, false); return -1; }
        return 0;
    }
    // points: K of them, checked by the caller (mc_set_curve).  On while on: the curve's state anew (a table of another size)
    int set_curve(int32_t K_, const unsigned long long *points)
    {
        (void)turn(curve, false);
        if (K_ == 0) return 0;
        K = K_;
        if (turn(curve, true)) return -1;
        if (mc_owned_ck(hipMemcpy(d_pts, points, sizeof(unsigned long long) * (size_t)K, hipMemcpyHostToDevice), "hipMemcpy(d_pts, points)")) { (void)turn(curve, false); return -1; }
        return 0;
    }
    // capacity: entries of the list, checked by the caller (mc_set_gene_bootstrap; mc_set_tie_bootstrap: ties and the gene bootstrap are on;
    // mc_set_coverage_bootstrap: counts and coverage are on); 0: off.  On while on: a list of another size
    int set_gene_bootstrap(int64_t capacity) { return set_list(gboot, capacity); }
    int set_tie_bootstrap(int64_t capacity) { return set_list(tboot, capacity); }
    int set_coverage_bootstrap(int64_t capacity) { return set_list(cboot, capacity); }
    // on: refused by the caller while the curve is on (mc_set_abundance_classes)
    int set_classes(bool to) { return turn(classes, to); }
    int set_identity(bool to) { return turn(ident, to); }
    // The gene fold: seg: ix_nseq records, goff: ngenes + 1 offsets of the genes' residues (both checked and made by the caller,
    // mc_set_gene_fold); ngenes == 0: off, the tables are the index's again.  The tables are sized by nseq and nres: with the counts on
    // and another size the caller has refused, so here a size changes only while every table is off; with the counts on all is zeroed.
    int set_fold(int32_t ngenes, const McFoldSeg *seg, const uint32_t *goff)
    {
        fold = false; folded_cap = 0; fold_ms = 0.f;
        d_seg.reset(); d_goff.reset(); d_folded.reset(); d_edge.reset(); ev_fold[0].reset(); ev_fold[1].reset();
        nseq = ix_nseq; nres = ix_nres; off = ix_off;
        if (ngenes == 0) return on ? reset() : 0;
        if (d_seg.alloc((size_t)ix_nseq) || d_goff.alloc((size_t)ngenes + 1) || d_edge.alloc(1) || ev_fold[0].create() || ev_fold[1].create() ||
            mc_owned_ck(hipMemcpy(d_seg, seg, sizeof(McFoldSeg) * (size_t)ix_nseq, hipMemcpyHostToDevice), "hipMemcpy(d_seg, seg)") ||
            mc_owned_ck(hipMemcpy(d_goff, goff, sizeof(uint32_t) * ((size_t)ngenes + 1), hipMemcpyHostToDevice), "hipMemcpy(d_goff, goff)") ||
            mc_owned_ck(hipMemset(d_edge, 0, sizeof(unsigned long long)), "hipMemset(d_edge)")) { (void)set_fold(0, nullptr, nullptr); return -1; }
        fold = true; nseq = ngenes; nres = (size_t)goff[ngenes]; off = d_goff;
        return on ? reset() : 0;
    }
    // what a table would be sized by under a fold of ngenes genes and nres_ residues (0 genes: the index's): the caller's refusal
    bool fold_keeps_sizes(int32_t ngenes, size_t nres_) const { return ngenes ? ngenes == nseq && nres_ == nres : ix_nseq == nseq && ix_nres == nres; }
    int read_fold(int64_t *edge_rows) const
    {
        unsigned long long e = 0;
        if (fold) HIPCK(hipMemcpy(&e, d_edge, sizeof e, hipMemcpyDeviceToHost));
        if (edge_rows) *edge_rows = (int64_t)e;
        return 0;
    }
    int reset()
    {
        HIPCK(hipMemset(d_counts, 0, sizeof(unsigned long long) * mc_pair_slots((size_t)nseq)));
        if (d_diff) HIPCK(hipMemset(d_diff, 0, sizeof(uint32_t) * mc_diff_slots(nres, (size_t)nseq)));
        if (d_ties) HIPCK(hipMemset(d_ties, 0, sizeof(unsigned long long) * mc_tie_slots((size_t)nseq, (size_t)ngroups)));
        if (d_diff_any) HIPCK(hipMemset(d_diff_any, 0, sizeof(uint32_t) * mc_diff_slots(nres, (size_t)nseq)));
        if (d_bins) HIPCK(hipMemset(d_bins, 0, sizeof(unsigned long long) * mc_curve_bin_slots((size_t)K, (size_t)nseq)));
        if (d_first) HIPCK(hipMemset(d_first, 0xFF, sizeof(uint32_t) * nres));
        if (gboot.reset() || tboot.reset() || cboot.reset()) return -1;
        if (d_cls) HIPCK(hipMemset(d_cls, 0, sizeof(unsigned long long) * MC_AC_SLOTS));
        if (d_edge) HIPCK(hipMemset(d_edge, 0, sizeof(unsigned long long)));
        if (d_idhist) HIPCK(hipMemset(d_idhist, 0, sizeof(uint32_t) * mc_id_hist_slots((size_t)nseq)));
        if (d_idsums) HIPCK(hipMemset(d_idsums, 0, sizeof(McIdSums) * (size_t)nseq));
        fold_ms = ident_ms = iscan_ms = dstat_ms = 0.f;
        searched = 0; ms = cov_ms = ties_ms = curve_ms = cscan_ms = cls_ms = 0.f;
        gmat_n = -1; grp_ms = grp_values_ms = grp_summary_ms = 0.f;
        return 0;
    }

    // ---- a range (range_end): its final rows where they lie, and what is kept once its stream has been waited for ----
    // nreads: the range's reads - the class table's, while a batch's pieces ride (ride_begin)
    // With a gene fold the rows are folded FIRST, into d_folded (grown here when a range has more rows than any before it: the kernels of
    // the range before have been waited for, range_end), and everything behind sees the folded rows: the one site where segments become genes.
    int launch(const McRow *rows, uint32_t nr, hipStream_t st, int64_t nreads = 0)
    {
        gmat_n = -1;
        if (fold) {
            if (nr > folded_cap) { folded_cap = 0; const size_t want = (size_t)nr + nr / 4 + 1024; if (d_folded.alloc(want)) return -1; folded_cap = want; }
            HIPCK(hipEventRecord(ev_fold[0], st));
            if (nr) k_fold<<<dim3((nr + 255) / 256), dim3(256), 0, st>>>(rows, nr, ix_nseq, d_seg, d_folded, d_edge);
            HIPCK(hipEventRecord(ev_fold[1], st));
            rows = d_folded;
        }
        const McAbundBufs B = {nseq, off, d_counts, d_diff, d_ties, d_group, d_diff_any};
        const hipEvent_t ev[3] = {ev_count[0], ev_count[1], ev_ties};
        const McCurveBufs C = {K, d_pts, d_bins, d_first, ev_curve};
        const McGeneBootBufs G = gboot.bufs();
        const McClassRide R = {map, d_cls, map_K, piece_k, (unsigned long long)nreads, ev_cls};
        const McTieBootBufs T = tboot.bufs();
        const McCovBootBufs V = cboot.bufs();
        const McIdentBufs I = {d_idhist, d_idsums, ev_ident};
        return mc_abund_launch(pars, B, rows, nr, st, ev, curve ? &C : nullptr, gboot ? &G : nullptr, riding() ? &R : nullptr, tboot ? &T : nullptr, cboot ? &V : nullptr, ident ? &I : nullptr);
    }
    // ---- a batch of a class run under the switch (classes_batch): perm: the row index of every sorted position, on the device, for as
    // long as the pieces run; base: the batch's first read id; K_: its classes.  ride_piece: the class of the piece whose range ends next.
    // rows_below: the rows without a class are searched by nobody - they count as searched, and in slot K of the table (no host sync)
    int ride_begin(const uint32_t *perm, int64_t base, int32_t K_, hipStream_t st)
    {
        if (!classes) return 0;
        k_abund_class_mark<<<dim3(1), dim3(64), 0, st>>>(d_cls, d_counts.get() + mc_pair_at((size_t)nseq));
        HIPCK(hipGetLastError());
        map = {perm, base}; map_K = K_; piece_k = 0;
        return 0;
    }
    void ride_piece(int32_t k) { piece_k = k; }
    void ride_end() { map = {nullptr, 0}; map_K = 0; piece_k = 0; }
    bool riding() const { return classes && map.perm != nullptr; }
    int rows_below(int64_t n, hipStream_t st)
    {
        if (!riding() || n <= 0) return 0;
        k_abund_class_add<<<dim3(1), dim3(64), 0, st>>>(d_cls, map_K, map_K, (unsigned long long)n, d_counts.get() + mc_pair_at((size_t)nseq));
        HIPCK(hipGetLastError());
        add_searched(n);
        return 0;
    }
    void range_done(int64_t nreads)
    {
        add_searched(nreads); ms += ev_ms(ev_count[0], ev_count[1]);
        if (fold) fold_ms += ev_ms(ev_fold[0], ev_fold[1]);
        hipEvent_t prev = ev_count[1];                              // the last event recorded, in mc_abund_launch's order
        const auto part = [&prev](bool is_on, hipEvent_t e, float &t) { if (is_on) { t += ev_ms(prev, e); prev = e; } };
        part(ties, ev_ties, ties_ms); part(curve, ev_curve, curve_ms);
        part(gboot.on, gboot.ev, gboot.collect_ms); part(tboot.on, tboot.ev, tboot.collect_ms); part(cboot.on, cboot.ev, cboot.collect_ms);
        part(ident, ev_ident, ident_ms); part(riding(), ev_cls, cls_ms);
    }
    void add_searched(int64_t nreads) { if (on) searched += nreads; }   // (mc_search_varlen: reads too short to have a frame are searched, and have no rows)

    // ---- the readers: the kernel of every completed range has been waited for (range_end) ----
    int read_counts(int64_t *reads, int64_t *aligned, int64_t *searched_out, int64_t *assigned) const
    {
        const size_t ns = (size_t)nseq; std::vector<unsigned long long> tab(mc_pair_slots(ns));
        HIPCK(hipMemcpy(tab.data(), d_counts, tab.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < ns; s++) { if (reads) reads[s] = (int64_t)tab[mc_pair_at(s)]; if (aligned) aligned[s] = (int64_t)tab[mc_pair_at(s) + 1]; }
        if (searched_out) *searched_out = searched; if (assigned) *assigned = (int64_t)tab[mc_pair_at(ns)];
        return 0;
    }
    int read_ties(int64_t *candidates, int64_t *unique, uint64_t *share, int64_t *group_unique, int64_t *ambiguous, int64_t *group_ambiguous) const
    {
        const size_t ns = (size_t)nseq; std::vector<unsigned long long> tab(mc_tie_slots(ns, (size_t)ngroups));
        HIPCK(hipMemcpy(tab.data(), d_ties, tab.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < ns; s++) { if (candidates) candidates[s] = (int64_t)tab[mc_pair_at(s)]; if (unique) unique[s] = (int64_t)tab[mc_pair_at(s) + 1]; if (share) share[s] = (uint64_t)tab[mc_tie_share_at(ns) + s]; }
        for (int32_t g = 0; group_unique && g < ngroups; g++) group_unique[g] = (int64_t)tab[mc_tie_group_at(ns) + (size_t)g];
        if (ambiguous) *ambiguous = (int64_t)tab[mc_pair_at(ns)]; if (group_ambiguous) *group_ambiguous = (int64_t)tab[mc_pair_at(ns) + 1];
        return 0;
    }
    // covered, spanned and max_depth per gene: of the depth, or (any) of the any-depth - the same scan over the other pair of tables
    int read_figures(bool any, int64_t *covered, int64_t *spanned, int64_t *max_depth)
    {
        if (scan(any, nullptr)) return -1;
        const size_t ns = (size_t)nseq; std::vector<unsigned long long> out(3 * ns);
        HIPCK(hipMemcpy(out.data(), d_covout, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < ns; s++) { if (covered) covered[s] = (int64_t)out[3 * s]; if (spanned) spanned[s] = (int64_t)out[3 * s + 1]; if (max_depth) max_depth[s] = (int64_t)out[3 * s + 2]; }
        return 0;
    }
    // The order statistics of every gene's depth as they stand (mc_depthstats.h): of the depth, or (any) of the any-depth with the head of the tie
    // table saying which genes have candidates - as read_figures takes its tables.  P: the percent kept, checked by the caller (mc_depth_stats).
    // median, trimmed_sum, low, high: nseq values each, every one or null.  The selection runs on the device: no residue's depth comes to the host
    int read_depth_stats(bool any, int32_t P, int64_t *median, int64_t *trimmed_sum, int64_t *low, int64_t *high)
    {
        const McDepthRead R = {any ? d_ties.get() : d_counts.get(), off, any ? d_diff_any.get() : d_diff.get(), nseq, P, d_dsout};
        const hipEvent_t ev[2] = {ev_ds[0], ev_ds[1]};
        if (mc_depthstats_launch(R, 0, ev)) return -1;
        HIPCK(hipEventSynchronize(ev_ds[1]));
        dstat_ms += ev_ms(ev_ds[0], ev_ds[1]);
        const size_t ns = (size_t)nseq; std::vector<unsigned long long> out(mc_ds_out_slots(ns));
        HIPCK(hipMemcpy(out.data(), d_dsout, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        int64_t *const to[MC_DS_NOUT] = {median, trimmed_sum, low, high};      // (MC_DS_MEDIAN, MC_DS_SUM, MC_DS_LOW, MC_DS_HIGH)
        for (size_t s = 0; s < ns; s++)
            for (int k = 0; k < MC_DS_NOUT; k++) if (to[k]) to[k][s] = (int64_t)out[MC_DS_NOUT * s + (size_t)k];
        return 0;
    }
    // the curve as it stands: reads, aligned and (or null) covered as K x nseq values, point by point; assigned: K values; beyond: one
    int read_curve(int64_t *reads, int64_t *aligned, int64_t *covered, int64_t *assigned, int64_t *beyond)
    {
        const size_t ns = (size_t)nseq, nk = (size_t)K, tot = mc_curve_tot_at(nk, ns);
        HIPCK(hipMemsetAsync(d_curveout.get() + tot, 0, sizeof(unsigned long long) * (nk + 1), 0));
        HIPCK(hipEventRecord(ev_cscan[0], 0));
        k_curve_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256), 0, 0>>>(d_counts, d_bins, d_pts, K, off, d_first, nseq, d_curveout, d_curveout.get() + tot);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(ev_cscan[1], 0));
        HIPCK(hipEventSynchronize(ev_cscan[1]));
        cscan_ms += ev_ms(ev_cscan[0], ev_cscan[1]);
        std::vector<unsigned long long> out(mc_curve_out_slots(nk, ns));
        HIPCK(hipMemcpy(out.data(), d_curveout, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nk * ns; i++) { if (reads) reads[i] = (int64_t)out[3 * i]; if (aligned) aligned[i] = (int64_t)out[3 * i + 1]; if (covered) covered[i] = (int64_t)out[3 * i + 2]; }
        for (size_t k = 0; assigned && k < nk; k++) assigned[k] = (int64_t)out[tot + k];
        if (beyond) *beyond = (int64_t)out[tot + nk];
        return 0;
    }
    // The bootstrap of the counts as they stand (mc_geneboot.h): B replicates under `seed`, scale: B doubles.  counts (or null): nseq x B
    // replicate counts; stats: nseq x 6 doubles; dropped: the assigned reads that did not fit the list - not zero: an error that names it,
    // and nothing else is computed.
    int read_gene_bootstrap(int32_t B, uint64_t seed, const double *scale, int64_t *counts, double *stats, int64_t *dropped)
    {
        McBootPlan P;
        if (make_mat("mc_gene_bootstrap", B, seed, scale, false, P, dropped, gboot.read_ms)) return -1;
        if (mc_boot_stats(P.idx, P.ng, gboot.d_out, P.m ? 0.0 : mc_gb_nan(), stats)) return -1;   // (a gene without reads: zero in every replicate)
        return counts ? mc_boot_rows(P.idx, P.ng, B, gboot.d_mat, counts) : 0;
    }
    // The bootstrap of the tie shares as they stand (mc_tieboot.h): read_gene_bootstrap's contract on the tie list, its slices sized by the head of
    // the tie table.  shares (or null): nseq x B replicate shares in units of 2^-32; stats: nseq x 6 doubles of the values share x scale x 2^-32;
    // dropped: the entries that did not fit the list - not zero: an error that names it, and nothing else is computed.
    int read_tie_bootstrap(int32_t B, uint64_t seed, const double *scale, uint64_t *shares, double *stats, int64_t *dropped)
    {
        std::vector<double> s32((size_t)B);
        for (int32_t b = 0; b < B; b++) s32[(size_t)b] = mc_tb_scale(scale[b]);
        McBootPlan P; McBootRead<McTbEntry> R;
        if (tboot.plan("mc_tie_bootstrap", "mc_set_tie_bootstrap", MC_BOOT_OF_TIES, d_ties, nseq, B, s32.data(), P, dropped) || tboot.stage(P, nseq, B, seed, true, R)) return -1;
        const hipEvent_t ev[2] = {tboot.ev_read[0], tboot.ev_read[1]};
        if (mc_tieboot_launch(R, 0, ev) || tboot.finish(tboot.read_ms)) return -1;
        if (mc_boot_stats(P.idx, P.ng, tboot.d_out, P.m ? 0.0 : mc_gb_nan(), stats)) return -1;   // (a gene without candidates: zero in every replicate)
        return shares ? mc_boot_rows(P.idx, P.ng, B, tboot.d_mat, shares) : 0;
    }
    // The bootstrap of the coverage columns as they stand (mc_covboot.h): B replicates under `seed`.  need (or null): nseq values, none of them 0,
    // checked by the caller; covered (or null): nseq x B covered residues; stats: nseq x 6 doubles of those values, every replicate used;
    // detected (or null; only with need): nseq counts of the replicates with covered >= need; dropped: the assigned reads that did not fit the
    // list - not zero: an error that names it, and nothing else is computed.
    int read_coverage_bootstrap(int32_t B, uint64_t seed, const uint32_t *need, int64_t *covered, double *stats, int64_t *detected, int64_t *dropped)
    {
        const size_t ns = (size_t)nseq;
        const std::vector<double> ones((size_t)B, 1.0);
        McBootPlan P; McBootRead<McCbEntry> R;
        if (cboot.plan("mc_coverage_bootstrap", "mc_set_coverage_bootstrap", MC_BOOT_OF_READS, d_counts, nseq, B, ones.data(), P, dropped)) return -1;
        std::vector<uint32_t> hoff(ns + 1);
        HIPCK(hipMemcpy(hoff.data(), off, sizeof(uint32_t) * (ns + 1), hipMemcpyDeviceToHost));   // (the genes' residues: the index's offsets, or the fold's)
        std::vector<McCbGene> genes((size_t)P.ng);
        for (size_t s = 0; s < ns; s++)
            if (P.idx[s] >= 0) genes[(size_t)P.idx[s]] = {P.start[s], (uint32_t)P.tab[mc_pair_at(s)], hoff[s + 1] - hoff[s], need ? need[s] : 0u};
        if (cboot.stage(P, nseq, B, seed, false, R)) return -1;
        if (P.ng) HIPCK(hipMemcpy(d_cgene, genes.data(), sizeof(McCbGene) * (size_t)P.ng, hipMemcpyHostToDevice));
        HIPCK(hipMemsetAsync(d_cdet, 0, sizeof(unsigned long long) * ns, 0));
        const hipEvent_t ev[2] = {cboot.ev_read[0], cboot.ev_read[1]};
        const McCovBootRead C = {R.nseq, R.ngenes, R.n, R.list, R.cursor, R.idx, R.sorted, d_cgene, R.mat, need ? d_cdet.get() : nullptr, R.scale, B, seed, R.out};
        if (mc_covboot_launch(C, 0, ev) || cboot.finish(cboot.read_ms)) return -1;
        if (mc_boot_stats(P.idx, P.ng, cboot.d_out, 0.0, stats)) return -1;   // (a gene without reads: nothing covered in any replicate)
        if (detected && mc_boot_rows(P.idx, P.ng, 1, d_cdet, detected)) return -1;
        return covered ? mc_boot_rows(P.idx, P.ng, B, cboot.d_mat, covered) : 0;
    }
    // The bootstrap of the GROUPS (mc_groupboot.h) on the counts as they stand: group_of: nseq groups below ngroups_, gene_kb: nseq doubles, all
    // checked by the caller (mc_group_bootstrap).  counts (or null): ngroups_ x B group replicate counts; stats: ngroups_ x 6 doubles.  mat is
    // that of the read before when it is still this one's (the same B, seed and entries, no range since), and made here otherwise.
    int read_group_bootstrap(int32_t B, uint64_t seed, const double *scale, const int32_t *group_of, int32_t ngroups_, const double *gene_kb, int64_t *counts, double *stats, int64_t *dropped)
    {
        const size_t ns = (size_t)nseq, ngr = (size_t)ngroups_;
        McBootPlan P; float took = 0.f;
        if (make_mat("mc_group_bootstrap", B, seed, scale, true, P, dropped, took)) return -1;
        const int32_t ng = P.ng;
        std::vector<int32_t> gidx(ngr); std::vector<uint32_t> start(ngr + 1), member((size_t)ng); std::vector<double> kb((size_t)ng);
        const int32_t ngrp = mc_grb_plan(P.idx.data(), nseq, group_of, ngroups_, gene_kb, gidx.data(), start.data(), member.data(), kb.data());
        const size_t need = (size_t)ngrp * (size_t)B;
        if (!d_grstart && (d_grstart.alloc(ns + 1) || d_grmember.alloc(ns) || d_grkb.alloc(ns) || d_grout.alloc((size_t)MC_GB_NOUT * ns) || ev_grp[0].create() || ev_grp[1].create() || ev_grp[2].create())) {
            d_grstart.reset(); return -1;
        }
        if (need > grval_slots) { grval_slots = 0; if (d_grval.alloc(need)) return -1; grval_slots = need; }
        if (counts && need > grcnt_slots) { grcnt_slots = 0; if (d_grcnt.alloc(need)) return -1; grcnt_slots = need; }
        HIPCK(hipMemcpy(d_grstart, start.data(), sizeof(uint32_t) * ((size_t)ngrp + 1), hipMemcpyHostToDevice));
        if (ng) HIPCK(hipMemcpy(d_grmember, member.data(), sizeof(uint32_t) * (size_t)ng, hipMemcpyHostToDevice));
        if (ng) HIPCK(hipMemcpy(d_grkb, kb.data(), sizeof(double) * (size_t)ng, hipMemcpyHostToDevice));
        const McGroupBootRead R = {ng, ngrp, gboot.d_mat, d_grstart, d_grmember, d_grkb, d_grval, counts ? d_grcnt.get() : nullptr, gboot.d_scale, B, P.m, d_grout};
        const hipEvent_t ev[3] = {ev_grp[0], ev_grp[1], ev_grp[2]};
        if (mc_groupboot_launch(R, 0, ev)) return -1;
        HIPCK(hipEventSynchronize(ev_grp[1]));
        const float tv = ev_ms(ev_grp[0], ev_grp[2]), ts = ev_ms(ev_grp[2], ev_grp[1]);
        grp_values_ms += tv; grp_summary_ms += ts; grp_ms += took + tv + ts;
        if (mc_boot_stats(gidx, ngrp, d_grout, P.m ? 0.0 : mc_gb_nan(), stats)) return -1;   // (a group without reads: zero in every replicate)
        return counts ? mc_boot_rows(gidx, ngrp, B, d_grcnt, counts) : 0;
    }
    // the per-class table as it stands: n pairs, class 0 .. n - 2 and the rows below the lowest class (the caller knows its K: n = K + 1)
    int read_classes(int64_t *rows, int64_t *assigned, int32_t n) const
    {
        unsigned long long tab[MC_AC_SLOTS];
        HIPCK(hipMemcpy(tab, d_cls, sizeof tab, hipMemcpyDeviceToHost));
        for (int32_t k = 0; k < n; k++) { if (rows) rows[k] = (int64_t)tab[2 * k]; if (assigned) assigned[k] = (int64_t)tab[2 * k + 1]; }
        return 0;
    }
    // The identity as it stands (mc_identity.h): level: nlevels levels, checked by the caller (mc_identity_read).  The sums and the three bins per
    // gene (MC_ID_NONE for a gene without reads), every one or null; ge (or null): nseq x nlevels counts, gene by gene.  The scan runs on the
    // device: the histogram does not come to the host
    int read_identity(const int32_t *level, int32_t nlevels, int64_t *matched, int64_t *mismatched, int64_t *gap_opens, int32_t *imin, int32_t *imedian, int32_t *imax, int64_t *ge)
    {
        const size_t ns = (size_t)nseq, nout = 3 + (size_t)nlevels;
        if (nlevels) HIPCK(hipMemcpy(d_idlev, level, sizeof(int32_t) * (size_t)nlevels, hipMemcpyHostToDevice));
        const McIdentRead R = {nseq, d_idhist, d_idlev, nlevels, d_idout};
        const hipEvent_t ev[2] = {ev_iscan[0], ev_iscan[1]};
        if (mc_identity_launch(R, 0, ev)) return -1;
        HIPCK(hipEventSynchronize(ev_iscan[1]));
        iscan_ms += ev_ms(ev_iscan[0], ev_iscan[1]);
        std::vector<long long> out(nout * ns); std::vector<McIdSums> sums(ns);
        HIPCK(hipMemcpy(out.data(), d_idout, out.size() * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(sums.data(), d_idsums, ns * sizeof(McIdSums), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < ns; s++) {
            if (matched) matched[s] = (int64_t)sums[s].matched; if (mismatched) mismatched[s] = (int64_t)sums[s].mismatched; if (gap_opens) gap_opens[s] = (int64_t)sums[s].gap_opens;
            if (imin) imin[s] = (int32_t)out[nout * s]; if (imedian) imedian[s] = (int32_t)out[nout * s + 1]; if (imax) imax[s] = (int32_t)out[nout * s + 2];
            for (size_t j = 0; ge && j < (size_t)nlevels; j++) ge[(size_t)nlevels * s + j] = (int64_t)out[nout * s + 3 + j];
        }
        return 0;
    }
    // the histogram without its padding: nseq x MC_ID_BINS counters
    int read_identity_hist(uint32_t *hist) const
    {
        if (nseq) HIPCK(hipMemcpy2D(hist, sizeof(uint32_t) * MC_ID_BINS, d_idhist, sizeof(uint32_t) * MC_ID_STRIDE, sizeof(uint32_t) * MC_ID_BINS, (size_t)nseq, hipMemcpyDeviceToHost));
        return 0;
    }
    int read_depth(uint32_t *depth)                                // nres values
    {
        McDevBuf buf; uint32_t *d_depth = nullptr;
        if (buf.get(&d_depth, nres) || scan(false, d_depth)) return -1;
        HIPCK(hipMemcpy(depth, d_depth, sizeof(uint32_t) * nres, hipMemcpyDeviceToHost));
        return 0;
    }

private:
    // mat of the counts as they stand - genes with reads x B replicate counts under `seed` - and the six doubles of every gene with reads in gboot.d_out,
    // through ONE copy of the count table: the list's refusals under the caller's name `who`, the plan P, the three kernels of mc_geneboot_launch,
    // their milliseconds added to `took`.  With reuse, a mat that is still this one's (gmat_*) is kept and nothing is launched: the scales alone
    // go to the device.
    int make_mat(const char *who, int32_t B, uint64_t seed, const double *scale, bool reuse, McBootPlan &P, int64_t *dropped, float &took)
    {
        if (gboot.plan(who, "mc_set_gene_bootstrap", MC_BOOT_OF_READS, d_counts, nseq, B, scale, P, dropped)) return -1;
        if (reuse && gmat_n == P.n && gmat_B == B && gmat_seed == seed) return 0;
        gmat_n = -1;
        McBootRead<McGbEntry> R;
        if (gboot.stage(P, nseq, B, seed, true, R)) return -1;
        const hipEvent_t ev[2] = {gboot.ev_read[0], gboot.ev_read[1]};
        if (mc_geneboot_launch(R, 0, ev) || gboot.finish(took)) return -1;
        gmat_B = B; gmat_seed = seed; gmat_n = P.n;
        return 0;
    }
    template <class E> int set_list(McBootList<E> &L, int64_t capacity)
    {
        (void)turn(L.on, false);
        if (capacity == 0) return 0;
        L.cap = capacity;
        return turn(L.on, true);
    }
    // the switches as they stand, made consistent; then the buffer rule: what they need is made where it is missing, everything else freed
    int fit()
    {
        if (!on) { cov = ties = curve = gboot.on = classes = ident = false; searched = 0; ms = 0.f; }
        if (!ident) ident_ms = iscan_ms = 0.f;
        if (!classes) { cls_ms = 0.f; ride_end(); }
        if (!cov) cov_ms = dstat_ms = 0.f;
        if (!ties) { ngroups = 0; ties_ms = 0.f; }
        if (!curve) { K = 0; curve_ms = cscan_ms = 0.f; }
        if (!gboot.on) {
            grp_ms = grp_values_ms = grp_summary_ms = 0.f; gmat_n = -1;
            d_grstart.reset(); d_grmember.reset(); d_grkb.reset(); d_grval.reset(); d_grcnt.reset(); d_grout.reset(); grval_slots = grcnt_slots = 0;
            for (McEvent &e : ev_grp) e.reset();
        }
        const size_t ns = (size_t)nseq, slots = mc_diff_slots(nres, ns);
        return fit_one(d_counts, on, mc_pair_slots(ns)) || fit_one(ev_count[0], on) || fit_one(ev_count[1], on) ||
               fit_one(d_diff, cov, slots) || fit_one(d_covout, cov, 3 * ns) || fit_one(ev_cov[0], cov) || fit_one(ev_cov[1], cov) ||
               fit_one(d_dsout, cov, mc_ds_out_slots(ns)) || fit_one(ev_ds[0], cov) || fit_one(ev_ds[1], cov) ||
               fit_one(d_ties, ties, mc_tie_slots(ns, (size_t)ngroups)) || fit_one(ev_ties, ties) || fit_one(d_group, ties && ngroups > 0, ns) ||
               fit_one(d_diff_any, cov && ties, slots) ||
               fit_one(d_pts, curve, MC_CURVE_MAXK) || fit_one(d_bins, curve, mc_curve_bin_slots((size_t)K, ns)) || fit_one(d_curveout, curve, mc_curve_out_slots((size_t)K, ns)) ||
               fit_one(ev_curve, curve) || fit_one(ev_cscan[0], curve) || fit_one(ev_cscan[1], curve) || fit_one(d_first, curve && cov, nres) ||
               gboot.fit(gboot.on, ns) || tboot.fit(tboot.on && ties && gboot.on, ns) || cboot.fit(cboot.on && cov, ns) || fit_one(d_cgene, cboot.on, ns) || fit_one(d_cdet, cboot.on, ns) ||
               fit_one(d_cls, classes, MC_AC_SLOTS) || fit_one(ev_cls, classes) ||
               fit_one(d_idhist, ident, mc_id_hist_slots(ns)) || fit_one(d_idsums, ident, ns) || fit_one(d_idout, ident, mc_id_out_slots(ns)) || fit_one(d_idlev, ident, MC_ID_LEVELS) ||
               fit_one(ev_ident, ident) || fit_one(ev_iscan[0], ident) || fit_one(ev_iscan[1], ident);
    }
    // one switch to `to`.  A switch whose buffers cannot be had ends off and leaves the others as they were (freeing cannot fail).
    int turn(bool &sw, bool to)
    {
        sw = to;
        if (fit()) { sw = false; (void)fit(); return -1; }
        return to ? reset() : 0;
    }
    // the scan of a difference array as it stands, into d_covout and (when given) d_depth: device memory of nres values
    int scan(bool any, uint32_t *d_depth)
    {
        if (d_depth) HIPCK(hipMemsetAsync(d_depth, 0, sizeof(uint32_t) * nres, 0));
        HIPCK(hipEventRecord(ev_cov[0], 0));
        k_coverage_scan<<<dim3(((unsigned)nseq + 3) / 4), dim3(256), 0, 0>>>(any ? d_ties.get() : d_counts.get(), off, any ? d_diff_any.get() : d_diff.get(), nseq, d_covout, d_depth);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(ev_cov[1], 0));
        HIPCK(hipEventSynchronize(ev_cov[1]));
        cov_ms += ev_ms(ev_cov[0], ev_cov[1]);
        return 0;
    }
};
