// mc_abund.h - the one owner of the per-gene counts (mc_set_abundance), the coverage depth (mc_set_coverage), the tie accounting
// (mc_set_ties) and the rarefaction curve (mc_set_curve): where their tables lie, how their kernels are launched on the rows of a range,
// and which buffer exists when.
// k_abundance.h, k_coverage.h, k_ties.h and k_curve.h state the rules and hold the kernels; mc_hip.hip keeps the C ABI as thin wrappers (arguments,
// hipSetDevice, a call here) and tests/emul/device_coverage.hip, device_ties.hip and device_curve.hip launch through mc_abund_launch like range_end.
#pragma once
#include "k_abundance.h"
#include "k_coverage.h"
#include "k_ties.h"
#include "k_curve.h"
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

// The kernels of a range's final rows (ascending read id), in `st`: the counting kernel - k_abundance_cov INSTEAD of k_abundance while
// coverage is on, the marks ride with the counts - between ev[0] and ev[1]; with ties k_ties behind it on the same rows where they
// lie, and ev[2] behind that; with the curve k_curve behind those on the same rows, and its event behind that.  The events are recorded
// with nr == 0 too: whoever reads the times need not know.  Without the curve (C null) nothing more is issued than before it existed.
static int mc_abund_launch(const McAbundPars &A, const McAbundBufs &B, const McRow *rows, uint32_t nr, hipStream_t st, const hipEvent_t (&ev)[3], const McCurveBufs *C = nullptr)
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
    if (!C) return 0;
    if (nr) k_curve<<<grid, block, 0, st>>>(A, rows, nr, B.nseq, C->pts, C->K, C->bins, B.off, C->first);
    HIPCK(hipEventRecord(C->ev, st));
    return 0;
}

// ---- Owner --------------------------------------------------------------------------------------------------------------------
// The four switches and everything that hangs on them.  THE BUFFER RULE, kept by fit() and by nobody else:
//     the count table, its two events                              exist while   counts are on
//     the difference array, the scan's output, its two events                    coverage is on
//     the tie table, its event                                                   ties are on
//     the group map                                                              ties are on with ngroups > 0
//     the any-depth's difference array                                           coverage and ties are on
//     the curve's points, bin table, scan output, its three events                the curve is on
//     the curve's first ids                                                       the curve and coverage are on
// Coverage, ties and the curve are on only while the counts are.  Every switch that goes on, and reset(), zeroes ALL counters, both
// difference arrays, the curve's bins (and refills its first ids with 0xFF), `searched` and the times: counts, depth, ties and curve
// describe the same reads.  A switch that goes off frees its buffers and zeroes nothing of the others; the counts going off take the
// other three with them.
struct McAbundance {
    int32_t nseq = 0; size_t nres = 0; const uint32_t *off = nullptr;   // the database: bind(), once the index is on the device
    bool on = false, cov = false, ties = false, curve = false; int32_t ngroups = 0, K = 0;
    McAbundPars pars = {};
    McDev<unsigned long long> d_counts, d_covout, d_ties, d_pts, d_bins, d_curveout; McDev<uint32_t> d_diff, d_diff_any, d_first; McDev<int32_t> d_group;
    McEvent ev_count[2], ev_cov[2], ev_ties;                       // around the counting kernel of a range; around a scan; behind k_ties
    McEvent ev_curve, ev_cscan[2];                                 // behind k_curve; around a scan of the curve
    float curve_ms = 0, cscan_ms = 0;                              // k_curve's, the curve scans' time since the last zeroing
    int64_t searched = 0;                                          // the reads of the completed ranges
    float ms = 0, cov_ms = 0, ties_ms = 0;                         // the counting kernels', the scans', k_ties' time since the last zeroing

    void bind(int32_t nseq_, size_t nres_, const uint32_t *d_off) { nseq = nseq_; nres = nres_; off = d_off; }
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
    int reset()
    {
        HIPCK(hipMemset(d_counts, 0, sizeof(unsigned long long) * mc_pair_slots((size_t)nseq)));
        if (d_diff) HIPCK(hipMemset(d_diff, 0, sizeof(uint32_t) * mc_diff_slots(nres, (size_t)nseq)));
        if (d_ties) HIPCK(hipMemset(d_ties, 0, sizeof(unsigned long long) * mc_tie_slots((size_t)nseq, (size_t)ngroups)));
        if (d_diff_any) HIPCK(hipMemset(d_diff_any, 0, sizeof(uint32_t) * mc_diff_slots(nres, (size_t)nseq)));
        if (d_bins) HIPCK(hipMemset(d_bins, 0, sizeof(unsigned long long) * mc_curve_bin_slots((size_t)K, (size_t)nseq)));
        if (d_first) HIPCK(hipMemset(d_first, 0xFF, sizeof(uint32_t) * nres));
        searched = 0; ms = cov_ms = ties_ms = curve_ms = cscan_ms = 0.f;
        return 0;
    }

    // ---- a range (range_end): its final rows where they lie, and what is kept once its stream has been waited for ----
    int launch(const McRow *rows, uint32_t nr, hipStream_t st)
    {
        const McAbundBufs B = {nseq, off, d_counts, d_diff, d_ties, d_group, d_diff_any};
        const hipEvent_t ev[3] = {ev_count[0], ev_count[1], ev_ties};
        const McCurveBufs C = {K, d_pts, d_bins, d_first, ev_curve};
        return mc_abund_launch(pars, B, rows, nr, st, ev, curve ? &C : nullptr);
    }
    void range_done(int64_t nreads)
    {
        add_searched(nreads); ms += ev_ms(ev_count[0], ev_count[1]);
        if (ties) ties_ms += ev_ms(ev_count[1], ev_ties);
        if (curve) curve_ms += ev_ms(ties ? ev_ties : ev_count[1], ev_curve);
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
    int read_depth(uint32_t *depth)                                // nres values
    {
        McDevBuf buf; uint32_t *d_depth = nullptr;
        if (buf.get(&d_depth, nres) || scan(false, d_depth)) return -1;
        HIPCK(hipMemcpy(depth, d_depth, sizeof(uint32_t) * nres, hipMemcpyDeviceToHost));
        return 0;
    }

private:
    template <class Tp> static int fit_one(McDev<Tp> &d, bool want, size_t n) { if (!want) d.reset(); return want && !d ? d.alloc(n) : 0; }
    static int fit_one(McEvent &e, bool want) { if (!want) e.reset(); return want && !e ? e.create() : 0; }
    // the switches as they stand, made consistent; then the buffer rule: what they need is made where it is missing, everything else freed
    int fit()
    {
        if (!on) { cov = ties = curve = false; searched = 0; ms = 0.f; }
        if (!cov) cov_ms = 0.f;
        if (!ties) { ngroups = 0; ties_ms = 0.f; }
        if (!curve) { K = 0; curve_ms = cscan_ms = 0.f; }
        const size_t ns = (size_t)nseq, slots = mc_diff_slots(nres, ns);
        return fit_one(d_counts, on, mc_pair_slots(ns)) || fit_one(ev_count[0], on) || fit_one(ev_count[1], on) ||
               fit_one(d_diff, cov, slots) || fit_one(d_covout, cov, 3 * ns) || fit_one(ev_cov[0], cov) || fit_one(ev_cov[1], cov) ||
               fit_one(d_ties, ties, mc_tie_slots(ns, (size_t)ngroups)) || fit_one(ev_ties, ties) || fit_one(d_group, ties && ngroups > 0, ns) ||
               fit_one(d_diff_any, cov && ties, slots) ||
               fit_one(d_pts, curve, MC_CURVE_MAXK) || fit_one(d_bins, curve, mc_curve_bin_slots((size_t)K, ns)) || fit_one(d_curveout, curve, mc_curve_out_slots((size_t)K, ns)) ||
               fit_one(ev_curve, curve) || fit_one(ev_cscan[0], curve) || fit_one(ev_cscan[1], curve) || fit_one(d_first, curve && cov, nres);
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
