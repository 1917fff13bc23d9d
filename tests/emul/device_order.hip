// tests/emul/device_order.hip - the ordering and finishing kernels' device algorithms (csrc/k_order.h, csrc/k_finish.h) run on inputs
// built to reach their edges: a stand-alone program that includes the library's kernel headers in mc_hip.hip's order - it compiles the
// text the library compiles and copies none of it - and links neither the library nor the reader.
//   device_order CASE IN OUT      (files of sections: order_io.h; tests/order_cases.py writes IN and reads OUT)
// Cases: wave_sort, thread_sorts, mergesort, order, heap_lanes, counting_sorts, bins_and_scan - and adversary (host only: the frozen
// keys of McIlroy's adversary, wave_sort_form.h).  Stage C's binning and ordering run through csrc/mc_stages.h, the launch functions
// the library's own stage C calls - fork, joins and all; every LDS size, grid constant and the heavy words' offset come from there and
// from k_finish.h.  Three single kernels are launched here directly (k_heap_lanes, k_heavy_order, k_heap_order: the header wraps the
// finishing chain as a whole, and these cases feed one kernel lists and words the chain itself would never hand it); the wrapper kernels below (t_*)
// only stage a function's input in LDS and carry its result out.
// Expected values come from the product's host-compilable statements (mc_std_sort, mc_heapsort, mc_build_stacks) and go to OUT beside
// the device's; the test compares.  Every HIP call is checked: an error is printed and ends the program with status 3 at once.
#include "mc_hip_common.h"
#include "k_translate_seg.h"
#include "k_enumerate.h"
#include "k_eval_seeds.h"
#include "k_gapped.h"
#include "k_order.h"
#include "k_finish.h"
#include "mc_stages.h"

#include "order_io.h"
#include "wave_sort_form.h"
#include "order_expect.h"
#include "device_ck.h"                                              // CK, CK_LAUNCH, Dev<T>

// ---- a. mc_wave_std_sort: a wave per array, the items and the three index arrays in LDS as k_finish_heavy<MAXN> lays them out -----
template <int MAXN>
__global__ void __launch_bounds__(64) t_wave_sort(const double *__restrict__ keys, const uint32_t *__restrict__ off, uint32_t *perm)
{
    McSortItem *items = (McSortItem *)mc_smem;
    uint16_t *gst = (uint16_t *)(items + MAXN), *gkept = gst + (MAXN + 2), *gofs = gkept + (MAXN + 2);
    __shared__ int s_stk[3 * 64];
    const int lane = mc_lane();
    const uint32_t a = off[blockIdx.x];
    const int n = (int)(off[blockIdx.x + 1] - a);
    for (int i = lane; i < n; i += 64) { McSortItem it; it.k = keys[a + i]; it.i = (uint32_t)i; it.pad = 0; items[i] = it; }
    __syncthreads();
    mc_wave_std_sort(items, n, gst, gkept, gofs, s_stk, lane);
    __syncthreads();
    for (int i = lane; i < n; i += 64) perm[a + i] = items[i].i;
}
template <int MAXN>
static void wave_sort_set(const uint32_t *off, size_t narr, const double *keys, size_t nkeys, Sections &out)
{
    for (size_t b = 0; b < narr; b++) if (off[b + 1] - off[b] > (uint32_t)MAXN) { fprintf(stderr, "wave_sort: array %zu longer than %d\n", b, MAXN); exit(2); }
    const size_t lds = mc_finish_heavy_lds(MAXN);
    if (lds > 48 * 1024) CK(hipFuncSetAttribute((const void *)t_wave_sort<MAXN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Dev<double> d_keys(keys, nkeys);
    Dev<uint32_t> d_off(off, narr + 1), d_perm(nkeys, 0xFF);
    if (narr) { t_wave_sort<MAXN><<<dim3((unsigned)narr), dim3(64), lds>>>(d_keys, d_off, d_perm); CK_LAUNCH(); }
    out.put(d_perm.host());
    std::vector<uint32_t> want;
    std::vector<int32_t> stats;
    for (size_t b = 0; b < narr; b++) {
        const int n = (int)(off[b + 1] - off[b]);
        std::vector<McSortItem> x(n + 1), y(n + 1);
        for (int i = 0; i < n; i++) { x[i].k = keys[off[b] + i]; x[i].i = (uint32_t)i; x[i].pad = 0; y[i] = x[i]; }
        mc_std_sort(x.data(), (long)n, 0);
        for (int i = 0; i < n; i++) want.push_back(x[i].i);
        WaveSortStats st;                                          // (the formulation with the counters: was the fallback reached, and how long)
        wave_sort_form(y.data(), n, st);
        stats.push_back((int32_t)st.fallbacks); stats.push_back((int32_t)st.largest); stats.push_back((int32_t)st.overflow);
    }
    out.put(want); out.put(stats);
}
static void case_wave_sort(Sections &in, Sections &out)
{
    const uint32_t nsets = *in.take<uint32_t>();
    for (uint32_t q = 0; q < nsets; q++) {
        size_t no, nk;
        const uint32_t maxn = *in.take<uint32_t>();
        const uint32_t *off = in.take<uint32_t>(&no);
        const double *keys = in.take<double>(&nk);
        if (maxn == MC_FH_N1) wave_sort_set<MC_FH_N1>(off, no - 1, keys, nk, out);
        else if (maxn == MC_FH_N2) wave_sort_set<MC_FH_N2>(off, no - 1, keys, nk, out);
        else if (maxn == MC_FH_N3) wave_sort_set<MC_FH_N3>(off, no - 1, keys, nk, out);
        else { fprintf(stderr, "wave_sort: MAXN %u is none of the library's\n", maxn); exit(2); }
    }
}

// ---- b. mc_std_sort_inl / mc_heapsort_inl on a thread's own stretch of LDS, placed as k_finish<TPB, ITEMS, .> places it -------------
template <int TPB, int ITEMS>
__global__ void __launch_bounds__(TPB) t_thread_sorts(const double *__restrict__ keys, const uint32_t *__restrict__ off, uint32_t narr, int heap, uint32_t *perm)
{
    constexpr int STRIDE = ITEMS * 16 + 16;
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    if (g >= narr) return;
    McSortItem *items = (McSortItem *)(mc_smem + (size_t)threadIdx.x * STRIDE);
    const uint32_t a = off[g];
    const int n = (int)(off[g + 1] - a);
    for (int i = 0; i < n; i++) { items[i].k = keys[a + i]; items[i].i = (uint32_t)i; items[i].pad = 0; }
    if (heap) mc_heapsort_inl(items, (long)n, 0); else mc_std_sort_inl(items, (long)n, 0);
    for (int i = 0; i < n; i++) perm[a + i] = items[i].i;
}
template <int TPB, int ITEMS>
static void thread_sorts_set(const uint32_t *off, size_t narr, const double *keys, size_t nkeys, Sections &out)
{
    for (size_t b = 0; b < narr; b++) if (off[b + 1] - off[b] > (uint32_t)ITEMS) { fprintf(stderr, "thread_sorts: array %zu longer than %d\n", b, ITEMS); exit(2); }
    const size_t lds = mc_finish_lds(TPB, ITEMS);
    if (lds > 48 * 1024) CK(hipFuncSetAttribute((const void *)t_thread_sorts<TPB, ITEMS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Dev<double> d_keys(keys, nkeys);
    Dev<uint32_t> d_off(off, narr + 1);
    for (int heap = 0; heap < 2; heap++) {
        Dev<uint32_t> d_perm(nkeys, 0xFF);
        if (narr) { t_thread_sorts<TPB, ITEMS><<<dim3((unsigned)((narr + TPB - 1) / TPB)), dim3(TPB), lds>>>(d_keys, d_off, (uint32_t)narr, heap, d_perm); CK_LAUNCH(); }
        out.put(d_perm.host());
        std::vector<uint32_t> want;
        for (size_t b = 0; b < narr; b++) {
            const int n = (int)(off[b + 1] - off[b]);
            std::vector<McSortItem> x(n + 1);
            for (int i = 0; i < n; i++) { x[i].k = keys[off[b] + i]; x[i].i = (uint32_t)i; x[i].pad = 0; }
            if (heap) mc_heapsort(x.data(), (long)n, 0); else mc_std_sort(x.data(), (long)n, 0);
            for (int i = 0; i < n; i++) want.push_back(x[i].i);
        }
        out.put(want);
    }
}
static void case_thread_sorts(Sections &in, Sections &out)
{
    const uint32_t nsets = *in.take<uint32_t>();
    for (uint32_t q = 0; q < nsets; q++) {
        size_t no, nk;
        const uint32_t items = *in.take<uint32_t>();
        const uint32_t *off = in.take<uint32_t>(&no);
        const double *keys = in.take<double>(&nk);
        if (items == MC_FH_MIN) thread_sorts_set<32, MC_FH_MIN>(off, no - 1, keys, nk, out);
        else if (items == 16) thread_sorts_set<128, 16>(off, no - 1, keys, nk, out);
        else { fprintf(stderr, "thread_sorts: %u items per thread is none of k_finish's\n", items); exit(2); }
    }
}

// ---- c. mc_group_mergesort: m items in the first of k_order_heavy's two LDS buffers --------------------------------------------------
template <int NT, uint32_t CAP>
__global__ void __launch_bounds__(NT) t_mergesort(const uint64_t *__restrict__ in, const uint32_t *__restrict__ off, uint64_t *out)
{
    uint64_t *lds = (uint64_t *)mc_smem;
    const int tid = (int)threadIdx.x;
    const uint32_t a = off[blockIdx.x], m = off[blockIdx.x + 1] - a;
    for (uint32_t k = (uint32_t)tid; k < m; k += NT) lds[k] = in[a + k];
    mc_group_sync<NT>();
    const uint64_t *x = mc_group_mergesort<NT>(lds, lds + CAP, m, tid);
    for (uint32_t k = (uint32_t)tid; k < m; k += NT) out[a + k] = x[k];
}
template <int NT, uint32_t CAP>
static void mergesort_set(const uint32_t *off, size_t narr, const uint64_t *items, size_t nitems, Sections &out)
{
    for (size_t b = 0; b < narr; b++) {
        const uint32_t m = off[b + 1] - off[b];
        if (m < 64 || m > CAP || (m & (m - 1))) { fprintf(stderr, "mergesort: array %zu of %u items (a power of two from 64 to %u)\n", b, m, CAP); exit(2); }
    }
    const size_t lds = mc_order_heavy_lds(CAP);
    if (lds > 48 * 1024) CK(hipFuncSetAttribute((const void *)t_mergesort<NT, CAP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Dev<uint64_t> d_in(items, nitems), d_out(nitems, 0xFF);
    Dev<uint32_t> d_off(off, narr + 1);
    if (narr) { t_mergesort<NT, CAP><<<dim3((unsigned)narr), dim3(NT), lds>>>(d_in, d_off, d_out); CK_LAUNCH(); }
    out.put(d_out.host());
    std::vector<uint64_t> want(items, items + nitems);
    for (size_t b = 0; b < narr; b++) std::sort(want.begin() + off[b], want.begin() + off[b + 1]);
    out.put(want);
}
static void case_mergesort(Sections &in, Sections &out)
{
    const uint32_t nsets = *in.take<uint32_t>();
    for (uint32_t q = 0; q < nsets; q++) {
        size_t no, ni;
        const uint32_t cap = *in.take<uint32_t>();
        const uint32_t *off = in.take<uint32_t>(&no);
        const uint64_t *items = in.take<uint64_t>(&ni);
        if (cap == MC_ORDER_SMALL) mergesort_set<64, MC_ORDER_SMALL>(off, no - 1, items, ni, out);
        else if (cap == MC_ORDER_MID) mergesort_set<256, MC_ORDER_MID>(off, no - 1, items, ni, out);
        else if (cap == MC_ORDER_LDS) mergesort_set<1024, MC_ORDER_LDS>(off, no - 1, items, ni, out);
        else { fprintf(stderr, "mergesort: capacity %u is none of the library's\n", cap); exit(2); }
    }
}

// ---- d. the ordering step as stage C launches it, behind the binning: lists, the four ordering kernels, the copy -----------------
static void case_order(Sections &in, Sections &out)
{
    size_t npool, nslots, nh, nlow;
    const McHsp *pool = in.take<McHsp>(&npool);
    const uint32_t *slots = in.take<uint32_t>(&nslots);
    const uint32_t *heads = in.take<uint32_t>(&nh);
    const uint8_t *low = in.take<uint8_t>(&nlow);
    const uint32_t n = (uint32_t)nh - 1;
    if (nlow != n || heads[n] != nslots) { fprintf(stderr, "order: %zu marks for %u reads, %zu slots for segments of %u\n", nlow, n, nslots, heads[n]); exit(2); }
    std::vector<uint64_t> keys(nslots), places(nslots);
    for (size_t p = 0; p < nslots; p++) {
        if (slots[p] >= npool) { fprintf(stderr, "order: slot %u of a pool of %zu\n", slots[p], npool); exit(2); }
        const McHsp &h = pool[slots[p]];
        keys[p] = MC_HSP_KEY(h); places[p] = MC_HSP_PLACE(h);
    }
    for (uint32_t r = 0; r < n; r++) for (uint32_t p = heads[r]; p < heads[r + 1]; p++) if ((keys[p] >> 43) != r) { fprintf(stderr, "order: an HSP of read %llu in the segment of read %u\n", (unsigned long long)(keys[p] >> 43), r); exit(2); }
    Dev<McHsp> d_pool(pool, npool), d_v(nslots), d_tmp(2 * nslots);
    Dev<uint64_t> d_keys(keys.data(), nslots), d_places(places.data(), nslots);
    Dev<uint32_t> d_slots(slots, nslots), d_heads(heads, nh), d_counters((size_t)C_N), d_order(nslots, 0xFF), d_gsz(nslots), d_nv(n + 1), d_nrow(n + 1);
    Dev<uint32_t> heavy(n), heavy2(n), heavy3(n);
    Dev<uint8_t> d_low(low, n);
    McOrderBufs B = {};
    B.counters = d_counters; B.heads = d_heads; B.keys = d_keys; B.places = d_places; B.slots = d_slots; B.order = d_order;
    B.heavy = heavy; B.heavy2 = heavy2; B.heavy3 = heavy3; B.low = d_low; B.gsz = d_gsz; B.nv = d_nv; B.nrow = d_nrow;
    B.scratch = (uint64_t *)d_tmp.p; B.hsps = d_pool; B.v = d_v;
    Stream st, side, side2;                                         // the fork and the two joins as the library runs them: a stream of the step's own, two beside it
    Event fork, join, join2;
    CK_STAGE(mc_order_launch(B, n, st, McFork{side, side2, fork, join, join2}, false));
    out.put(d_v.host()); out.put(d_nv.host().data(), n); out.put(d_nrow.host().data(), n); out.put(d_counters.host());
    out.put(heavy.host()); out.put(heavy2.host()); out.put(heavy3.host());
    std::vector<McHsp> vexp(nslots + 1);
    std::vector<uint32_t> vn(n + 1);
    order_expected(pool, slots, heads, n, vexp.data(), vn.data());
    out.put(vexp.data(), nslots); out.put(vn.data(), n);
}

// ---- e. k_heap_lanes on heap words in the reads' scratch --------------------------------------------------------------------------
struct HeapWord { uint32_t w; };
inline bool mc_hless(const HeapWord &a, const HeapWord &b, int) { return (a.w >> 16) < (b.w >> 16); }
static size_t heavy_words_at(uint32_t a, uint32_t nseg) { return mc_heavy_words_at(a, (int)nseg) / 4; }   // mc_heavy_words, as a word offset into tmp
static void case_heap_lanes(Sections &in, Sections &out)
{
    const uint32_t nsets = *in.take<uint32_t>();
    const size_t lh = mc_heap_lanes_lds();
    CK(hipFuncSetAttribute((const void *)k_heap_lanes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lh));
    for (uint32_t q = 0; q < nsets; q++) {
        size_t nh, nr, nheavy, no, nw;
        const uint32_t *heads = in.take<uint32_t>(&nh);
        const uint32_t *nrow = in.take<uint32_t>(&nr);
        const uint32_t *heavy_first = in.take<uint32_t>(&nheavy);
        const uint32_t *order = in.take<uint32_t>(&no);
        const uint32_t *words = in.take<uint32_t>(&nw);          // the reads' words one after the other, nrow[s] of read s
        const uint32_t nheads = (uint32_t)nh - 1, total = heads[nheads];
        if (nr != nheads || no != nheavy) { fprintf(stderr, "heap_lanes: set %u: %zu row counts for %u reads, %zu places for %zu heavy reads\n", q, nr, nheads, no, nheavy); exit(2); }
        std::vector<uint32_t> tmp((size_t)total * 2 * sizeof(McHsp) / 4 + 4, 0u);
        size_t w0 = 0;
        for (uint32_t s = 0; s < nheads; s++) {
            const uint32_t a = heads[s], nseg = heads[s + 1] - a, n = nrow[s];
            // (the words lie behind the place of the rows: 4 n + 8 <= 24 nseg bytes whenever 0 < n <= nseg)
            if (n > nseg || n > MC_MAX_M8 || w0 + n > nw) { fprintf(stderr, "heap_lanes: set %u: read %u has %u rows in a segment of %u\n", q, s, n, nseg); exit(2); }
            for (uint32_t e = 0; e < n; e++) tmp[heavy_words_at(a, nseg) + 1 + e] = words[w0 + e];
            w0 += n;
        }
        for (size_t i = 0; i < nheavy; i++) if ((heavy_first[i] & 0x7FFFFFFFu) >= nheads || order[i] >= nheavy) { fprintf(stderr, "heap_lanes: set %u: entry %zu out of range\n", q, i); exit(2); }
        std::vector<uint32_t> counters(C_N, 0u);
        counters[C_HEAVY] = (uint32_t)nheavy;
        Dev<uint32_t> d_tmp(tmp.data(), tmp.size()), d_heads(heads, nh), d_nrow(nrow, nr), d_counters(counters.data(), counters.size()), d_hf(heavy_first, nheavy), d_order(order, nheavy);
        k_heap_lanes<<<dim3(MC_CUS), dim3(64), lh>>>(d_heads, nheads, total, (McHsp *)d_tmp.p, d_nrow, d_counters, d_hf, d_order);
        CK_LAUNCH();
        const std::vector<uint32_t> got = d_tmp.host();
        std::vector<uint32_t> dev, want;
        w0 = 0;
        for (uint32_t s = 0; s < nheads; s++) {
            const uint32_t a = heads[s], nseg = heads[s + 1] - a, n = nrow[s];
            std::vector<HeapWord> x(n + 1);
            for (uint32_t e = 0; e < n; e++) { dev.push_back(got[heavy_words_at(a, nseg) + 1 + e]); x[e].w = words[w0 + e]; }
            mc_heapsort(x.data(), (long)n, 0);
            for (uint32_t e = 0; e < n; e++) want.push_back(x[e].w);
            w0 += n;
        }
        out.put(dev); out.put(want);
    }
}

// ---- f. the counting sorts k_heavy_order and k_heap_order ------------------------------------------------------------------------
static void case_counting_sorts(Sections &in, Sections &out)
{
    const uint32_t nsets = *in.take<uint32_t>();
    for (uint32_t q = 0; q < nsets; q++) {
        const uint32_t *par = in.take<uint32_t>();                // kind (0: k_heavy_order, 1: k_heap_order), shift
        if (par[0] == 0) {
            size_t nl, nhv, nnv;
            const uint32_t *list = in.take<uint32_t>(&nl);
            const uint32_t *heavy = in.take<uint32_t>(&nhv);
            const uint32_t *nv = in.take<uint32_t>(&nnv);
            for (size_t i = 0; i < nl; i++) if (list[i] >= nhv || (heavy[list[i]] & 0x7FFFFFFFu) >= nnv) { fprintf(stderr, "counting_sorts: set %u: entry %zu out of range\n", q, i); exit(2); }
            const uint32_t cnt = (uint32_t)nl;
            Dev<uint32_t> d_list(list, nl), d_heavy(heavy, nhv), d_nv(nv, nnv), d_cnt(&cnt, 1), d_out(nl, 0xFF);
            k_heavy_order<<<dim3(1), dim3(1024)>>>(d_list, d_cnt, d_heavy, d_nv, (int)par[1], d_out);
            CK_LAUNCH();
            out.put(d_out.host());
        } else {
            size_t nhv, nnr;
            const uint32_t *heavy_first = in.take<uint32_t>(&nhv);
            const uint32_t *nrow = in.take<uint32_t>(&nnr);
            for (size_t i = 0; i < nhv; i++) if ((heavy_first[i] & 0x7FFFFFFFu) >= nnr) { fprintf(stderr, "counting_sorts: set %u: entry %zu out of range\n", q, i); exit(2); }
            std::vector<uint32_t> counters(C_N, 0u);
            counters[C_HEAVY] = (uint32_t)nhv;
            Dev<uint32_t> d_hf(heavy_first, nhv), d_nrow(nrow, nnr), d_counters(counters.data(), counters.size()), d_out(nhv, 0xFF);
            k_heap_order<<<dim3(1), dim3(1024)>>>(d_hf, d_nrow, d_counters, d_out);
            CK_LAUNCH();
            out.put(d_out.host());
        }
    }
}

// ---- g. k_bin_count, mc_scan_u32, k_bin_scatter as stage C chains them; the scan alone ----------------------------------------------
static void case_bins_and_scan(Sections &in, Sections &out)
{
    const uint32_t *nsets = in.take<uint32_t>();                  // bin sets, scan sets, refused scans
    for (uint32_t q = 0; q < nsets[0]; q++) {
        size_t nk, np, nc;
        const uint32_t *par = in.take<uint32_t>();                // reads, 1: with the cand filter
        const uint64_t *hkeys = in.take<uint64_t>(&nk);
        const uint64_t *hplace = in.take<uint64_t>(&np);
        const uint8_t *cand = in.take<uint8_t>(&nc);
        const uint32_t n = par[0];
        if (np != nk || nc != n) { fprintf(stderr, "bins: set %u: %zu place words for %zu keys, %zu marks for %u reads\n", q, np, nk, nc, n); exit(2); }
        for (size_t i = 0; i < nk; i++) if (hkeys[i] != ~0ull && (hkeys[i] >> 43) >= n) { fprintf(stderr, "bins: set %u: key %zu of a read past %u\n", q, i, n); exit(2); }
        std::vector<uint32_t> counters(C_N, 0u);
        counters[C_HSPS] = (uint32_t)nk;
        Dev<uint64_t> d_hkeys(hkeys, nk), d_hplace(hplace, nk), d_keys(nk, 0xFF), d_places(nk, 0xFF);
        Dev<uint32_t> d_counters(counters.data(), counters.size()), d_heads((size_t)n + 2), d_scan((size_t)n / MC_SCAN_BLK + 2), d_slots(nk, 0xFF);
        Dev<uint8_t> d_cand(cand, n);
        McOrderBufs B = {};
        B.hkeys = d_hkeys; B.hplace = d_hplace; B.cap_hsps = (uint32_t)nk; B.cand = par[1] ? d_cand.p : nullptr; B.counters = d_counters;
        B.heads = d_heads; B.scan = d_scan; B.keys = d_keys; B.places = d_places; B.slots = d_slots;
        uint32_t *cur = d_heads.p + 1;
        // (mc_bin_launch's three steps one by one: the counts and the starts are read between them)
        CK_STAGE(mc_bin_count_launch(B, nullptr));
        out.put(d_heads.host().data() + 1, n);
        if (mc_scan_u32(cur, n, cur, d_scan, nullptr)) { fprintf(stderr, "bins: set %u: %s\n", q, g_err.c_str()); exit(2); }
        CK_LAUNCH();
        out.put(d_heads.host().data() + 1, n);
        CK_STAGE(mc_bin_scatter_launch(B, nullptr));
        out.put(d_heads.host().data() + 1, n);
        out.put(d_keys.host()); out.put(d_places.host()); out.put(d_slots.host());
    }
    for (uint32_t q = 0; q < nsets[1]; q++) {
        size_t n;
        const uint32_t *par = in.take<uint32_t>();                // 1: in place
        const uint32_t *v = in.take<uint32_t>(&n);
        Dev<uint32_t> d_in(v, n), d_other(par[0] ? 0 : n, 0xFF), d_scan(n / MC_SCAN_BLK + 2);
        uint32_t *d_out = par[0] ? d_in.p : d_other.p;
        if (mc_scan_u32(d_in, (uint32_t)n, d_out, d_scan, nullptr)) { fprintf(stderr, "scan: set %u: %s\n", q, g_err.c_str()); exit(2); }
        CK_LAUNCH();
        out.put(par[0] ? d_in.host() : d_other.host());
    }
    for (uint32_t q = 0; q < nsets[2]; q++) {                        // refused on the host, before any launch: nothing is allocated for it
        const uint32_t n = *in.take<uint32_t>();
        Dev<uint32_t> d_none(1);
        g_err.clear();
        const int32_t rc = mc_scan_u32(d_none, n, d_none, d_none, nullptr);
        CK_LAUNCH();
        out.put(&rc, 1); out.put(g_err.data(), g_err.size());
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s CASE IN OUT\n", argv[0]); return 2; }
    const std::string name = argv[1];
    Sections in = sections_read(argv[2]), out;
    if (name == "adversary") {                                      // (host only)
        size_t nl;
        const int32_t *lens = in.take<int32_t>(&nl);
        for (size_t i = 0; i < nl; i++) out.put(wave_sort_adversary(lens[i]));
    } else if (name == "wave_sort") case_wave_sort(in, out);
    else if (name == "thread_sorts") case_thread_sorts(in, out);
    else if (name == "mergesort") case_mergesort(in, out);
    else if (name == "order") case_order(in, out);
    else if (name == "heap_lanes") case_heap_lanes(in, out);
    else if (name == "counting_sorts") case_counting_sorts(in, out);
    else if (name == "bins_and_scan") case_bins_and_scan(in, out);
    else { fprintf(stderr, "unknown case %s\n", name.c_str()); return 2; }
    sections_write(argv[3], out);
    printf("%s: %zu sections\n", name.c_str(), out.s.size());
    return 0;
}
