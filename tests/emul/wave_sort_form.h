// tests/emul/wave_sort_form.h - the formulation of mc_wave_std_sort (csrc/k_finish.h) in plain C++, the 64 lanes flattened into loops:
// what the comment above the kernel function states, written out so that it can be held to mc_std_sort (mc_sort_impl.h, the
// move-for-move statement of libstdc++'s std::sort) on the CPU.  Step by step the kernel's:
//  * the stop lists of __unguarded_partition - A: the positions whose element is not < pivot, ascending; B: those whose element
//    is not > pivot, descending;
//  * K = the number of k with A_k < B_k, counted in rounds of 64 with the kernel's early exit (a round that is not full of them ends it);
//  * all K swaps at once; the cut `split` from A_K and B_(K-1);
//  * the recursion on a stack of 64 (first, last, depth) entries - the kernel's has no guard, this one reports an overflow -, ranges
//    of <= 16 left alone, mc_heapsort at depth 0 (counted: how often, and the largest range);
//  * the final placement: position - (larger keys among the 15 before) + (smaller keys among the 15 behind), 64 at a time with
//    the next 64 read before anything of a round is written.
// And McIlroy's adversary ("A killer adversary for quicksort", 1999) played against mc_std_sort itself: the keys it freezes are an
// input on which that sort - and so this formulation and the kernel - runs out of depth and takes the heap-sort fallback.
#pragma once
#include <stdint.h>
#include <vector>
#include "mc_finish.h"

struct WaveSortStats { long fallbacks = 0, largest = 0, overflow = 0; };

inline void wave_sort_form(McSortItem *items, int n, WaveSortStats &st)
{
    if (n <= 1) return;
    std::vector<uint16_t> posA(n + 2), posB(n + 2), npos(n + 2);
    int stk[3 * 64];
    int lg = 0;
    for (int t = n; t > 1; t >>= 1) lg++;
    int sp = 1;
    stk[0] = 0; stk[1] = n; stk[2] = 2 * lg;
    while (sp > 0) {
        sp--;
        int f = stk[3 * sp], l = stk[3 * sp + 1], depth = stk[3 * sp + 2];
        while (l - f > 16) {
            if (depth == 0) {
                mc_heapsort(items + f, (long)(l - f), 0);
                st.fallbacks++;
                if (l - f > st.largest) st.largest = l - f;
                break;
            }
            --depth;
            const double x = items[f].k, y = items[f + (l - f) / 2].k, z = items[l - 1].k;
            double p;
            if (x < y) { if (y < z) p = y; else if (x < z) p = z; else p = x; }
            else if (x < z) p = x;
            else if (y < z) p = z;
            else p = y;
            int nA = 0, nB = 0;
            for (int i = f; i < l; i++) if (!(items[i].k < p)) posA[nA++] = (uint16_t)i;
            for (int i = l - 1; i >= f; i--) if (!(p < items[i].k)) posB[nB++] = (uint16_t)i;
            const int mn = nA < nB ? nA : nB;
            int K = 0;
            for (int k0 = 0; k0 < mn; k0 += 64) {
                int cnt = 0;
                for (int lane = 0; lane < 64; lane++) { const int k = k0 + lane; if (k < mn && posA[k] < posB[k]) cnt++; }
                K += cnt;
                if (cnt != 64) break;
            }
            for (int k0 = 0; k0 < K; k0 += 64) {                    // a round's lanes read both elements, then write them
                McSortItem t1[64], t2[64];
                for (int lane = 0; lane < 64 && k0 + lane < K; lane++) { t1[lane] = items[posA[k0 + lane]]; t2[lane] = items[posB[k0 + lane]]; }
                for (int lane = 0; lane < 64 && k0 + lane < K; lane++) { items[posA[k0 + lane]] = t2[lane]; items[posB[k0 + lane]] = t1[lane]; }
            }
            int split;
            if (K == 0) split = posA[0];
            else if (K < nA) { const int a = posA[K], b = posB[K - 1]; split = a < b ? a : b; }
            else split = posB[K - 1];
            if (sp >= 64) { st.overflow++; return; }
            stk[3 * sp] = split; stk[3 * sp + 1] = l; stk[3 * sp + 2] = depth;
            sp++;
            l = split;
        }
    }
    for (int x = 0; x < n; x++) {
        const double kx = items[x].k;
        int np = x;
        const int y0 = x - 15 > 0 ? x - 15 : 0, y1 = x + 15 < n - 1 ? x + 15 : n - 1;
        for (int yy = y0; yy < x; yy++) np -= (items[yy].k > kx) ? 1 : 0;
        for (int yy = x + 1; yy <= y1; yy++) np += (items[yy].k < kx) ? 1 : 0;
        npos[x] = (uint16_t)np;
    }
    McSortItem cur[64], nxt[64];
    for (int lane = 0; lane < 64; lane++) cur[lane] = items[lane < n ? lane : 0];
    for (int c0 = 0; c0 < n; c0 += 64) {
        for (int lane = 0; lane < 64; lane++) { const int nx = c0 + 64 + lane; nxt[lane] = items[nx < n ? nx : 0]; }
        for (int lane = 0; lane < 64; lane++) if (c0 + lane < n) items[npos[c0 + lane]] = cur[lane];
        for (int lane = 0; lane < 64; lane++) cur[lane] = nxt[lane];
    }
}

// ---- McIlroy's adversary against mc_std_sort ---------------------------------------------------------------------------------------
// The sort moves handles; a comparison of two handles whose keys are both still "gas" freezes one of them at the next solid value -
// the one the sort has been comparing everything with (its pivot), so that the pivot always ends among the smallest of its range.
struct AdvItem { int idx; };
struct AdvState { std::vector<int> val; int nsolid, cand, gas; };
inline AdvState *&adv_state() { static AdvState *s = nullptr; return s; }
inline bool mc_hless(const AdvItem &a, const AdvItem &b, int)
{
    AdvState &S = *adv_state();
    const int x = a.idx, y = b.idx;
    if (S.val[x] == S.gas && S.val[y] == S.gas) { if (x == S.cand) S.val[x] = S.nsolid++; else S.val[y] = S.nsolid++; }
    if (S.val[x] == S.gas) S.cand = x;
    else if (S.val[y] == S.gas) S.cand = y;
    return S.val[x] < S.val[y];
}
inline std::vector<double> wave_sort_adversary(int n)
{
    AdvState S;
    S.val.assign(n, n); S.nsolid = 0; S.cand = 0; S.gas = n;
    std::vector<AdvItem> h(n);
    for (int i = 0; i < n; i++) h[i].idx = i;
    adv_state() = &S;
    mc_std_sort(h.data(), (long)n, 0);
    adv_state() = nullptr;
    return std::vector<double>(S.val.begin(), S.val.end());
}
