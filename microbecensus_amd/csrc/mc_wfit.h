// mc_wfit.h - the fit of the per-family weights (TRAINING.txt step 5, optimize_weights.R) restated as a deterministic candidate
// search.  Host and device code alike: k_wfit.h runs it one candidate per wave, tests/emul/wfit.cpp compiles it with g++
// (-ffp-contract=off), tests/wfit_restated.py restates it in numpy and reads the constants out of this file.  No HIP include here (see
// mc_simlib.h, whose mc_mix64 and MC_SIM_HD this uses).  Every product, sum and quotient below is one IEEE float64 operation rounded
// on its own: nothing may be contracted into an FMA.
//
// Per read length L: N libraries, F families, pred[n][f] (NaN = "NA": the family's rate was 0 in that library), truth[n] > 0.
//
// The mask (never changes during a fit; it does not depend on the weights).  Over the valid (non-NaN) predictions v of library n:
//     centre = median(v);  spread = 1.48 x median(|v - centre|);  keep[n][f] = pred[n][f] is a number and |pred[n][f] - centre| < spread
// median of k sorted values: the middle one, or (lo + hi) x 0.5 for even k - microbe_census.py's median and mad, the cut
// _ags_of_sums applies (strict <; R's mad() would use 1.4826).  pm[n][f] = pred[n][f] where kept, 0.0 elsewhere.
//
// The error of library n under weights w (all in [0, 1]), f ascending, both sums started at 0.0:
//     num = sum_f  w[f] x pm[n][f]                den = sum_f (keep[n][f] ? w[f] : 0.0)
//     err = den == 0 ? +inf : |truth[n] - num / den| / truth[n]
// (Adding the +0.0 of a family that is not kept leaves a sum as it was - a sum that starts at +0.0 is never -0.0 - so this is the sum
// over the kept families alone, which is what _ags_of_sums computes.)
//     mue(w) = median over n of err                (of the N errors sorted; +inf sorts last)
//
// The candidates.  key domain MC_WFIT_KEY, as MC_BOOT_KEY is the bootstrap's:
//     k(seed, L, g, c) = mix(mix(mix(mix(seed ^ mix(L)) ^ MC_WFIT_KEY) + g) + c)          (64-bit, wrapping)
//     m = mix(k);  u = mix(k + 1 + f);  x = (double)(u >> 11) x 2^-52 - 1.0                (exact steps: x is uniform on [-1, 1))
//     mode = m & 3:   0  every coordinate moves
//                     1  coordinate f moves if (u & 3) == 0                                (one in four)
//                     2, 3  coordinate (m >> 8) & 31 moves, no other                       (none if that is >= F)
//     d(seed, L, g, c, f) = x where f moves, 0.0 where it does not
//     candidate 0 = w*;  candidate c > 0:  w[f] = alive[f] ? clamp(w*[f] + sigma x d, 0, 1) : w*[f]
// alive[f]: the family is kept in at least one library.  sigma is a power of two, so sigma x d is exact.
//
// The search:  w* = 1 / F each, sigma = MC_WFIT_SIGMA0, best = mue(w*), trace[0] = (best, 0, sigma).  Generation g = 0 .. G - 1:
//     sigma < MC_WFIT_SIGMA_MIN: the search has ended;  trace[g + 1] = (best, -1, sigma)
//     else the winner is the candidate c of 0 .. C - 1 with the lowest mue, the lowest index among equals;
//          mue(c) < best:  w* = candidate c, best = mue(c);   otherwise sigma = sigma x 0.5;    trace[g + 1] = (best, c, sigma)
#pragma once
#include <math.h>
#include "mc_simlib.h"
#include <algorithm>
#include <vector>

#define MC_WFIT_KEY 0xC2B2AE3D27D4EB4Full
#define MC_WFIT_MAX_F 32
#define MC_WFIT_MAX_N 4096
#define MC_WFIT_MAX_C 65536
#define MC_WFIT_MAX_G 4096
#define MC_WFIT_C 4096                      // the defaults: DESIGN.md section 11 says what was tried
#define MC_WFIT_G 192
#define MC_WFIT_SIGMA0 0.25                 // 2^-2
#define MC_WFIT_SIGMA_MIN 9.5367431640625e-07   // 2^-20
#define MC_WFIT_MAD_CONST 1.48

MC_SIM_HD uint64_t mc_wfit_key(uint64_t seed, uint64_t L, uint64_t g, uint64_t c)
{
    return mc_mix64(mc_mix64(mc_mix64(mc_mix64(seed ^ mc_mix64(L)) ^ MC_WFIT_KEY) + g) + c);
}

// d of the candidate whose key is k, for family f
MC_SIM_HD double mc_wfit_d_of_key(uint64_t k, int f)
{
    const uint64_t m = mc_mix64(k);
    const uint64_t u = mc_mix64(k + 1ull + (uint64_t)f);
    const int mode = (int)(m & 3ull);
    const bool moves = mode == 0 ? true : mode == 1 ? (u & 3ull) == 0ull : (int)((m >> 8) & 31ull) == f;
    const double x = (double)(int64_t)(u >> 11) * 2.220446049250313e-16 - 1.0;      // 2^-52
    return moves ? x : 0.0;
}

MC_SIM_HD double mc_wfit_d(uint64_t seed, uint64_t L, uint64_t g, uint64_t c, int f) { return mc_wfit_d_of_key(mc_wfit_key(seed, L, g, c), f); }

// one weight of a candidate c > 0
MC_SIM_HD double mc_wfit_move(double w, double sigma, double d, bool alive)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!alive) return w;
    const double s = sigma * d;
    const double v = w + s;
    return v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
}

// the error of one library: pm[f x stride] its masked predictions, keep its kept families (bit f), w(f) the weights - an array
// on the host (McWfitArray), the lanes of a wave on the device (k_wfit.h)
struct McWfitArray {
    const double *w;
    MC_SIM_HD double operator()(int f) const { return w[f]; }
};

template <class Weights>
MC_SIM_HD double mc_wfit_error(const double *pm, size_t stride, uint32_t keep, double truth, const Weights &w, int F)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double num = 0.0, den = 0.0;
    for (int f = 0; f < F; f++) {
        const double wf = w(f);
        const double t = wf * pm[(size_t)f * stride];
        num = num + t;
        den = den + (((keep >> f) & 1u) ? wf : 0.0);
    }
    if (den == 0.0) return __builtin_huge_val();
    const double est = num / den;
    return fabs(truth - est) / truth;
}

MC_SIM_HD double mc_wfit_mid(double lo, double hi) { return (lo + hi) * 0.5; }

// ---- host side: the mask, mue and the whole search as the statement above gives them (the library makes the mask with these; the
// tests' driver runs all of it) ------------------------------------------------------------------------------------------------------
inline double mc_wfit_median(std::vector<double> v)                 // of non-NaN values; NaN for none
{
    if (v.empty()) return __builtin_nan("");
    std::sort(v.begin(), v.end());
    const size_t k = v.size();
    return (k & 1) ? v[k / 2] : mc_wfit_mid(v[k / 2 - 1], v[k / 2]);
}

// pred[N][F] -> pm[N][F], keep[N]; returns alive
inline uint32_t mc_wfit_mask(const double *pred, int N, int F, double *pm, uint32_t *keep)
{
    uint32_t alive = 0;
    std::vector<double> v, dev;
    for (int n = 0; n < N; n++) {
        v.clear(); dev.clear();
        for (int f = 0; f < F; f++) if (pred[(size_t)n * F + f] == pred[(size_t)n * F + f]) v.push_back(pred[(size_t)n * F + f]);
        const double centre = mc_wfit_median(v);
        for (double x : v) dev.push_back(fabs(x - centre));
        const double spread = MC_WFIT_MAD_CONST * mc_wfit_median(dev);
        uint32_t k = 0;
        for (int f = 0; f < F; f++) {
            const double p = pred[(size_t)n * F + f];
            const bool kept = p == p && fabs(p - centre) < spread;
            pm[(size_t)n * F + f] = kept ? p : 0.0;
            if (kept) k |= 1u << f;
        }
        keep[n] = k;
        alive |= k;
    }
    return alive;
}

inline double mc_wfit_mue(const double *pm, const uint32_t *keep, const double *truth, int N, int F, const double *w, double *errs = nullptr)
{
    std::vector<double> e((size_t)N);
    for (int n = 0; n < N; n++) e[n] = mc_wfit_error(pm + (size_t)n * F, 1, keep[n], truth[n], McWfitArray{w}, F);
    if (errs) std::copy(e.begin(), e.end(), errs);
    return mc_wfit_median(e);
}

inline void mc_wfit_candidate(const double *wstar, double sigma, uint32_t alive, uint64_t seed, uint64_t L, uint64_t g, uint64_t c, int F, double *w)
{
    const uint64_t k = mc_wfit_key(seed, L, g, c);
    for (int f = 0; f < F; f++) w[f] = c == 0 ? wstar[f] : mc_wfit_move(wstar[f], sigma, mc_wfit_d_of_key(k, f), (alive >> f) & 1u);
}

// weights[F], trace[G + 1][3]
inline void mc_wfit_fit(const double *pred, const double *truth, int N, int F, uint64_t seed, uint64_t L, int C, int G, double *weights, double *trace)
{
    std::vector<double> pm((size_t)N * F), w(F), cand(F);
    std::vector<uint32_t> keep(N);
    const uint32_t alive = mc_wfit_mask(pred, N, F, pm.data(), keep.data());
    for (int f = 0; f < F; f++) w[f] = 1.0 / (double)F;
    double sigma = MC_WFIT_SIGMA0, best = mc_wfit_mue(pm.data(), keep.data(), truth, N, F, w.data());
    trace[0] = best; trace[1] = 0.0; trace[2] = sigma;
    for (int g = 0; g < G; g++) {
        double *row = trace + 3 * (size_t)(g + 1);
        if (sigma < MC_WFIT_SIGMA_MIN) { row[0] = best; row[1] = -1.0; row[2] = sigma; continue; }
        double wm = 0.0; int wc = -1;
        for (int c = 0; c < C; c++) {
            mc_wfit_candidate(w.data(), sigma, alive, seed, L, (uint64_t)g, (uint64_t)c, F, cand.data());
            const double m = mc_wfit_mue(pm.data(), keep.data(), truth, N, F, cand.data());
            if (wc < 0 || m < wm) { wm = m; wc = c; }
        }
        if (wm < best) { mc_wfit_candidate(w.data(), sigma, alive, seed, L, (uint64_t)g, (uint64_t)wc, F, cand.data()); w = cand; best = wm; }
        else sigma = sigma * 0.5;
        row[0] = best; row[1] = (double)wc; row[2] = sigma;
    }
    for (int f = 0; f < F; f++) weights[f] = w[f];
}
