// k_wfit.h - the fit of the per-family weights (mc_fit_weights, mc_weights_mue): the candidate search mc_wfit.h states, one
// candidate per wave.
#pragma once
#include "mc_hip_common.h"
#include "mc_wfit.h"

// The table is tab[F + 2][N] float64: rows 0 .. F-1 the masked predictions pm[f][n], row F the truths, row F + 1 the keep bits of a
// library (a 64-bit word in the float64's place) - [f][n], so that a wave's lanes, one library each, read consecutive words.  A table of
// at most MC_WFIT_TAB_LDS bytes is staged in the block's LDS once and serves every candidate of the block's waves (150 x 30: 38,400
// bytes); a larger one is read where it lies (read-only, shared by every block: the L2's).  A wave makes its candidate's weights
// itself - lane f hashes w[f], and the sums take it from there with v_readlane, so the weights are scalars - and owns library
// n = 64 r + lane in round r.  The median is a selection on the errors' bit patterns (they are >= +0.0, so the patterns order as the
// values do): 63 steps, each fixing one bit of the k-th smallest pattern by counting the errors below a trial value with ballots.
// Integer comparisons alone, so neither the launch geometry nor any order of additions can move it.  Up to four rounds (N <= 256)
// the errors stay in registers; beyond that each wave keeps them in N words of LDS that only their own lane reads back.
// The block's best (mue, candidate), lower index among equals, goes to blockbest[block]; k_wfit_update - one block - reduces those
// with the same rule, moves w* or halves sigma, and writes the generation's trace row.  No atomics anywhere.
#define MC_WFIT_TAB_LDS 49152
#define MC_WFIT_LDS_MAX 65536
#define MC_WFIT_MAX_WAVES 8
#define MC_WFIT_REG_ROUNDS 4

struct McWfitState { double w[MC_WFIT_MAX_F]; double sigma, best; int32_t done, pad; };
struct McWfitPars { int32_t N, F, C, pad; uint32_t alive, pad2; uint64_t seed, L; };

struct McWfitLanes {                      // w(f): lane f's value, read as a scalar
    double v;
    __device__ double operator()(int f) const
    {
        const long long b = __double_as_longlong(v);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, f), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), f);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
};

__device__ __forceinline__ unsigned long long mc_wfit_wave_min(unsigned long long x)
{
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, d), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), d);
        const unsigned long long y = ((unsigned long long)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}

// mue of the wave's candidate (weights in W's lanes); err: the wave's N words of LDS when N > 64 x MC_WFIT_REG_ROUNDS.  Every lane returns it.
__device__ __forceinline__ double mc_wfit_wave_mue(const double *tab, int N, int F, const McWfitLanes &W, unsigned long long *err, int lane)
{
    const int rounds = (N + 63) >> 6;
    const bool in_regs = rounds <= MC_WFIT_REG_ROUNDS;
    unsigned long long x[MC_WFIT_REG_ROUNDS];
#pragma unroll
    for (int r = 0; r < MC_WFIT_REG_ROUNDS; r++) x[r] = ~0ull;                    // (no trial value reaches it)
    for (int r = 0; r < rounds; r++) {                                            // (every lane runs the sums - readlane needs lane f awake - on a library that exists)
        const int n = r * 64 + lane, nn = n < N ? n : N - 1;
        const uint32_t keep = (uint32_t)__double_as_longlong(tab[(size_t)(F + 1) * N + nn]);
        const double e = mc_wfit_error(tab + nn, (size_t)N, keep, tab[(size_t)F * N + nn], W, F);
        const unsigned long long b = n < N ? (unsigned long long)__double_as_longlong(e) : ~0ull;
        if (in_regs) {
#pragma unroll
            for (int q = 0; q < MC_WFIT_REG_ROUNDS; q++) if (q == r) x[q] = b;
        } else if (n < N) err[n] = b;
    }
    const int k = (N - 1) >> 1;                                                    // the lower middle, 0-based
    unsigned long long res = 0ull;
    for (int bit = 62; bit >= 0; bit--) {
        const unsigned long long trial = res | (1ull << bit);
        int cnt = 0;
        if (in_regs) {
#pragma unroll
            for (int q = 0; q < MC_WFIT_REG_ROUNDS; q++) cnt += __popcll(__ballot(x[q] < trial));
        } else {
            for (int r = 0; r < rounds; r++) { const int n = r * 64 + lane; cnt += __popcll(__ballot(n < N && err[n] < trial)); }
        }
        if (cnt <= k) res = trial;                                                 // the k-th smallest is not below trial
    }
    if (N & 1) return __longlong_as_double((long long)res);
    int le = 0;
    unsigned long long above = ~0ull;                                              // the smallest error above res
    if (in_regs) {
#pragma unroll
        for (int q = 0; q < MC_WFIT_REG_ROUNDS; q++) { le += __popcll(__ballot(x[q] <= res)); if (x[q] > res && x[q] < above) above = x[q]; }
    } else {
        for (int r = 0; r < rounds; r++) {
            const int n = r * 64 + lane;
            const unsigned long long v = n < N ? err[n] : ~0ull;
            le += __popcll(__ballot(v <= res));
            if (v > res && v < above) above = v;
        }
    }
    const unsigned long long hi = le >= k + 2 ? res : mc_wfit_wave_min(above);
    return mc_wfit_mid(__longlong_as_double((long long)res), __longlong_as_double((long long)hi));
}

// gen >= 0: generation gen of a search (candidates around S->w);  gen < 0: candidate 0 alone, the start.  wgiven: the candidates are
// the caller's vectors wgiven[C][F] and every mue goes to out_mue[C] (mc_weights_mue).  Dynamic LDS: the table if TAB_LDS, then err_words
// words per wave, then two words per wave for the block's best.
template <bool TAB_LDS>
__global__ void __launch_bounds__(MC_WFIT_MAX_WAVES * 64) k_wfit_eval(McWfitPars P, const double *__restrict__ gtab, const McWfitState *__restrict__ S, int32_t gen, int32_t err_words,
                                                                       const double *__restrict__ wgiven, double *__restrict__ out_mue, unsigned long long *__restrict__ blockbest)
{
    double *lds = (double *)mc_smem;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, waves = (int)blockDim.x >> 6;
    const int N = P.N, F = P.F;
    if (!wgiven && gen >= 0 && S->done) return;                                    // the search has ended (the same answer in every block)
    const size_t tab_words = TAB_LDS ? (size_t)(F + 2) * N : 0;
    if (TAB_LDS) {
        for (size_t i = threadIdx.x; i < tab_words; i += blockDim.x) lds[i] = gtab[i];
        __syncthreads();
    }
    const double *tab = TAB_LDS ? lds : gtab;
    unsigned long long *err = (unsigned long long *)(lds + tab_words) + (size_t)wave * err_words;
    unsigned long long *bb = (unsigned long long *)(lds + tab_words) + (size_t)waves * err_words;
    const double sigma = wgiven ? 0.0 : S->sigma;
    const double wstar = !wgiven && lane < F ? S->w[lane] : 0.0;
    unsigned long long best = ~0ull, bestc = ~0ull;
    for (int64_t c = (int64_t)blockIdx.x * waves + wave; c < P.C; c += (int64_t)gridDim.x * waves) {
        McWfitLanes W;
        W.v = 0.0;
        if (lane < F) {
            if (wgiven) W.v = wgiven[(size_t)c * F + lane];
            else W.v = c == 0 ? wstar : mc_wfit_move(wstar, sigma, mc_wfit_d_of_key(mc_wfit_key(P.seed, P.L, (uint64_t)gen, (uint64_t)c), lane), (P.alive >> lane) & 1u);
        }
        const double m = mc_wfit_wave_mue(tab, N, F, W, err, lane);
        const unsigned long long mb = (unsigned long long)__double_as_longlong(m);
        if (wgiven) { if (lane == 0) out_mue[c] = m; }
        else if (mb < best) { best = mb; bestc = (unsigned long long)c; }           // (a wave's candidates ascend: the first of equals stays)
    }
    if (wgiven) return;
    if (lane == 0) { bb[2 * wave] = best; bb[2 * wave + 1] = bestc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < waves; v++) {
            const unsigned long long m = bb[2 * v], c = bb[2 * v + 1];
            if (m < best || (m == best && c < bestc)) { best = m; bestc = c; }
        }
        blockbest[2 * (size_t)blockIdx.x] = best;
        blockbest[2 * (size_t)blockIdx.x + 1] = bestc;
    }
}

// one block: the winner of the generation among the blocks' bests, then w*, sigma and the trace row (mc_wfit.h, "the search")
__global__ void __launch_bounds__(256) k_wfit_update(McWfitPars P, McWfitState *__restrict__ S, int32_t gen, int32_t nblocks, const unsigned long long *__restrict__ blockbest,
                                                     double *__restrict__ trace)
{
    __shared__ unsigned long long sm[256], sc[256];
    const int t = (int)threadIdx.x;
    double *row = trace + 3 * (size_t)(gen + 1);
    const double sigma = S->sigma, best = S->best;
    const double wold = t < P.F ? S->w[t] : 0.0;
    if (gen >= 0 && S->done) {
        if (t == 0) { row[0] = best; row[1] = -1.0; row[2] = sigma; }
        return;
    }
    unsigned long long m = ~0ull, c = ~0ull;
    for (int i = t; i < nblocks; i += 256) {
        const unsigned long long mm = blockbest[2 * (size_t)i], cc = blockbest[2 * (size_t)i + 1];
        if (mm < m || (mm == m && cc < c)) { m = mm; c = cc; }
    }
    sm[t] = m; sc[t] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const unsigned long long mm = sm[t + s], cc = sc[t + s];
            if (mm < sm[t] || (mm == sm[t] && cc < sc[t])) { sm[t] = mm; sc[t] = cc; }
        }
        __syncthreads();
    }
    m = sm[0]; c = sc[0];
    const double wm = __longlong_as_double((long long)m);
    __syncthreads();                                                               // (every thread has read the state)
    if (gen < 0) {
        if (t == 0) { S->best = wm; row[0] = wm; row[1] = 0.0; row[2] = sigma; }
        return;
    }
    const bool better = wm < best;
    if (better && c > 0 && t < P.F) S->w[t] = mc_wfit_move(wold, sigma, mc_wfit_d_of_key(mc_wfit_key(P.seed, P.L, (uint64_t)gen, (uint64_t)c), t), (P.alive >> t) & 1u);
    if (t == 0) {
        const double ns = better ? sigma : sigma * 0.5;
        S->best = better ? wm : best;
        S->sigma = ns;
        if (ns < MC_WFIT_SIGMA_MIN) S->done = 1;
        row[0] = better ? wm : best; row[1] = (double)c; row[2] = ns;
    }
}
