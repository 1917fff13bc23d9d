// mc_boot.h - the Poisson bootstrap over the sampled reads: the weight of one read in one replicate, a pure function of
// (seed, replicate b, global read id r).  Host and device code alike: k_bootstrap.h runs it one replicate per lane,
// tests/emul/boot_weights.cpp compiles it with g++, and the tests' numpy statement reads the threshold table out of this file.
// No HIP include here (see mc_simlib.h, whose mc_mix64 and MC_SIM_HD this uses).
//
//     key(seed, b) = mix(mix(seed ^ mix(b)) ^ MC_BOOT_KEY)              (the bootstrap's own key domain, as MC_SIM_EKEY is the error process's)
//     u            = mix(key(seed, b) + r)                               (64-bit, wrapping; r = mc_best_hit.read, never negative)
//     w(b, r)      = the number of k in 0 .. MC_BOOT_K - 1 with u >= MC_BOOT_THR[k]
// MC_BOOT_THR[k] = floor(2^64 x P[X <= k]) for X ~ Poisson(1), so w is X by inverse CDF with every value above MC_BOOT_K counted
// as MC_BOOT_K: that folded tail is P[X > 19] = 1.59e-19 < 2^-60 (19 is the smallest K for which it is).  Integer comparisons
// alone decide a weight, so every compiler and numpy's uint64 arithmetic give the same one.
//
// Per replicate b and family f, over the best hits (read, family, aln, target_len) - aln_stat as pars.map gives it to aggregate_hits:
//     hits:  S[b, f] = sum of w(b, read)                                   int64, exact
//     aln:   S[b, f] = sum of w(b, read) x aln                             int64, exact
//     cov:   S[b, f] = sum of (double)w(b, read) x ((double)aln / (double)target_len)   float64; each term rounded as written, the
//            order of the additions is the implementation's (the terms are positive: any order lies within (terms - 1) x 2^-53 of the exact sum)
// and W[b] = sum of w(b, read) over all best hits: the classified reads the replicate drew.
#pragma once
#include "mc_simlib.h"

#define MC_BOOT_KEY 0xE7037ED1A0B428DBull
#define MC_BOOT_K 19
enum { MC_BOOT_HITS = 0, MC_BOOT_COV = 1, MC_BOOT_ALN = 2 };        // aln_stat, numbered as mc_set_run() takes it

// floor(2^64 x sum_{j <= k} e^-1 / j!), k = 0 .. 18 (tests/test_bootstrap_host.py checks them against exact rational arithmetic)
static constexpr uint64_t MC_BOOT_THR[MC_BOOT_K] = {
    0x5E2D58D8B3BCDF1Aull, 0xBC5AB1B16779BE35ull, 0xEB715E1DC1582DC2ull, 0xFB23979734A252F1ull, 0xFF1025F59174DC3Dull, 0xFFD90F3BA4055E19ull, 0xFFFA8B71FC72C913ull,
    0xFFFF540C0914B3C9ull, 0xFFFFED1F4AA8F120ull, 0xFFFFFE216E641462ull, 0xFFFFFFD4D85D3183ull, 0xFFFFFFFC6DA262B4ull, 0xFFFFFFFFBA12D178ull, 0xFFFFFFFFFB07C64Cull,
    0xFFFFFFFFFFAB8EA5ull, 0xFFFFFFFFFFFABE22ull, 0xFFFFFFFFFFFFB11Aull, 0xFFFFFFFFFFFFFBA1ull, 0xFFFFFFFFFFFFFFC5ull};

MC_SIM_HD uint64_t mc_boot_key(uint64_t seed, uint64_t b) { return mc_mix64(mc_mix64(seed ^ mc_mix64(b)) ^ MC_BOOT_KEY); }

MC_SIM_HD int mc_boot_weight(uint64_t key, uint64_t r)
{
    const uint64_t u = mc_mix64(key + r);
    int w = 0;
    while (w < MC_BOOT_K && u >= MC_BOOT_THR[w]) w++;
    return w;
}
