// tests/emul/wave_sort_form.cpp - the CPU driver of tests/test_order_host.py (g++, no GPU):
//   check N          wave_sort_form (wave_sort_form.h: mc_wave_std_sort's formulation) against mc_std_sort on N generated arrays
//                    (constant, 2 / 5 / 50 distinct keys, distinct, sorted, reversed, organ pipe; n up to 6144) and on McIlroy's
//                    adversary for every length the device test uses; prints the counts
//   adversary IN OUT the adversary's frozen keys for the lengths in IN (section 0: int32 lengths) - one section of doubles per length
//   waves IN OUT     the arrays of the device test's wave_sort case: per set mc_std_sort's permutation, the formulation's, and per
//                    array (fallbacks, largest fallback range, stack overflows)
//   stacks IN OUT    the device test's order case: mc_build_stacks on every read's sorted records (order_expect.h)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "order_io.h"
#include "wave_sort_form.h"
#include "order_expect.h"

static bool one_array(const std::vector<double> &keys, WaveSortStats &st, std::vector<uint32_t> *want_out = nullptr, std::vector<uint32_t> *got_out = nullptr)
{
    const int n = (int)keys.size();
    std::vector<McSortItem> a(n + 1), b(n + 1);
    for (int i = 0; i < n; i++) { a[i].k = keys[i]; a[i].i = (uint32_t)i; a[i].pad = 0; b[i] = a[i]; }
    mc_std_sort(a.data(), (long)n, 0);
    wave_sort_form(b.data(), n, st);
    bool same = true;
    for (int i = 0; i < n; i++) same = same && a[i].i == b[i].i && a[i].k == b[i].k;
    if (want_out) for (int i = 0; i < n; i++) want_out->push_back(a[i].i);
    if (got_out) for (int i = 0; i < n; i++) got_out->push_back(b[i].i);
    return same;
}
static int check(long narrays)
{
    static const int lens[] = {0, 1, 2, 15, 16, 17, 18, 32, 33, 63, 64, 65, 127, 128, 129, 500, 511, 512, 513, 1279, 1280, 1281, 4096, 6143, 6144};
    uint64_t s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); };
    long bad = 0, total = 0, adv_bad = 0, adv_total = 0, adv_nofall = 0;
    WaveSortStats st, adv;
    for (long it = 0; it < narrays; it++) {
        const int n = it % 100 == 0 ? (int)(rnd() % 6145) : it % 10 == 0 ? (int)(rnd() % 1300) : (int)(rnd() % 200);
        const int kind = (int)(it % 8);
        std::vector<double> k(n);
        for (int i = 0; i < n; i++) {
            switch (kind) {
            case 0: k[i] = -3.5; break;
            case 1: k[i] = (double)(rnd() % 2); break;
            case 2: k[i] = (double)(rnd() % 5); break;
            case 3: k[i] = (double)(rnd() % 50); break;
            case 4: k[i] = (double)rnd() + 1e-3 * i; break;
            case 5: k[i] = (double)i; break;
            case 6: k[i] = (double)(n - i); break;
            default: k[i] = (double)(i < n / 2 ? i : n - 1 - i); break;
            }
        }
        total++;
        if (!one_array(k, st)) bad++;
    }
    for (int n : lens) {
        WaveSortStats one;
        adv_total++;
        if (!one_array(wave_sort_adversary(n), one)) adv_bad++;
        if (n >= 64 && one.fallbacks == 0) adv_nofall++;
        adv.fallbacks += one.fallbacks; adv.overflow += one.overflow;
        if (one.largest > adv.largest) adv.largest = one.largest;
    }
    printf("arrays %ld differ %ld overflow %ld fallbacks %ld largest %ld adversary_arrays %ld adversary_differ %ld adversary_overflow %ld adversary_fallbacks %ld adversary_largest %ld adversary_ge64_without_fallback %ld\n",
           total, bad, st.overflow, st.fallbacks, st.largest, adv_total, adv_bad, adv.overflow, adv.fallbacks, adv.largest, adv_nofall);
    return (bad || adv_bad || st.overflow || adv.overflow) ? 1 : 0;
}
int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "check" && argc == 3) return check(atol(argv[2]));
    if (argc != 4) { fprintf(stderr, "usage: %s check N | adversary IN OUT | waves IN OUT | stacks IN OUT\n", argv[0]); return 2; }
    Sections in = sections_read(argv[2]), out;
    if (mode == "adversary") {
        size_t nl;
        const int32_t *lens = in.take<int32_t>(&nl);
        for (size_t i = 0; i < nl; i++) out.put(wave_sort_adversary(lens[i]));
    } else if (mode == "waves") {
        const uint32_t nsets = *in.take<uint32_t>();
        for (uint32_t q = 0; q < nsets; q++) {
            size_t no, nk;
            in.take<uint32_t>();                                    // (the set's MAXN: the device's business)
            const uint32_t *off = in.take<uint32_t>(&no);
            const double *keys = in.take<double>(&nk);
            std::vector<uint32_t> want, got;
            std::vector<int32_t> stats;
            for (size_t b = 0; b + 1 < no; b++) {
                WaveSortStats st;
                one_array(std::vector<double>(keys + off[b], keys + off[b + 1]), st, &want, &got);
                stats.push_back((int32_t)st.fallbacks); stats.push_back((int32_t)st.largest); stats.push_back((int32_t)st.overflow);
            }
            out.put(want); out.put(got); out.put(stats);
        }
    } else if (mode == "stacks") {
        size_t npool, nslots, nh;
        const McHsp *pool = in.take<McHsp>(&npool);
        const uint32_t *slots = in.take<uint32_t>(&nslots);
        const uint32_t *heads = in.take<uint32_t>(&nh);
        const uint32_t nreads = (uint32_t)nh - 1;
        std::vector<McHsp> vexp(nslots + 1);
        std::vector<uint32_t> vn(nreads + 1);
        order_expected(pool, slots, heads, nreads, vexp.data(), vn.data());
        out.put(vexp.data(), nslots); out.put(vn.data(), nreads);
    } else { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
    sections_write(argv[3], out);
    return 0;
}
