// seg_narrow - the one-word form of the SEG masking (mc_seg_mask_fx2<McBits64>, csrc/mc_core.h: what a lane of the narrow k_translate_seg
// restates, for frames of at most MC_NARROW_MAXAA = 63 residues) beside the three-word form, and the McBits64 primitives against
// McBits192.  tests/test_seg_narrow_host.py holds the frames to the oracle's rs_translate6().
//
//   seg_narrow frames READS L OUT   READS: n x L bytes of bases, 18 <= L <= 191.  OUT: per read, per form (0 McBits192 with a work list of
//                                   MC_SEG_STK entries, 1 McBits64 with one of MC_SEG_STK_NARROW entries - an array of exactly that size),
//                                   the six frames in rows of MC_MAXAA + 2 bytes, MC_INV behind the frame's length.
//                                   stdout: "reads N frames M full_list_pushes K0 K1" - the pushes that found the work list full, per form.
//   seg_narrow primitives           every McBits64 operation against McBits192 on sets over n <= 63 positions.
//                                   stdout: "primitives CHECKS mismatches K"; exit status 1 if K > 0.
static long g_seg_full[2] = {0, 0};
static int g_form = 0;
#define MC_SEG_ON_FULL() (g_seg_full[g_form]++)
#include "../../microbecensus_amd/csrc/mc_index.h"

static long g_checks = 0, g_bad = 0;
static void check(bool ok, const char *what, int a, int b, int c)
{
    g_checks++;
    if (!ok && g_bad++ < 20) fprintf(stderr, "mismatch: %s (%d, %d, %d)\n", what, a, b, c);
}
static bool same(const McBits64 &x, const McBits192 &y) { return x.a == y.a && y.b == 0 && y.c == 0; }
// "no bit": 192 in the wide form, 64 in the narrow one - both at or beyond every length n <= 63; a found bit is the same position
static bool same_next(int r64, int r192) { return r192 < 64 ? r64 == r192 : (r192 == 192 && r64 == 64); }

static int primitives()
{
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    for (int n = 0; n <= MC_NARROW_MAXAA; n++) {
        const uint64_t all = n ? (~0ull >> (64 - n)) : 0;
        std::vector<uint64_t> sets = {0, 1, 1ull << 62, 1ull | (1ull << 62), ~0ull, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull};
        for (int k = 0; k < 24; k++) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; sets.push_back(lcg ^ (lcg >> 29)); }
        {   // low(n), bits set one by one, clear
            McBits64 l = mc_bits_low(McBits64(), n); McBits192 L = mc_bits_low(McBits192(), n);
            check(same(l, L) && l.a == all, "low", n, 0, 0);
            McBits64 s; McBits192 S; mc_bits_clear(s); mc_bits_clear(S);
            for (int i = 0; i < n; i += 1 + (i % 3)) { mc_bits_set(s, i); mc_bits_set(S, i); }
            check(same(s, S), "set", n, 0, 0);
            for (int i = 0; i < n; i++) check(mc_bits_test(s, i) == mc_bits_test(S, i), "test", n, i, 0);
            check(mc_bits_any(s) == mc_bits_any(S), "any", n, 0, 0);
        }
        for (size_t q = 0; q < sets.size(); q++) {
            McBits64 x; x.a = sets[q] & all;                         // a set over [0, n): empty, bit 0, bit 62 (n = 63), both, full, patterns
            McBits192 X; X.a = x.a; X.b = 0; X.c = 0;
            check(mc_bits_any(x) == mc_bits_any(X), "any", n, (int)q, 0);
            for (int from = 0; from <= n; from++) check(same_next(mc_bits_next(x, from), mc_bits_next(X, from)), "next", n, (int)q, from);
            for (int from = -1; from < n; from++) check(mc_bits_prev(x, from) == mc_bits_prev(X, from), "prev", n, (int)q, from);
            for (int k = 0; k <= 63; k++) check(same(mc_bits_shr(x, k), mc_bits_shr(X, k)), "shr", n, (int)q, k);   // 0 and 62 among them
            McBits64 y; y.a = sets[(q + 5) % sets.size()] & all;
            McBits192 Y; Y.a = y.a; Y.b = 0; Y.c = 0;
            check(same(mc_bits_and(x, y), mc_bits_and(X, Y)), "and", n, (int)q, 0);
            check(same(mc_bits_or(x, y), mc_bits_or(X, Y)), "or", n, (int)q, 0);
            check(same(mc_bits_andnot(x, y), mc_bits_andnot(X, Y)), "andnot", n, (int)q, 0);
            // the flags of every segment [base, base + m) of a frame of n residues, for both windows
            for (int W = 8; W <= 12; W += 4)
                for (int base = 0; base + W <= n; base++)
                    for (int m = W; base + m <= n; m++) check(same(mc_seg_flags_of(x, base, m, W), mc_seg_flags_of(X, base, m, W)), "flags_of", n, base, m);
        }
    }
    for (int lo = 0; lo <= 62; lo++)
        for (int hi = lo; hi <= 62; hi++) check(same(mc_bits_range(McBits64(), lo, hi), mc_bits_range(McBits192(), lo, hi)), "range", lo, hi, 0);   // (0, 62) among them
    printf("primitives %ld mismatches %ld\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "primitives")) return primitives();
    if (argc != 5 || strcmp(argv[1], "frames")) { fprintf(stderr, "usage: seg_narrow frames READS L OUT | seg_narrow primitives\n"); return 2; }
    const int L = atoi(argv[3]);
    if (L < 18 || L / 3 > MC_NARROW_MAXAA) { fprintf(stderr, "L out of range (18..%d)\n", 3 * MC_NARROW_MAXAA + 2); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    std::vector<uint8_t> reads;
    { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) reads.insert(reads.end(), buf, buf + k); }
    fclose(f);
    if (reads.size() % (size_t)L) { fprintf(stderr, "%s: %zu bytes are no multiple of L = %d\n", argv[2], reads.size(), L); return 2; }
    const size_t n = reads.size() / (size_t)L;
    static McTables T;
    McHostIndex X;                                                   // the SEG and codon tables do not depend on the index
    X.rt_mask = 0; X.max_bucket = 0; X.freq_thr = 0; X.nres = 1000000; X.nseq = 1000;
    for (int g = 0; g < 10; g++) X.letter_p[g] = 0.1;
    mc_fill_tables(T, X, L, 1.0);
    { double mm = 0; if (mc_seg_fx_verify(T, &mm)) { fprintf(stderr, "the fixed-point entropy tests disagree with the double arithmetic\n"); return 3; } }
    const int FP = MC_MAXAA + 2;
    std::vector<uint8_t> out(n * 2 * 6 * (size_t)FP, (uint8_t)MC_INV);
    for (size_t r = 0; r < n; r++)
        for (int form = 0; form < 2; form++)
            for (int fr = 0; fr < 6; fr++) {
                uint8_t *p = &out[((r * 2 + (size_t)form) * 6 + (size_t)fr) * (size_t)FP];
                const int m = mc_translate_frame(T, &reads[r * (size_t)L], L, fr, p);
                uint8_t comp[20], sv[24];
                g_form = form;
                if (form == 0) {
                    int16_t stk[MC_SEG_STK];
                    McSegWS ws{comp, sv, stk};
                    mc_seg_mask_fx2<McBits192>(T.lnfac, T.seg_dout, p, m, ws);
                } else {
                    int16_t stk[MC_SEG_STK_NARROW];                  // exactly the narrow row's list: a push behind it is an address error
                    McSegWS ws{comp, sv, stk};
                    mc_seg_mask_fx2<McBits64>(T.lnfac, T.seg_dout, p, m, ws);
                }
            }
    FILE *o = fopen(argv[4], "wb");
    if (!o || fwrite(out.data(), 1, out.size(), o) != out.size() || fclose(o)) { perror(argv[4]); return 2; }
    printf("reads %zu frames %zu full_list_pushes %ld %ld\n", n, n * 6, g_seg_full[0], g_seg_full[1]);
    return 0;
}
