// seg_forms - the four per-frame statements of the translation + SEG masking (csrc/mc_core.h) on reads of one length, without the
// marker index and without the search: tests/test_seg_oracle_host.py holds each of them to the oracle's rs_translate6().
//
//   seg_forms READS L OUT     READS: n x L bytes of bases.  OUT: per read, per form (0 mc_seg_mask, 1 mc_seg_mask_ws, 2 mc_seg_mask_fx,
//                             3 mc_seg_mask_fx2), the six frames in rows of MC_MAXAA + 2 bytes, MC_INV behind the frame's length.
// stdout: "reads N frames M full_list_pushes K" - K counts the pushes that found the SEG work list full (MC_SEG_ON_FULL; the bound
// at MC_SEG_STK in mc_core.h says there are none).
static long g_seg_full = 0;
#define MC_SEG_ON_FULL() (g_seg_full++)
#include "../../microbecensus_amd/csrc/mc_index.h"

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: seg_forms READS L OUT\n"); return 2; }
    const int L = atoi(argv[2]);
    if (L < 18 || L > 3 * MC_MAXAA) { fprintf(stderr, "L out of range (18..%d)\n", 3 * MC_MAXAA); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> reads;
    { uint8_t buf[65536]; size_t k; while ((k = fread(buf, 1, sizeof buf, f)) > 0) reads.insert(reads.end(), buf, buf + k); }
    fclose(f);
    if (reads.size() % (size_t)L) { fprintf(stderr, "%s: %zu bytes are no multiple of L = %d\n", argv[1], reads.size(), L); return 2; }
    const size_t n = reads.size() / (size_t)L;
    static McTables T;
    McHostIndex X;                                                   // the SEG and codon tables do not depend on the index
    X.rt_mask = 0; X.max_bucket = 0; X.freq_thr = 0; X.nres = 1000000; X.nseq = 1000;
    for (int g = 0; g < 10; g++) X.letter_p[g] = 0.1;
    mc_fill_tables(T, X, L, 1.0);
    { double mm = 0; if (mc_seg_fx_verify(T, &mm)) { fprintf(stderr, "the fixed-point entropy tests disagree with the double arithmetic\n"); return 3; } }
    const int FP = MC_MAXAA + 2;
    std::vector<uint8_t> out(n * 4 * 6 * (size_t)FP, (uint8_t)MC_INV);
    for (size_t r = 0; r < n; r++)
        for (int form = 0; form < 4; form++)
            for (int fr = 0; fr < 6; fr++) {
                uint8_t *p = &out[((r * 4 + (size_t)form) * 6 + (size_t)fr) * (size_t)FP];
                const int m = mc_translate_frame(T, &reads[r * (size_t)L], L, fr, p);
                uint8_t comp[20], sv[24]; int16_t stk[MC_SEG_STK];
                McSegWS ws{comp, sv, stk};
                if (form == 0) {
                    uint8_t mask[(MC_MAXAA + 7) / 8]; double H[MC_MAXAA + 2];
                    mc_seg_mask(T, p, m, mask, H);
                    for (int i = 0; i < m; i++) if (mask[i >> 3] & (1 << (i & 7))) p[i] = MC_INV;
                } else if (form == 1) mc_seg_mask_ws(T, p, m, ws);
                else if (form == 2) mc_seg_mask_fx(T.lnfac, T.seg_dout, p, m, ws);
                else mc_seg_mask_fx2(T.lnfac, T.seg_dout, p, m, ws);
            }
    FILE *o = fopen(argv[3], "wb");
    if (!o || fwrite(out.data(), 1, out.size(), o) != out.size() || fclose(o)) { perror(argv[3]); return 2; }
    printf("reads %zu frames %zu full_list_pushes %ld\n", n, n * 6, g_seg_full);
    return 0;
}
