// Host build of csrc/mc_fold.h for tests/test_fold_host.py.
//   fold segs L V len...   -> per len one line "len n off_0:len_0:lo_0:hi_0 ..." (mc_fold_nsegs, mc_fold_seg, mc_fold_seg_len)
//   fold spans L V len     -> every span [a, b] of a gene of len residues with at most V + 1 residues: the number of those that do NOT lie
//                             inside segment mc_fold_seg_of(a), and the number checked: "bad checked"
//   fold rows IN OUT       -> IN: one int32 (the segments), the records (McFoldSeg), the rows (McRow); OUT: the rows folded by mc_fold_row
//                             and one int64, the rows mc_fold_edge names  (files of sections: order_io.h)
//   fold consts            -> "MC_FOLD_SEG_LEN MC_FOLD_OVERLAP MC_FOLD_MAX_GENE MC_FOLD_MAX_SEGS MC_MAXAA"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../microbecensus_amd/csrc/mc_fold.h"
#include "order_io.h"

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "consts")) { printf("%d %d %d %d %d\n", MC_FOLD_SEG_LEN, MC_FOLD_OVERLAP, MC_FOLD_MAX_GENE, MC_FOLD_MAX_SEGS, MC_MAXAA); return 0; }
    if (argc >= 5 && !strcmp(argv[1], "segs")) {
        const int L = atoi(argv[2]), V = atoi(argv[3]);
        for (int k = 4; k < argc; k++) {
            const int len = atoi(argv[k]), n = mc_fold_nsegs(len, L, V);
            printf("%d %d", len, n);
            for (int j = 0; j < n; j++) { const McFoldSeg s = mc_fold_seg(0, len, j, L, V); printf(" %d:%d:%d:%d", s.off, mc_fold_seg_len(len, j, L, V), s.lo, s.hi); }
            printf("\n");
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "spans")) {
        const int L = atoi(argv[2]), V = atoi(argv[3]), len = atoi(argv[4]);
        long long bad = 0, checked = 0;
        for (int a = 0; a < len; a++)
            for (int b = a; b < len && b - a + 1 <= V + 1; b++) {
                const int j = mc_fold_seg_of(a, len, L, V), o = mc_fold_seg_off(j, L, V);
                checked++;
                if (!(j >= 0 && j < mc_fold_nsegs(len, L, V) && o <= a && b <= o + mc_fold_seg_len(len, j, L, V) - 1)) bad++;
            }
        printf("%lld %lld\n", bad, checked);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "rows")) {
        Sections in = sections_read(argv[2]), out;
        size_t nm, nseg, nrows;
        const int32_t *meta = in.take<int32_t>(&nm);
        const McFoldSeg *seg = in.take<McFoldSeg>(&nseg);
        const McRow *rows = in.take<McRow>(&nrows);
        if (nm != 1 || (size_t)meta[0] != nseg) return 2;
        std::vector<McRow> f(nrows);
        int64_t edge = 0;
        for (size_t i = 0; i < nrows; i++) { f[i] = mc_fold_row(rows[i], meta[0], seg); edge += mc_fold_edge(rows[i], meta[0], seg) ? 1 : 0; }
        out.put(f); out.put(&edge, 1);
        sections_write(argv[3], out);
        return 0;
    }
    return 2;
}
