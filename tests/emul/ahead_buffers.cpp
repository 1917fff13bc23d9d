// Host build of csrc/mc_ahead.h for tests/test_ahead_buffers_host.py: which of a context's two frame buffers is the running range's
// after every operation.  Every argument is one operation on ONE McAhead, in order, and prints one line:
//   o:reads_gen:first:count:L:FP:tables_gen      offer            -> "o <live> <buffer the lookahead wrote> <current buffer>"
//   t:reads_gen:first:count:L:FP:tables_gen      take             -> "t <reads covered> <live> <current buffer>"
//   d                                            drop             -> "d <live> <current buffer>"
//   g                                            target           -> "g <the buffer a lookahead issued now would write>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../microbecensus_amd/csrc/mc_ahead.h"

static bool key_of(const char *s, McAheadKey *k)
{
    unsigned long long rg, tg; long long first, count; int L, FP;
    if (sscanf(s, "%llu:%lld:%lld:%d:%d:%llu", &rg, &first, &count, &L, &FP, &tg) != 6) return false;
    *k = {(uint64_t)rg, (int64_t)first, (int64_t)count, (int32_t)L, (int32_t)FP, (uint64_t)tg};
    return true;
}

int main(int argc, char **argv)
{
    McAhead a;
    for (int i = 1; i < argc; i++) {
        const char *s = argv[i];
        McAheadKey k;
        if (s[0] == 'o' && s[1] == ':') {
            if (!key_of(s + 2, &k)) return 2;
            mc_ahead_offer(a, k);
            printf("o %d %d %d\n", a.live ? 1 : 0, a.buf, a.cur);
        } else if (s[0] == 't' && s[1] == ':') {
            if (!key_of(s + 2, &k)) return 2;
            const int64_t covered = mc_ahead_take(a, k);
            printf("t %lld %d %d\n", (long long)covered, a.live ? 1 : 0, a.cur);
        } else if (!strcmp(s, "d")) {
            mc_ahead_drop(a);
            printf("d %d %d\n", a.live ? 1 : 0, a.cur);
        } else if (!strcmp(s, "g")) {
            printf("g %d\n", mc_ahead_target(a));
        } else
            return 2;
        if (a.cur != 0 && a.cur != 1) return 3;                      // (an index into two buffers)
    }
    return 0;
}
