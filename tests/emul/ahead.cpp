// Host build of csrc/mc_ahead.h for tests/test_ahead_host.py.  Every argument is one operation on ONE McAhead, in order, and prints one line:
//   p:first:count:nreads                         predict          -> "p <reads> <next_first>"
//   o:reads_gen:first:count:L:FP:tables_gen      offer            -> "o <live>"
//   t:reads_gen:first:count:L:FP:tables_gen      take             -> "t <reads covered> <live>"
//   d                                            drop             -> "d <live>"
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
        if (s[0] == 'p' && s[1] == ':') {
            long long first, count, nreads;
            if (sscanf(s + 2, "%lld:%lld:%lld", &first, &count, &nreads) != 3) return 2;
            int64_t at = -1;
            const int64_t n = mc_ahead_predict(first, count, nreads, &at);
            printf("p %lld %lld\n", (long long)n, (long long)at);
        } else if (s[0] == 'o' && s[1] == ':') {
            if (!key_of(s + 2, &k)) return 2;
            mc_ahead_offer(a, k);
            printf("o %d\n", a.live ? 1 : 0);
        } else if (s[0] == 't' && s[1] == ':') {
            if (!key_of(s + 2, &k)) return 2;
            const int64_t covered = mc_ahead_take(a, k);
            printf("t %lld %d\n", (long long)covered, a.live ? 1 : 0);
        } else if (!strcmp(s, "d")) {
            mc_ahead_drop(a);
            printf("d %d\n", a.live ? 1 : 0);
        } else
            return 2;
    }
    return 0;
}
