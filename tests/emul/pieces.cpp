// Host build of csrc/mc_pieces.h for tests/test_pieces_host.py.
//   pieces BATCH L:n:first,L:n:first,... -> first line "Lmax nmax nshort npieces", then one line "L tag bin_first bin_n first n" per
//   piece, in the cutter's order.  An empty list is written as ","
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../microbecensus_amd/csrc/mc_pieces.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const long long batch = atoll(argv[1]);
    std::vector<McBin> bins;
    for (char *p = strtok(argv[2], ","); p; p = strtok(nullptr, ",")) {
        int L; long long n, first;
        if (sscanf(p, "%d:%lld:%lld", &L, &n, &first) != 3) return 2;
        bins.push_back({L, (int64_t)n, (int64_t)first});
    }
    const McPieces P = mc_cut_pieces(bins, batch);
    printf("%d %lld %lld %zu\n", P.Lmax, (long long)P.nmax, (long long)P.nshort, P.v.size());
    for (const McPiece &q : P.v) printf("%d %d %lld %lld %lld %lld\n", q.L, q.tag, (long long)q.bin_first, (long long)q.bin_n, (long long)q.first, (long long)q.n);
    return 0;
}
