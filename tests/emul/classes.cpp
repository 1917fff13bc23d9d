// Host build of csrc/mc_classes.h for tests/test_classes_host.py.
//   classes L1,L2,... -> first line: what mc_classes_check returns and the value it names; then, for a legal list, for every
//   len = 0 .. 520 one line "len row_len class": the read of len bases written as a padded row (its first min(len, stride) bases, then
//   0 bytes), the length mc_class_row_len finds in it and the class of that length (K = none) - and the class of len itself, which
//   must be the same
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../microbecensus_amd/csrc/mc_classes.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::vector<int32_t> cl;
    for (char *p = strtok(argv[1], ","); p; p = strtok(nullptr, ",")) cl.push_back(atoi(p));
    int32_t bad = 0;
    const int what = mc_classes_check(cl.data(), (int32_t)cl.size(), &bad);
    printf("%d %d\n", what, bad);
    if (what) return 0;
    McClasses C; C.K = (int32_t)cl.size();
    for (int k = 0; k < C.K; k++) C.len[k] = cl[(size_t)k];
    const int stride = mc_class_stride(C);
    std::vector<uint8_t> row((size_t)stride);
    for (int len = 0; len <= 520; len++) {
        for (int i = 0; i < stride; i++) row[(size_t)i] = i < len ? (uint8_t)"ACGTN"[i % 5] : 0;
        const int rl = mc_class_row_len(row.data(), stride);
        printf("%d %d %d %d\n", len, rl, mc_class_of(C, rl), mc_class_of(C, len));
    }
    return 0;
}
