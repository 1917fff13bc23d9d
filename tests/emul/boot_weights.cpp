// Host build of csrc/mc_boot.h for tests/test_bootstrap_host.py: the weights of the (seed, replicate, read) triples in a file,
// and the threshold table as the compiler sees it.
//   boot_weights table                      -> prints MC_BOOT_K, MC_BOOT_KEY and the thresholds, one per line (decimal)
//   boot_weights weights <in.bin> <out.bin> -> in: n x 3 uint64 (seed, b, r); out: n uint8 weights
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../microbecensus_amd/csrc/mc_boot.h"

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "table")) {
        printf("%d\n%llu\n", MC_BOOT_K, (unsigned long long)MC_BOOT_KEY);
        for (int k = 0; k < MC_BOOT_K; k++) printf("%llu\n", (unsigned long long)MC_BOOT_THR[k]);
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "weights")) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 3;
    std::vector<uint64_t> in;
    uint64_t buf[3 * 4096];
    for (size_t got; (got = fread(buf, 24, 4096, f)) > 0;) in.insert(in.end(), buf, buf + 3 * got);
    fclose(f);
    std::vector<uint8_t> out(in.size() / 3);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)mc_boot_weight(mc_boot_key(in[3 * i], in[3 * i + 1]), in[3 * i + 2]);
    FILE *o = fopen(argv[3], "wb");
    if (!o) return 4;
    fwrite(out.data(), 1, out.size(), o);
    fclose(o);
    return 0;
}
