// sim_library_varlen.cpp - test driver: reads [first, first + n) of one simulated library in the reference read-length mode
// (csrc/mc_simlib.h, mc_sim_walk_ref), made on the CPU by the generator the device kernel runs: the bases back to back, then
// n + 1 int64 offsets in a second file.  Test infrastructure only; the product runs the HIP build.
//
//     sim_library_varlen bases.bin off.bin L paired insert model rate seed lib first n out.bin offsets.bin
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../microbecensus_amd/csrc/mc_simlib.h"

static std::vector<char> slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<char> v;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 14) { fprintf(stderr, "usage: sim_library_varlen bases.bin off.bin L paired insert model rate seed lib first n out.bin offsets.bin\n"); return 2; }
    const std::vector<char> braw = slurp(argv[1]), oraw = slurp(argv[2]);
    const uint8_t *bases = (const uint8_t *)braw.data();
    const int64_t *off = (const int64_t *)oraw.data();
    const int ncontig = (int)(oraw.size() / 8) - 1;
    const int L = atoi(argv[3]), paired = atoi(argv[4]), insert = atoi(argv[5]), model = atoi(argv[6]);
    const double rate = atof(argv[7]);
    const uint64_t seed = strtoull(argv[8], nullptr, 10), lib = strtoull(argv[9], nullptr, 10);
    const int64_t first = atoll(argv[10]), n = atoll(argv[11]);
    const int span = paired ? insert : L;
    std::vector<int64_t> vs((size_t)ncontig + 1, 0);
    for (int c = 0; c < ncontig; c++) vs[c + 1] = vs[c] + (off[c + 1] - off[c] - span + 1 > 0 ? off[c + 1] - off[c] - span + 1 : 0);
    if (vs[ncontig] == 0) { fprintf(stderr, "no contig of %d bases\n", span); return 2; }
    uint64_t thr[MC_SIM_NTHR];
    mc_sim_thresholds(model, rate, thr);
    const uint64_t key = mc_mix64(seed ^ mc_mix64(lib)), ekey = mc_mix64(key ^ MC_SIM_EKEY);
    std::vector<uint8_t> out;
    std::vector<int64_t> offs(1, 0);
    std::vector<uint8_t> row((size_t)2 * L + 1);
    for (int64_t k = 0; k < n; k++) {
        const int64_t i = first + k;
        const uint64_t u = mc_mix64(key + (uint64_t)(paired ? i >> 1 : i)) % (uint64_t)vs[ncontig];
        const int c = mc_sim_contig(vs.data(), ncontig, u);
        const int64_t s = off[c] + (int64_t)(u - (uint64_t)vs[c]);
        const bool rev = paired && (i & 1);
        auto base = [&](int64_t p) {
            if (p < off[c] || p >= off[c + 1]) { fprintf(stderr, "read %lld left its contig\n", (long long)i); exit(3); }
            return bases[p];
        };
        auto emit = [&](int o, uint8_t x) { row[(size_t)o] = x; };
        const int len = mc_sim_walk_ref(base, emit, rev ? s + span - 1 : s, rev ? -1 : 1, L, mc_mix64(ekey + (uint64_t)i), thr, model != MC_SIM_ERR_NONE);
        out.insert(out.end(), row.begin(), row.begin() + len);
        offs.push_back((int64_t)out.size());
    }
    FILE *f = fopen(argv[12], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { perror(argv[12]); return 2; }
    fclose(f);
    f = fopen(argv[13], "wb");
    if (!f || fwrite(offs.data(), 8, offs.size(), f) != offs.size()) { perror(argv[13]); return 2; }
    fclose(f);
    return 0;
}
