// community.cpp - test driver: reads [first, first + n) of one simulated community library, made on the CPU by the draw and the
// generator the device kernels run (csrc/mc_simlib.h: mc_sim_member_table, mc_sim_place, mc_sim_walk), written as n x L bytes, and
// where every read was placed.  Test infrastructure only; the product runs the HIP build.
//
//     community bases.bin off.bin mfirst.bin copies.bin L paired insert model rate seed lib first n out.bin places.bin
// bases.bin: the members' bytes one after another; off.bin: int64 contig offsets (ncontig + 1); mfirst.bin: int32 first contig of
// every member (M + 1); copies.bin: int64 (M); model: 0 none, 1 uniform, 2 illumina.  places.bin: per read int64 member, contig, start.
// An empty bases.bin: only the places are made (out.bin stays empty) - tables too large to have bases.
// Exit status 4: the universe is 0; 5: it does not stay below 2^62.
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
    if (argc != 16) { fprintf(stderr, "usage: community bases.bin off.bin mfirst.bin copies.bin L paired insert model rate seed lib first n out.bin places.bin\n"); return 2; }
    const std::vector<char> braw = slurp(argv[1]), oraw = slurp(argv[2]), mraw = slurp(argv[3]), craw = slurp(argv[4]);
    const uint8_t *bases = (const uint8_t *)braw.data();
    const int64_t *off = (const int64_t *)oraw.data();
    const int32_t *mfirst = (const int32_t *)mraw.data();
    const int64_t *copies = (const int64_t *)craw.data();
    const int ncontig = (int)(oraw.size() / 8) - 1, M = (int)(craw.size() / 8);
    if ((int)(mraw.size() / 4) != M + 1 || mfirst[0] != 0 || mfirst[M] != ncontig) { fprintf(stderr, "mfirst does not fit\n"); return 2; }
    const int L = atoi(argv[5]), paired = atoi(argv[6]), insert = atoi(argv[7]), model = atoi(argv[8]);
    const double rate = atof(argv[9]);
    const uint64_t seed = strtoull(argv[10], nullptr, 10), lib = strtoull(argv[11], nullptr, 10);
    const int64_t first = atoll(argv[12]), n = atoll(argv[13]);
    const int span = paired ? insert : L;
    std::vector<int64_t> vs((size_t)ncontig), total((size_t)M);
    std::vector<uint64_t> cum((size_t)M + 1);
    const int bad = mc_sim_member_table(off, mfirst, copies, M, span, vs.data(), total.data(), cum.data());
    if (bad) { fprintf(stderr, bad == 1 ? "no contig of %d bases\n" : "universe of 2^62 or more (span %d)\n", span); return 3 + bad; }
    uint64_t thr[MC_SIM_NTHR];
    mc_sim_thresholds(model, rate, thr);
    const uint64_t key = mc_mix64(seed ^ mc_mix64(lib)), ekey = mc_mix64(key ^ MC_SIM_EKEY);
    const bool walk = !braw.empty();
    std::vector<uint8_t> out(walk ? (size_t)n * L : 0);
    std::vector<int64_t> places((size_t)n * 3);
    for (int64_t k = 0; k < n; k++) {
        const int64_t i = first + k;
        const McSimPlace pl = mc_sim_place(cum.data(), total.data(), mfirst, vs.data(), off, M, mc_mix64(key + (uint64_t)(paired ? i >> 1 : i)));
        const int c = pl.contig;
        const int64_t s = pl.start;
        places[(size_t)k * 3] = pl.member; places[(size_t)k * 3 + 1] = c; places[(size_t)k * 3 + 2] = s;
        if (pl.member < 0 || pl.member >= M || c < mfirst[pl.member] || c >= mfirst[pl.member + 1] || s < off[c] || s + span > off[c + 1]) {
            fprintf(stderr, "read %lld placed outside its member\n", (long long)i);
            return 3;
        }
        if (!walk) continue;
        const bool rev = paired && (i & 1);
        auto base = [&](int64_t p) {
            if (p < off[c] || p >= off[c + 1]) { fprintf(stderr, "read %lld left its contig\n", (long long)i); exit(3); }
            return bases[p];
        };
        uint8_t *row = out.data() + (size_t)k * L;
        auto emit = [&](int o, uint8_t x) { row[o] = x; };
        McSimNoEvent ev;
        mc_sim_walk(base, emit, ev, off[c], off[c + 1], rev ? s + span - 1 : s, rev ? -1 : 1, L, mc_mix64(ekey + (uint64_t)i), thr, model != MC_SIM_ERR_NONE);
    }
    FILE *f = fopen(argv[14], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { perror(argv[14]); return 2; }
    fclose(f);
    f = fopen(argv[15], "wb");
    if (!f || fwrite(places.data(), 8, places.size(), f) != places.size()) { perror(argv[15]); return 2; }
    fclose(f);
    return 0;
}
