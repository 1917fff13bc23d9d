// Host build of csrc/mc_wfit.h for tests/test_wfit_host.py (g++ -ffp-contract=off): the perturbations, the mask, the per-library
// errors, mue and whole fits, as the compiler makes them of the header.
//   wfit consts                   -> MC_WFIT_KEY, C, G, MAX_N (decimal) and SIGMA0, SIGMA_MIN, MAD_CONST (%.17g), one per line
//   wfit d <in.bin> <out.bin>     -> in: n x 5 uint64 (seed, L, g, c, f); out: n float64
//   wfit eval <in.bin> <out.bin>  -> in: int64 N, F, K, 0, 0, 0; pred[N][F]; truth[N]; w[K][F]
//                                    out: pm[N][F]; keep[N] (as float64); alive (as float64); errors[K][N]; mue[K]
//   wfit fit <in.bin> <out.bin>   -> in: int64 N, F, C, G, seed, L; pred[N][F]; truth[N];  out: weights[F]; trace[G + 1][3]
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../microbecensus_amd/csrc/mc_wfit.h"

static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    unsigned char buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}

static int dump(const char *path, const std::vector<double> &out)
{
    FILE *o = fopen(path, "wb");
    if (!o) return 4;
    fwrite(out.data(), 8, out.size(), o);
    fclose(o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "consts")) {
        printf("%llu\n%d\n%d\n%d\n%.17g\n%.17g\n%.17g\n", (unsigned long long)MC_WFIT_KEY, MC_WFIT_C, MC_WFIT_G, MC_WFIT_MAX_N, (double)MC_WFIT_SIGMA0, (double)MC_WFIT_SIGMA_MIN,
               (double)MC_WFIT_MAD_CONST);
        return 0;
    }
    if (argc != 4) return 2;
    const std::vector<unsigned char> in = slurp(argv[2]);
    std::vector<double> out;
    if (!strcmp(argv[1], "d")) {
        const uint64_t *q = (const uint64_t *)in.data();
        for (size_t i = 0; i < in.size() / 40; i++) out.push_back(mc_wfit_d(q[5 * i], q[5 * i + 1], q[5 * i + 2], q[5 * i + 3], (int)q[5 * i + 4]));
        return dump(argv[3], out);
    }
    if (in.size() < 48) return 3;
    const int64_t *hd = (const int64_t *)in.data();
    const int N = (int)hd[0], F = (int)hd[1];
    const double *pred = (const double *)(in.data() + 48), *truth = pred + (size_t)N * F;
    if (!strcmp(argv[1], "eval")) {
        const int K = (int)hd[2];
        const double *w = truth + N;
        if (in.size() != 48 + 8 * ((size_t)N * F + N + (size_t)K * F)) return 3;
        std::vector<double> pm((size_t)N * F), errs(N);
        std::vector<uint32_t> keep(N);
        const uint32_t alive = mc_wfit_mask(pred, N, F, pm.data(), keep.data());
        out = pm;
        for (int n = 0; n < N; n++) out.push_back((double)keep[n]);
        out.push_back((double)alive);
        std::vector<double> mue(K);
        for (int k = 0; k < K; k++) {
            mue[k] = mc_wfit_mue(pm.data(), keep.data(), truth, N, F, w + (size_t)k * F, errs.data());
            out.insert(out.end(), errs.begin(), errs.end());
        }
        out.insert(out.end(), mue.begin(), mue.end());
        return dump(argv[3], out);
    }
    if (!strcmp(argv[1], "fit")) {
        const int C = (int)hd[2], G = (int)hd[3];
        if (in.size() != 48 + 8 * ((size_t)N * F + N)) return 3;
        out.resize((size_t)F + 3 * (size_t)(G + 1));
        mc_wfit_fit(pred, truth, N, F, (uint64_t)hd[4], (uint64_t)hd[5], C, G, out.data(), out.data() + F);
        return dump(argv[3], out);
    }
    return 2;
}
