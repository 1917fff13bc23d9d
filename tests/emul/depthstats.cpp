// tests/emul/depthstats.cpp - the rules of the depth statistics that need no GPU (csrc/mc_depthstats.h: mc_ds_cut, mc_ds_lo, mc_ds_hi,
// mc_ds_median_rank - the very functions k_depth_select runs per gene -, mc_ds_keep_ok, and mc_ds_trimmed_sum, the boundary arithmetic of
// the selection) compiled by g++ and run on the CPU: a stand-alone program that includes the library's header and copies none of it.
//   depthstats run IN OUT      (files of sections: order_io.h; tests/test_depthstats_host.py writes IN and reads OUT)
// IN:  pairs (uint32 len >= 1, P in 1 .. 100); records of 8 uint64 (low, high, lo, hi, n_lt_low, n_le_low, n_lt_high, between); values of P
//      (int64; any).
// OUT: per pair 4 uint32 (cut, lo, hi, the median's rank); per record one uint64 (the trimmed sum); per value of P one int32 (mc_ds_keep_ok);
//      and the int32 MC_DS_NOUT.
#include "../../microbecensus_amd/csrc/mc_depthstats.h"

#include "order_io.h"

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: depthstats run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npair, nrec, nkeep;
    const uint32_t *pair = in.take<uint32_t>(&npair);
    const uint64_t *rec = in.take<uint64_t>(&nrec);
    const int64_t *keep = in.take<int64_t>(&nkeep);
    if (npair % 2 || nrec % 8) { fprintf(stderr, "input: malformed\n"); return 2; }
    std::vector<uint32_t> ranks;
    for (size_t i = 0; i < npair; i += 2) {
        const uint32_t len = pair[i]; const int32_t P = (int32_t)pair[i + 1];
        if (len < 1 || len > 65535 || !mc_ds_keep_ok(P)) { fprintf(stderr, "input: pair %zu: len %u, P %d\n", i / 2, len, P); return 2; }
        ranks.push_back(mc_ds_cut(len, P)); ranks.push_back(mc_ds_lo(len, P)); ranks.push_back(mc_ds_hi(len, P)); ranks.push_back(mc_ds_median_rank(len));
    }
    std::vector<uint64_t> sums;
    for (size_t i = 0; i < nrec; i += 8) {
        const uint64_t *r = rec + i;
        sums.push_back(mc_ds_trimmed_sum((uint32_t)r[0], (uint32_t)r[1], (uint32_t)r[2], (uint32_t)r[3], (uint32_t)r[4], (uint32_t)r[5], (uint32_t)r[6], r[7]));
    }
    std::vector<int32_t> ok;
    for (size_t i = 0; i < nkeep; i++) ok.push_back(mc_ds_keep_ok(keep[i]) ? 1 : 0);
    const std::vector<int32_t> meta = {MC_DS_NOUT};
    out.put(ranks); out.put(sums); out.put(ok); out.put(meta);
    sections_write(argv[3], out);
    return 0;
}
