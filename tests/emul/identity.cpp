// tests/emul/identity.cpp - the rules of the identity that need no GPU (csrc/mc_identity.h: mc_id_bin - the very function k_identity runs
// per best row -, the figures of one histogram mc_id_total, mc_id_min, mc_id_median, mc_id_max and mc_id_ge, and mc_id_bad_level) compiled
// by g++ and run on the CPU: a stand-alone program that includes the library's header and copies none of it.
//   identity run IN OUT      (files of sections: order_io.h; tests/test_identity_host.py writes IN and reads OUT)
// IN:  pairs (int32 nmatch, alnlen), histograms (MC_ID_BINS uint32 each), levels (int32; any number: the check is mc_id_bad_level's).
// OUT: the pairs' bins (int32), per histogram 4 + L int64 (total, min, median, max, ge of every level; L = 0 when the levels are refused),
//      and three int32: mc_id_bad_level of the levels, MC_ID_BINS and MC_ID_LEVELS.
// Every histogram lives in a std::vector of its exact size: -fsanitize=address sees a read behind bin 100.
#include "../../microbecensus_amd/csrc/mc_identity.h"

#include "order_io.h"

int main(int argc, char **argv)
{
    if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: identity run IN OUT\n"); return 2; }
    Sections in = sections_read(argv[2]), out;
    size_t npair, nhist, nlev;
    const int32_t *pair = in.take<int32_t>(&npair);
    const uint32_t *hist = in.take<uint32_t>(&nhist);
    const int32_t *lev = in.take<int32_t>(&nlev);
    if (npair % 2 || nhist % MC_ID_BINS) { fprintf(stderr, "input: malformed\n"); return 2; }
    std::vector<int32_t> bins;
    for (size_t i = 0; i < npair; i += 2) bins.push_back(mc_id_bin(pair[i], pair[i + 1]));
    const std::vector<int32_t> levels(lev, lev + nlev);
    const int bad = mc_id_bad_level(levels.data(), (int)nlev);
    std::vector<int64_t> figs;
    for (size_t g = 0; g < nhist / MC_ID_BINS; g++) {
        const std::vector<uint32_t> h(hist + g * MC_ID_BINS, hist + (g + 1) * MC_ID_BINS);
        figs.push_back((int64_t)mc_id_total(h.data())); figs.push_back(mc_id_min(h.data())); figs.push_back(mc_id_median(h.data())); figs.push_back(mc_id_max(h.data()));
        for (size_t j = 0; bad < 0 && j < nlev; j++) figs.push_back((int64_t)mc_id_ge(h.data(), levels[j]));
    }
    const std::vector<int32_t> meta = {bad, MC_ID_BINS, MC_ID_LEVELS};
    out.put(bins); out.put(figs); out.put(meta);
    sections_write(argv[3], out);
    return 0;
}
