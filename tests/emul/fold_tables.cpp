// Host build of csrc/mc_index.h and csrc/mc_fold.h for tests/test_fold_host.py: the alignment statistics of an index of SEGMENTS that
// carries the statistics pair of the unsplit genes (McHostIndex::stat_nres, stat_nseq) are those of the unsplit index.
//   fold_tables <genes.faa> L V read_len   -> three lines of "name 0|1": `stats` 1 when ell, mprime, nprime, logK and every entry of loge_r
//   and bits_r of the segment index WITH the pair hold the bits of the unsplit index's; `unset_differs` 1 when the same segment index
//   WITHOUT the pair gives another nprime (the pair is what makes them equal); `rest` 1 when every other byte of the two segment tables is
//   the same (the pair touches nothing else); and a line "segments n genes g split k"
#include "../../microbecensus_amd/csrc/mc_finish.h"
#include "../../microbecensus_amd/csrc/mc_index.h"
#include "../../microbecensus_amd/csrc/mc_fold.h"
#include <fstream>

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int L = atoi(argv[2]), V = atoi(argv[3]), read_len = atoi(argv[4]);
    std::vector<std::string> names, seqs;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty()) continue;
            if (line[0] == '>') { names.push_back(line.substr(1)); seqs.push_back(""); }
            else if (!seqs.empty()) seqs.back() += line;
        }
    }
    std::vector<std::string> snames, sseqs;
    int64_t nres = 0; int split = 0;
    for (size_t g = 0; g < names.size(); g++) {
        const int len = (int)seqs[g].size(), n = mc_fold_nsegs(len, L, V);
        nres += len; split += n > 1;
        for (int j = 0; j < n; j++) { snames.push_back(names[g] + "|" + std::to_string(j)); sseqs.push_back(seqs[g].substr((size_t)mc_fold_seg_off(j, L, V), (size_t)mc_fold_seg_len(len, j, L, V))); }
    }
    const auto build = [](const std::vector<std::string> &nm, const std::vector<std::string> &sq, McHostIndex &X) {
        std::vector<const char *> a, b; std::string err;
        for (size_t i = 0; i < nm.size(); i++) { a.push_back(nm[i].c_str()); b.push_back(sq[i].c_str()); }
        if (!mc_build_index(X, a.data(), b.data(), (int)nm.size(), err)) { fprintf(stderr, "%s\n", err.c_str()); exit(2); }
    };
    static McHostIndex G, S;
    build(names, seqs, G); build(snames, sseqs, S);
    static McTables TG, TS, TU;
    mc_fill_tables(TG, G, read_len, 1.0);
    mc_fill_tables(TU, S, read_len, 1.0);
    S.stat_nres = nres; S.stat_nseq = (int)names.size();
    mc_fill_tables(TS, S, read_len, 1.0);
    const bool stats = !memcmp(&TG.ell, &TS.ell, sizeof TG.ell) && !memcmp(&TG.mprime, &TS.mprime, sizeof TG.mprime) && !memcmp(&TG.nprime, &TS.nprime, sizeof TG.nprime) &&
                       !memcmp(&TG.logK, &TS.logK, sizeof TG.logK) && !memcmp(TG.loge_r, TS.loge_r, sizeof TG.loge_r) && !memcmp(TG.bits_r, TS.bits_r, sizeof TG.bits_r);
    McTables A = TS, B = TU;                                        // the segment tables with the statistics fields made equal: every other byte
    A.ell = B.ell; A.mprime = B.mprime; A.nprime = B.nprime; memcpy(A.loge_r, B.loge_r, sizeof A.loge_r); memcpy(A.bits_r, B.bits_r, sizeof A.bits_r);
    printf("stats %d\nunset_differs %d\nrest %d\nsegments %zu genes %zu split %d\n", stats ? 1 : 0, TU.nprime != TG.nprime ? 1 : 0, !memcmp(&A, &B, sizeof A) ? 1 : 0, snames.size(), names.size(), split);
    return 0;
}
