// mc_pieces.h - the pieces of a batch that has been sorted into bins of one read length each (the length buckets of mc_search_varlen
// and of mc_train_library's reference read-length mode, the length classes of mc_search_classes): the fixed-length pipeline runs once
// per piece.  Host code: mc_hip.hip cuts every such batch with it, tests/emul/pieces.cpp compiles it with g++.  No HIP include here.
//
//     A bin is the reads of one length, back to back from sorted position `first` of the batch.
//     A bin of fewer than MC_PIECE_MINLEN bases makes no piece: such a read has no frame of more than 5 residues, which RAPsearch2
//     skips - hitless.  Its reads are counted in nshort.
//     Every other bin is cut into ranges of at most `batch` reads, in the order of the bins: range [first, first + n) of the bin.
//     The pools of the run are sized for Lmax, the longest length that made a piece, and nmax, the largest piece.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#define MC_PIECE_MINLEN 18

struct McBin { int L; int64_t n, first; };                       // reads of L bases: how many, and the first one's sorted position
// range [first, first + n) of bin number `tag` of the list: bin_n reads of L bases from sorted position bin_first
struct McPiece { int L, tag; int64_t bin_first, bin_n, first, n; };
struct McPieces { std::vector<McPiece> v; int Lmax = 0; int64_t nmax = 0, nshort = 0; };

inline McPieces mc_cut_pieces(const std::vector<McBin> &bins, int64_t batch)
{
    McPieces P;
    for (size_t b = 0; b < bins.size(); b++) {
        const McBin &x = bins[b];
        if (x.n <= 0) continue;
        if (x.L < MC_PIECE_MINLEN) { P.nshort += x.n; continue; }
        for (int64_t a = 0; a < x.n; a += batch) P.v.push_back({x.L, (int)b, x.first, x.n, a, std::min(batch, x.n - a)});
        P.Lmax = std::max(P.Lmax, x.L); P.nmax = std::max(P.nmax, std::min(batch, x.n));
    }
    return P;
}
