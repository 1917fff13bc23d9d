// mc_ahead.h - the bookkeeping of a lookahead: the translation (k_translate_seg, stage A0) of the range that is expected NEXT, issued
// while the ordering and finishing kernels of the running range leave the device nearly empty (mc_hip.hip: range_end, range_begin).
// Host code: mc_hip.hip keeps one McAhead per handle, tests/emul/ahead.cpp compiles it with g++.  No HIP include here.
//
//     The key of a lookahead says whose frames lie in d_frames: the generation of the resident read buffer (a device pointer is no
//     key - mc_upload and the stream's two slots reuse addresses for other reads; the generation is bumped wherever the buffer or its
//     contents change), the first read and the reads covered, the read length, the frame pitch, and the generation of the run's tables
//     (bumped wherever d_T changes: mc_set_run, mc_set_run_classes, McLenBorrow::use / close).
//     predict: the range that follows [first, first + count) contiguously in a set of nreads reads - up to count reads from
//     first + count, clipped to the set; nothing at its end.  That is how mc_search, mc_search_files and the bench walk a set.
//     offer: a lookahead with this key has been issued.
//     take: a range is begun - how many of its reads are covered?  None unless every field but the count matches; then the smaller of
//     the two counts: the frames of a read do not depend on its neighbours, so a range of the same first read and fewer reads is a
//     prefix of the lookahead, and one of more reads has the lookahead as its prefix - the caller translates the reads behind it on
//     top.  The lookahead is gone either way: d_frames is the begun range's from here on.
//     drop: the lookahead is gone.
#pragma once
#include <stdint.h>
#include <algorithm>

struct McAheadKey { uint64_t reads_gen; int64_t first, count; int32_t read_len, FP; uint64_t tables_gen; };
struct McAhead { McAheadKey key = {0, 0, 0, 0, 0, 0}; bool live = false; };

// the reads of the predicted range (0: none), its first read in *next_first
inline int64_t mc_ahead_predict(int64_t first, int64_t count, int64_t nreads, int64_t *next_first)
{
    *next_first = 0;
    if (first < 0 || count <= 0 || first > nreads - count) return 0;   // (not a range of the set: nothing follows it)
    const int64_t at = first + count;
    const int64_t n = std::min(count, nreads - at);
    if (n <= 0) return 0;
    *next_first = at;
    return n;
}

inline void mc_ahead_offer(McAhead &a, const McAheadKey &k) { a.key = k; a.live = true; }

inline void mc_ahead_drop(McAhead &a) { a.live = false; }

inline int64_t mc_ahead_take(McAhead &a, const McAheadKey &want)
{
    const bool was = a.live;
    a.live = false;
    const McAheadKey &k = a.key;
    if (!was || want.count <= 0 || k.count <= 0 || k.reads_gen != want.reads_gen || k.first != want.first || k.read_len != want.read_len || k.FP != want.FP || k.tables_gen != want.tables_gen) return 0;
    return std::min(k.count, want.count);
}
