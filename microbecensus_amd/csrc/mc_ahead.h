// mc_ahead.h - the bookkeeping of a lookahead: the translation (k_translate_seg, stage A0) of the range that is expected NEXT, issued
// beside the running range, into the frame buffer that range does not use (mc_hip.hip: range_begin, range_end, ahead_issue).
// Host code: mc_hip.hip keeps one McAhead per handle, tests/emul/ahead.cpp and ahead_buffers.cpp compile it with g++.  No HIP include here.
//
//     The key of a lookahead says whose frames lie in the buffer it wrote: the generation of the resident read buffer (a device pointer is no
//     key - mc_upload and the stream's two slots reuse addresses for other reads; the generation is bumped wherever the buffer or its
//     contents change), the first read and the reads covered, the read length, the frame pitch, and the generation of the run's tables
//     (bumped wherever d_T changes: mc_set_run, mc_set_run_classes, McLenBorrow::use / close).
//     predict: the range that follows [first, first + count) contiguously in a set of nreads reads - up to count reads from
//     first + count, clipped to the set; nothing at its end.  That is how mc_search, mc_search_files and the bench walk a set.
//     offer: a lookahead with this key has been issued.
//     take: a range is begun - how many of its reads are covered?  None unless every field but the count matches; then the smaller of
//     the two counts: the frames of a read do not depend on its neighbours, so a range of the same first read and fewer reads is a
//     prefix of the lookahead, and one of more reads has the lookahead as its prefix - the caller translates the reads behind it on
//     top.  The lookahead is gone either way.
//     drop: the lookahead is gone.
//     The buffers: a context has TWO frame buffers.  cur is the one that holds the running range's frames - what every reader of
//     d_frames sees; a lookahead writes the other one (mc_ahead_target), while the running range still reads its own, and offer records
//     which (buf).  A take that covers any read makes the lookahead's buffer the current one - the reads behind a partial cover are
//     translated on top, into the same buffer; a take that covers none, and a drop, leave cur as it is: a lookahead that is not taken
//     changes nothing.
#pragma once
#include <stdint.h>
#include <algorithm>

struct McAheadKey { uint64_t reads_gen; int64_t first, count; int32_t read_len, FP; uint64_t tables_gen; };
struct McAhead { McAheadKey key = {0, 0, 0, 0, 0, 0}; bool live = false; int cur = 0, buf = 1; };

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

// the buffer a lookahead issued now writes
inline int mc_ahead_target(const McAhead &a) { return a.cur ^ 1; }

inline void mc_ahead_offer(McAhead &a, const McAheadKey &k) { a.key = k; a.buf = mc_ahead_target(a); a.live = true; }

inline void mc_ahead_drop(McAhead &a) { a.live = false; }

inline int64_t mc_ahead_take(McAhead &a, const McAheadKey &want)
{
    const bool was = a.live;
    a.live = false;
    const McAheadKey &k = a.key;
    if (!was || want.count <= 0 || k.count <= 0 || k.reads_gen != want.reads_gen || k.first != want.first || k.read_len != want.read_len || k.FP != want.FP || k.tables_gen != want.tables_gen) return 0;
    a.cur = a.buf;
    return std::min(k.count, want.count);
}
