// mc_ties.h - the per-read walk of the tie accounting (k_ties.h states the rule): what ONE GPU thread does for one read, at the read's
// first row.  Same conventions as mc_core.h and mc_finish.h: MC_HD code, no HIP include of its own, so that g++ compiles the very same
// walk into tests/emul/ties.cpp and runs it on the CPU against tests/ties_restated.py.
//
// The walk is a template over two things it does not know:
//   Pass   passes(row) -> bool: whether a row passes the cut-offs (on the device: mc_abund_passes of k_abundance.h on the row's fields)
//   Sink   where the counts go (on the device: vector atomics into the tables; on the CPU: plain additions):
//            cand(s)            candidates[s] += 1
//            mark(s, a, b)      the any-depth of subject s: +1 on residues a .. b (called only while the sink wants marks: marks())
//            share(s, v)        share[s] += v                       (units of 2^-32)
//            uniq(s)            unique[s] += 1
//            group_uniq(g)      group_unique[g] += 1
#pragma once
#include "mc_core.h"

#define MC_TIES_ONE 4294967296ull                                  // one read, in the fixed point of share[]

struct McTieRead { uint32_t k; bool across; };                      // the size of a read's tied set (0: the read adds nothing) and "spans more than one group"

// whether row j - a passing row with bits == T of a subject below nseq - names a subject that an EARLIER such row of the read, from
// `first` on, has named already.  Only called for tied rows: the check is quadratic in the tied rows, and a row that is not tied costs
// one comparison of its subject here.  The callers ask only when the subject's bit of a 64-bit mask of the tied subjects met so far
// (bit s mod 64) is set: a subject whose bit is clear has not been met, and a small tied set seldom asks at all.
template <class Pass>
MC_HD bool mc_ties_seen(const Pass &passes, const McRow *rows, uint32_t first, uint32_t j, double T)
{
    const int32_t s = rows[j].subject;
    for (uint32_t m = first; m < j; m++)
        if (rows[m].subject == s && rows[m].bits == T && passes(rows[m])) return true;
    return false;
}

// rows: the nrows final rows of a range, ascending read id; i: the read's first row.  group_of: nseq groups, or null.
// Up to three walks over the read's rows (at most 500):
//   1  T, the highest bits among the passing rows, the first and the last passing row that have it, and how many do - the first is the
//      row k_abundance.h assigns the read by; a read without one, or whose first-rule subject is not below nseq, adds nothing.  ONE row
//      at T is a tied set of one: the read is counted from what this walk kept, and most reads end here - after the walk k_abundance makes
//   2  from the first to the last row at T: every tied subject once, at its representative row: candidates, the any-depth mark, k, and
//      whether two groups are met
//   3  floor(2^32 / k) to every tied subject once more; a tied set of one subject (its rows all the same subject's) needs no third
//      walk, and a tied set without a repeated subject (as many tied rows as tied subjects) needs no duplicate check in it
template <class Pass, class Sink>
MC_HD McTieRead mc_ties_read(const Pass &passes, const McRow *rows, uint32_t nrows, uint32_t i, int32_t nseq, const int32_t *group_of, Sink &sink)
{
    McTieRead out; out.k = 0; out.across = false;
    const int32_t q = rows[i].query;
    double T = 0.0; uint32_t first = 0, last = 0, at_top = 0; int32_t fsub = -1, fa = 0, fb = 0;
    for (uint32_t j = i; j < nrows; j++) {
        const McRow r = rows[j];                                    // (the whole row at once, as k_abundance reads it)
        if (r.query != q) break;
        if (!passes(r)) continue;
        if (at_top == 0 || T < r.bits) { T = r.bits; first = last = j; at_top = 1; fsub = r.subject; fa = r.sstart; fb = r.send; }
        else if (r.bits == T) { at_top++; last = j; }
    }
    if (at_top == 0 || fsub < 0 || fsub >= nseq) return out;
    const int32_t g0 = group_of ? group_of[fsub] : 0;
    if (at_top == 1) {
        out.k = 1;
        sink.cand(fsub);
        if (sink.marks()) sink.mark(fsub, fa, fb);
        if (group_of) sink.group_uniq(g0);
        sink.uniq(fsub); sink.share(fsub, MC_TIES_ONE);
        return out;
    }
    uint32_t k = 0, tied_rows = 0;
    unsigned long long met = 0;
    for (uint32_t j = first; j <= last; j++) {
        const int32_t s = rows[j].subject;
        if (!(rows[j].bits == T) || s < 0 || s >= nseq || !passes(rows[j])) continue;
        tied_rows++;
        const unsigned long long bit = 1ull << (s & 63);
        if ((met & bit) && mc_ties_seen(passes, rows, first, j, T)) continue;
        met |= bit;
        k++;
        sink.cand(s);
        if (sink.marks()) sink.mark(s, rows[j].sstart, rows[j].send);
        if (group_of && group_of[s] != g0) out.across = true;
    }
    out.k = k;
    if (group_of && !out.across) sink.group_uniq(g0);
    if (k == 1) { sink.uniq(fsub); sink.share(fsub, MC_TIES_ONE); return out; }
    const unsigned long long each = MC_TIES_ONE / k;
    sink.share(fsub, each + (MC_TIES_ONE - each * k));              // (the remainder goes to the first tied subject)
    met = 1ull << (fsub & 63);
    for (uint32_t j = first + 1; j <= last; j++) {
        const int32_t s = rows[j].subject;
        if (!(rows[j].bits == T) || s < 0 || s >= nseq || !passes(rows[j])) continue;
        const unsigned long long bit = 1ull << (s & 63);
        if (tied_rows != k && (met & bit) && mc_ties_seen(passes, rows, first, j, T)) continue;
        met |= bit;
        sink.share(s, each);
    }
    return out;
}
