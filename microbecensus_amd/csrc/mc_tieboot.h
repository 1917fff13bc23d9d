// mc_tieboot.h - the bootstrap of the tie shares (mc_set_tie_bootstrap, mc_tie_bootstrap): how sure an rpkg_shared is.  It extends
// mc_geneboot.h from the count of a gene's reads to the gene's even share of the reads it ties for.  Same conventions as mc_geneboot.h
// and mc_ties.h: host and device code alike, no HIP include of its own - k_tieboot.h runs it on the device, g++ compiles the very same text
// into tests/emul/tieboot.cpp, and tests/tieboot_restated.py restates it in numpy.
//
// ---- THE STATEMENT ----------------------------------------------------------------------------------------------------------------
// WHICH READS.  A read's tied set, its size k (1 <= k <= 500), its first tied subject and its shares are exactly k_ties.h's: every tied
// subject gets floor(2^32 / k), the first tied subject the remainder 2^32 - k * floor(2^32 / k) as well; a read that k_abundance.h does
// not assign adds nothing.  The walk is mc_ties_read (mc_ties.h) and nothing else: the sinks below only look at what it hands them.
// IDS.  q is the read's global id, 0 <= q < 2^31, as in the gene bootstrap: mc_row.query, and in a class run base + perm[query]
// (mc_tb_id; k_geneboot.h's McIdMap).
// THE REPLICATE SHARE  cs[b][s], b in 0 .. B - 1, 1 <= B <= MC_GB_MAXB, is the sum of mc_boot_weight(mc_boot_key(seed, b), q) * share(q, s)
// over the reads q whose tied set holds s: an exact unsigned 64-bit integer in units of 2^-32 that does not depend on ranges, batches,
// launch geometry or the order of the atomics.  A weight is at most MC_BOOT_K = 19, a share at most 2^32, and the list holds at most
// MC_TB_MAXCAP = 2^27 entries: 19 * 2^32 * 2^27 < 2^64, no sum can wrap.  Replicate b under one seed is the same resample of the same
// reads as replicate b of mc_gene_bootstrap and of mc_bootstrap.
// THE VALUE.  s32[b] = scale[b] * 2^-32 (mc_tb_scale: one double multiplication, on the host); replicate b is USED when mc_gb_used(s32[b]);
// v[b] = mc_gb_value(cs[b][s], s32[b]).  The six doubles of a gene are mc_geneboot.h's on these values, in its addition order:
// k_geneboot_summary and mc_gb_gene are handed the share matrix and s32 as they are.
// INVARIANTS.  For every b the sum over s of cs[b][s] is 2^32 times the sum over s of c[b][s], c the gene bootstrap's replicate counts (a
// read's shares add up to 2^32).  If no read ties, cs = c * 2^32 and the six doubles are the gene bootstrap's bit for bit: (double) of
// c * 2^32 is (double)c * 2^32 and scale * 2^-32 is exact (short of underflow), so every product has the bits it had.
//
// ---- THE ENTRY --------------------------------------------------------------------------------------------------------------------
// One entry per (read, tied subject): 12 bytes - the read id, the gene, the share less one.  A share of 2^32 (k = 1) does not fit 32
// bits, share - 1 always does (a share is at least floor(2^32 / 500) > 0).  Read id (31 bits), gene (15) and share (32) are 78 bits: 8
// bytes cannot hold them, and 12 is the next size a 4-byte-aligned array can have; the list is read once by the scatter and once per
// replicate tile by the sums, so its bytes are the traffic of a read, and 16 bytes would buy one aligned load at a third more of both -
// at the cap of 2^27 entries the two lists are 3 GiB and not 4.  The share itself is kept, not k: the sums then need no division and no
// "first tied subject" flag, and an entry is everything a replicate needs of it.
#pragma once
#include "mc_geneboot.h"
#include "mc_ties.h"

#define MC_TB_MAXCAP 134217728                                      // 2^27 entries: the most a list may hold (THE REPLICATE SHARE: no sum wraps)

// an entry of the device list.  In the collected list `gene` is the subject; in the grouped list the compact index of the gene among
// those with candidates
struct McTbEntry { uint32_t q, gene, share_m1; };

MC_HD unsigned long long mc_tb_share(const McTbEntry &e) { return (unsigned long long)e.share_m1 + 1ull; }
MC_HD double mc_tb_scale(double s) { return s * 2.3283064365386962890625e-10; }      // (2^-32)
// the global id of the read whose rows carry `query`: perm null: the id itself; else base + perm[query], below 2^31 (mc_search_classes)
MC_HD uint32_t mc_tb_id(const uint32_t *perm, int64_t base, int32_t query) { return perm ? (uint32_t)(base + (int64_t)perm[query]) : (uint32_t)query; }

// The two sinks of mc_ties_read.  The counting sink takes nothing: the walk's own answer, McTieRead::k, is the number of entries.
struct McTbCount {
    MC_HD bool marks() const { return false; }
    MC_HD void cand(int32_t) {}
    MC_HD void mark(int32_t, int32_t, int32_t) {}
    MC_HD void share(int32_t, unsigned long long) {}
    MC_HD void uniq(int32_t) {}
    MC_HD void group_uniq(int32_t) {}
};
// The writing sink: share(s, v) is the next entry of read q, at `slot`.  An entry whose slot is not below capacity is counted in
// `dropped` and written nowhere: nothing is ever written behind the list.  Every other method is empty.
struct McTbWrite {
    McTbEntry *list; unsigned long long capacity, slot; uint32_t q, dropped;
    MC_HD bool marks() const { return false; }
    MC_HD void cand(int32_t) {}
    MC_HD void mark(int32_t, int32_t, int32_t) {}
    MC_HD void share(int32_t s, unsigned long long v)
    {
        if (slot < capacity) { McTbEntry e; e.q = q; e.gene = (uint32_t)s; e.share_m1 = (uint32_t)(v - 1ull); list[slot] = e; }
        else dropped++;
        slot++;
    }
    MC_HD void uniq(int32_t) {}
    MC_HD void group_uniq(int32_t) {}
};

// What ONE thread does for the read at row i, in two halves with the slot reservation between them (k_tieboot_collect: a scan over the
// workgroup and one atomic; the emulation: a running count).  mc_tb_count: the entries the read will write, 0 for a read that adds nothing.
// mc_tb_write: those entries at slot, slot + 1, ..; returns how many did not fit.
template <class Pass>
MC_HD uint32_t mc_tb_count(const Pass &passes, const McRow *rows, uint32_t nrows, uint32_t i, int32_t nseq)
{
    McTbCount sink;
    return mc_ties_read(passes, rows, nrows, i, nseq, (const int32_t *)nullptr, sink).k;
}
template <class Pass>
MC_HD uint32_t mc_tb_write(const Pass &passes, const McRow *rows, uint32_t nrows, uint32_t i, int32_t nseq, uint32_t q, McTbEntry *list, unsigned long long capacity, unsigned long long slot)
{
    McTbWrite sink; sink.list = list; sink.capacity = capacity; sink.slot = slot; sink.q = q; sink.dropped = 0;
    (void)mc_ties_read(passes, rows, nrows, i, nseq, (const int32_t *)nullptr, sink);
    return sink.dropped;
}
