// mc_simlib.h - the per-read generator of the training workflow's library simulator, for every library kind: error model none,
// uniform(rate) or illumina (training/sim_functions.py:92-140), single end or paired end with an insert (training/seq_sim.py -p -i).
// Host and device code alike: k_simulate.h runs it one read per lane, tests/emul/sim_library.cpp compiles it with g++.  No HIP
// include here: under hipcc the includer has included the HIP runtime already (MC_SIM_HD then is __host__ __device__).
//
// A library of kind (L, paired, insert, model) under (seed, lib); key as in k_simulate.h, G = 0x9E3779B97F4A7C15:
//     key     = mix(seed ^ mix(lib))                                    (starts)
//     ekey    = mix(key ^ 0xA0761D6478BD642F)                           (errors: their own domain, so an error model never moves a start)
//     span    = insert if paired else L;  vstart / total: the valid starts of span bases, as k_simulate.h makes them for L
//     frag    = i >> 1 if paired else i;  u = mix(key + frag) % total;  c, s = contig and start of u as in k_simulate.h
//     mate    = i & 1 if paired else 0
//     mate 0: walks forward from s;  mate 1: walks leftward from s + span - 1 and complements (ACGT <-> TGCA, acgt <-> tgca, any other
//             byte kept as it is)
//     r       = mix(ekey + i)                                            (row i: each mate has its own errors)
// The walk consumes fragment bases j = 0, 1, ... (b = the j-th base in the read's direction) and emits until the read has L bases:
//     d       = mix(r + j * G)                                           (the splitmix64 stream of state r)
//     error   = (d >> 32) < thr[min(j, MC_SIM_NTHR - 1)]                 (thr: mc_sim_thresholds; never drawn under model none)
//     kind    = (d >> 16) & 0xFFFF:  < 52429 substitution (0.8),  < 58982 insertion (0.1),  else deletion (0.1)
//     x       = "ACGT"[d & 3]
//     no error: emit b;  substitution: emit x;  insertion: emit x, then b;  deletion: emit nothing - unless fewer bases lie past b in
//     the read's direction inside its contig than the read still needs, and then b is emitted as if there were no error.
// So the walk never leaves the contig and the start set is that of the error-free library.  Deviation: the reference's read is
// the mutated L-base fragment prefix (L + insertions - deletions bases); here a read is the FIRST L bases the process emits (it
// reads on past the L-th fragment base after deletions), since the engine searches reads of one length.
// Read-length mode "reference" (mc_genome_set_read_lengths(g, MC_READLEN_REFERENCE); mc_sim_walk_ref): the same draws, but the walk
// consumes exactly the fragment bases j = 0 .. L-1 and emits whatever the errors produce - seq_sim.py's read of
// L + insertions - deletions bases:
//     no error: emit b;  substitution: emit x;  insertion: emit x, then b;  deletion: emit nothing (always: the walk never reads past
//     the L-th base, so no deletion is refused)
// Under error model none both modes give the same read.  A read longer than 510 bases is refused by the caller (never cut).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MC_SIM_HD __host__ __device__ inline
#else
#define MC_SIM_HD inline
#endif

enum { MC_SIM_ERR_NONE = 0, MC_SIM_ERR_UNIFORM = 1, MC_SIM_ERR_ILLUMINA = 2 };
enum { MC_SIM_LEN_FIXED = 0, MC_SIM_LEN_REFERENCE = 1 };
#define MC_SIM_NTHR 235                        // p(j) of both models is constant for j >= 234
#define MC_SIM_EKEY 0xA0761D6478BD642Full
#define MC_SIM_GAMMA 0x9E3779B97F4A7C15ull
#define MC_SIM_SUB 52429u                      // kind cut points of 65536: 0.8 and 0.9 within 2^-16
#define MC_SIM_INS 58982u

MC_SIM_HD uint64_t mc_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MC_SIM_HD uint8_t mc_sim_comp(uint8_t b)
{
    switch (b) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    default: return b;
    }
}

// The error thresholds of one model on the host (so that no compiler contracts p(j) differently on the device): thr[j] =
// floor(p(j) x 2^32), 2^32 where p(j) >= 1; p(j) = (3e-3 + 3.3e-8 (j+1)^4) / 100 for illumina, rate for uniform, 0 for none.
inline void mc_sim_thresholds(int model, double rate, uint64_t *thr)
{
    for (int j = 0; j < MC_SIM_NTHR; j++) {
        const double t = (double)(j + 1);
        const double t4 = t * t * t * t;                               // exact: (j+1)^4 < 2^53
        const double a = 3.3e-8 * t4;
        const double b = 3e-3 + a;
        const double p = model == MC_SIM_ERR_ILLUMINA ? b / 100.0 : model == MC_SIM_ERR_UNIFORM ? rate : 0.0;
        thr[j] = p >= 1.0 ? (1ull << 32) : (uint64_t)(p * 4294967296.0);
    }
}

// the contig of valid start u: the last c with vstart[c] <= u
MC_SIM_HD int mc_sim_contig(const int64_t *vstart, int ncontig, uint64_t u)
{
    int lo = 0, hi = ncontig;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((uint64_t)vstart[mid] <= u) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

// A community library (k_community.h; tests/emul/community.cpp): M member genomes with copies[m] cells each, their contigs one
// after another (member m holds contigs mfirst[m] .. mfirst[m + 1] - 1).  key, ekey, span, frag, mate, the walk and the error stream
// are those of a genome's library above; only the place of a fragment is drawn differently - a read comes from member m with
// probability proportional to copies[m] x (valid starts of m):
//     total[m] = valid starts of span bases in member m;  vstart[c] = valid starts of the member's contigs in front of contig c
//     cum[m]   = sum over k < m of copies[k] x total[k];  universe = cum[M]  (0 < universe < 2^62)
//     u        = mix(key + frag) % universe
//     m        = the member with cum[m] <= u < cum[m + 1]            (a member without a contig of span bases is never drawn)
//     v        = (u - cum[m]) % total[m];  c = the contig of m with vstart[c] <= v < vstart[c] + its valid starts;  s = off[c] + v - vstart[c]
// One member with one copy: universe = total, u = v, and the library is the genome's, byte for byte.
struct McSimPlace { int member, contig; int64_t start; };           // start: the fragment's first base in the concatenated bases

MC_SIM_HD McSimPlace mc_sim_place(const uint64_t *cum, const int64_t *total, const int32_t *mfirst, const int64_t *vstart, const int64_t *off, int M, uint64_t x)
{
    const uint64_t u = x % cum[M];
    int lo = 0, hi = M;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum[mid] <= u) lo = mid + 1; else hi = mid; }
    McSimPlace p;
    p.member = lo - 1;
    const uint64_t v = (u - cum[p.member]) % (uint64_t)total[p.member];
    const int c0 = mfirst[p.member];
    p.contig = c0 + mc_sim_contig(vstart + c0, mfirst[p.member + 1] - c0, v);
    p.start = off[p.contig] + (int64_t)(v - (uint64_t)vstart[p.contig]);
    return p;
}

// The member table of a community for fragments of span bases, on the host (mc_community_* and the g++ test build): vstart
// (ncontig), total (M), cum (M + 1).  Returns 0, or 1 when the universe is 0 (no member has a contig of span bases) and 2 when it
// does not stay below 2^62.
#define MC_SIM_MAX_MEMBERS 65536
#define MC_SIM_MAX_COPIES (1 << 20)
#define MC_SIM_MAX_UNIVERSE (1ull << 62)
inline int mc_sim_member_table(const int64_t *off, const int32_t *mfirst, const int64_t *copies, int M, int span, int64_t *vstart, int64_t *total, uint64_t *cum)
{
    cum[0] = 0;
    for (int m = 0; m < M; m++) {
        int64_t t = 0;
        for (int c = mfirst[m]; c < mfirst[m + 1]; c++) {
            vstart[c] = t;
            const int64_t w = off[c + 1] - off[c] - span + 1;
            if (w > 0) t += w;
        }
        total[m] = t;
        const unsigned __int128 next = (unsigned __int128)cum[m] + (unsigned __int128)(uint64_t)copies[m] * (uint64_t)t;
        if (next >= MC_SIM_MAX_UNIVERSE) return 2;
        cum[m + 1] = (uint64_t)next;
    }
    return cum[M] == 0 ? 1 : 0;
}

// One read's walk.  base(p) returns the genome byte at absolute position p; emit(o, x) stores byte o of the read; event(j, e, x),
// if the caller wants the log, sees every consumed base (e: 0 none, 1 substitution, 2 insertion, 3 deletion, 4 deletion refused).
// [cs, ce) is the read's contig, p0 its first consumed base, dir +1 or -1.
template <class Base, class Emit, class Event>
MC_SIM_HD void mc_sim_walk(Base &base, Emit &emit, Event &event, int64_t cs, int64_t ce, int64_t p0, int dir, int L, uint64_t r, const uint64_t *thr, bool errors)
{
    int64_t p = p0;
    int o = 0;
    for (int j = 0; o < L; j++, p += dir) {
        uint8_t b = base(p);
        if (dir < 0) b = mc_sim_comp(b);
        int e = 0;
        uint8_t x = 0;
        if (errors) {
            const uint64_t d = mc_mix64(r + (uint64_t)j * MC_SIM_GAMMA);
            if ((d >> 32) < thr[j < MC_SIM_NTHR ? j : MC_SIM_NTHR - 1]) {
                const uint32_t kind = (uint32_t)(d >> 16) & 0xFFFFu;
                x = (uint8_t)(0x54474341u >> (8 * (uint32_t)(d & 3)));     // "ACGT"[d & 3]
                e = kind < MC_SIM_SUB ? 1 : kind < MC_SIM_INS ? 2 : 3;
                if (e == 3 && (dir > 0 ? ce - 1 - p : p - cs) < (int64_t)(L - o)) e = 4;
            }
        }
        event(j, e, x);
        if (e == 0 || e == 4) emit(o++, b);
        else if (e == 1) emit(o++, x);
        else if (e == 2) { emit(o++, x); if (o < L) emit(o++, b); }
    }
}

// The walk of the reference mode: fragment bases j = 0 .. L-1, every event emitted as drawn; returns the read's length.  emit may
// be a counter only (the length pass of k_simulate.h).
template <class Base, class Emit>
MC_SIM_HD int mc_sim_walk_ref(Base &base, Emit &emit, int64_t p0, int dir, int L, uint64_t r, const uint64_t *thr, bool errors)
{
    int64_t p = p0;
    int o = 0;
    for (int j = 0; j < L; j++, p += dir) {
        uint8_t b = base(p);
        if (dir < 0) b = mc_sim_comp(b);
        int e = 0;
        uint8_t x = 0;
        if (errors) {
            const uint64_t d = mc_mix64(r + (uint64_t)j * MC_SIM_GAMMA);
            if ((d >> 32) < thr[j < MC_SIM_NTHR ? j : MC_SIM_NTHR - 1]) {
                const uint32_t kind = (uint32_t)(d >> 16) & 0xFFFFu;
                x = (uint8_t)(0x54474341u >> (8 * (uint32_t)(d & 3)));     // "ACGT"[d & 3]
                e = kind < MC_SIM_SUB ? 1 : kind < MC_SIM_INS ? 2 : 3;
            }
        }
        if (e == 0) emit(o++, b);
        else if (e == 1) emit(o++, x);
        else if (e == 2) { emit(o++, x); emit(o++, b); }
    }
    return o;
}

struct McSimNoEvent {
    MC_SIM_HD void operator()(int, int, uint8_t) const {}
};
