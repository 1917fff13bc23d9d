// mc_classes.h - length classes: how a run that estimates from reads of mixed lengths (mc_set_run_classes, mc_reader_open_classes)
// assigns every read the length it is searched and classified at.  Host and device code alike: k_classes.h runs it on the rows of a
// batch, mc_reader.cpp on the records of a file, tests/emul/classes.cpp compiles it with g++.  No HIP include here.
//
//     A run has K length classes class_len[0] < ... < class_len[K - 1], 1 <= K <= MC_CLS_MAX, each in MC_CLS_MINLEN .. MC_CLS_MAXLEN.
//     The class of a read of len bases is the largest k with class_len[k] <= len; the read is cut to its first class_len[k] bases.
//     A read with len < class_len[0] has no class (k = K): it is "too short".
//     A read travels as one row of stride = class_len[K - 1] bytes: its first min(len, stride) bases, then 0 bytes.  No base is a
//     0 byte, so the length of a row is the index of its first 0 byte, or stride.  (A read longer than stride belongs to the top
//     class whatever was cut off: min(len, stride) has the class of len.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MC_CLS_HD __host__ __device__ inline
#else
#define MC_CLS_HD inline
#endif

#define MC_CLS_MAX 32
#define MC_CLS_MINLEN 18
#define MC_CLS_MAXLEN 510

struct McClasses { int32_t K; int32_t len[MC_CLS_MAX]; };

// 0: a legal class list; else what is wrong: 1 K, 2 a length outside MC_CLS_MINLEN .. MC_CLS_MAXLEN, 3 not ascending; *bad = the offending value
MC_CLS_HD int mc_classes_check(const int32_t *class_len, int32_t K, int32_t *bad)
{
    if (K < 1 || K > MC_CLS_MAX) { *bad = K; return 1; }
    for (int k = 0; k < K; k++) {
        if (class_len[k] < MC_CLS_MINLEN || class_len[k] > MC_CLS_MAXLEN) { *bad = class_len[k]; return 2; }
        if (k && class_len[k] <= class_len[k - 1]) { *bad = class_len[k]; return 3; }
    }
    return 0;
}

// the class of a read of len bases: 0 .. K - 1, or K = none
MC_CLS_HD int mc_class_of(const McClasses &c, int len)
{
    int k = c.K;
    for (int j = 0; j < c.K; j++) if (c.len[j] <= len) k = j;   // (ascending: the last one that fits is the largest)
    return k;
}

MC_CLS_HD int mc_class_stride(const McClasses &c) { return c.len[c.K - 1]; }

// the length of a row: the index of its first 0 byte, or stride
MC_CLS_HD int mc_class_row_len(const uint8_t *row, int stride)
{
    int n = 0;
    while (n < stride && row[n]) n++;
    return n;
}
