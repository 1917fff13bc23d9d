// k_abund_classes.h - the per-class table of a class run that the abundance counts ride on (mc_set_abundance_classes,
// mc_abundance_classes_read): per length class the rows sorted into it and the reads of it that were assigned to a gene - the n_k of a
// mixed-length RPKG's denominator, sum n_k x L_k, and what every class gave to the numerator.
//
// ---- Layout -----------------------------------------------------------------------------------------------------------------------
// (K + 1) x 2 counters, class k at [2 k]: rows, [2 k + 1]: assigned.  Slot K is the rows below the lowest class: they are searched
// by nobody and assign nothing.  The buffer is sized for the most classes a run may have (MC_CLS_MAX: the class list may change while
// the switch is on) and holds ONE more slot behind those, [MC_AC_SEEN]: the count table's `assigned` total as the last piece left
// it.  The buffer is zeroed with the counts and by nobody else, so that slot and the total agree.
//
// ---- The rule ---------------------------------------------------------------------------------------------------------------------
// A piece is a range of ONE class, and the counting kernel of a range adds its assigned reads to one total (k_abundance.h,
// counts[nseq][0]).  So what a piece assigned is that total behind its counting kernel minus the total behind the piece before it
// (k_abund_class_mark notes it before a batch's first piece): one thread reads the total in the piece's stream, behind the counting
// kernel, and adds the difference to the piece's class (k_abund_class_add).  No
// second walk over the rows, no sync on the host; a piece that overflowed a pool never gets here and its halves come one by one
// (range_end).  A handle runs one range at a time, in one stream: the pieces cannot interleave.
#pragma once
#include <hip/hip_runtime.h>
#include "mc_classes.h"

#define MC_AC_SEEN (2 * (MC_CLS_MAX + 1))
#define MC_AC_SLOTS (MC_AC_SEEN + 1)

// Before the first piece of a batch: the total as it stands (ranges that were no pieces may have added to it since the last piece)
__global__ void __launch_bounds__(64) k_abund_class_mark(unsigned long long *tab, const unsigned long long *__restrict__ total)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) tab[MC_AC_SEEN] = *total;
}

// tab: the buffer above; K: the classes of the run, 1 .. MC_CLS_MAX; k: the piece's class, 0 .. K (K: rows without a class - no
// counting kernel ran for them); nreads: the piece's reads; total: the count table's `assigned` slot.  A K or k outside that adds nothing.
__global__ void __launch_bounds__(64) k_abund_class_add(unsigned long long *tab, int32_t K, int32_t k, unsigned long long nreads, const unsigned long long *__restrict__ total)
{
    if (blockIdx.x || threadIdx.x || K < 1 || K > MC_CLS_MAX || k < 0 || k > K) return;
    const unsigned long long now = *total;
    tab[2 * k] += nreads;
    tab[2 * k + 1] += now - tab[MC_AC_SEEN];
    tab[MC_AC_SEEN] = now;
}
