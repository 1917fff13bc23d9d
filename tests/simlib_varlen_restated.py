"""The simulator's reference read-length mode (csrc/mc_simlib.h, mc_sim_walk_ref; mc_genome_set_read_lengths MC_READLEN_REFERENCE)
restated in plain Python, read by read: the walk consumes the fragment bases j = 0 .. L-1 and emits whatever the error process makes
of them - seq_sim.py's read of L + insertions - deletions bases.  The draws are those of simlib_restated.simulate."""
import numpy as np

import simlib_restated as sr


def simulate_varlen(bases, off, L, first, n, seed, lib, error_model=None, error_rate=None, paired_end=False, insert=None):
    """Rows [first, first + n) of library (seed, lib): (bases uint8, offsets int64 of n + 1, events (ins, del) per read)."""
    bases = np.asarray(bases, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    span = insert if paired_end else L
    vstart = np.zeros(len(off), dtype=np.int64)
    vstart[1:] = np.cumsum(np.maximum(0, np.diff(off) - span + 1))
    total = int(vstart[-1])
    key = sr.mix64(seed ^ sr.mix64(lib))
    ekey = sr.mix64(key ^ sr.EKEY)
    thr = sr.thresholds(error_model, error_rate)
    errors = error_model is not None
    out, offs, events = bytearray(), [0], []
    for i in range(first, first + n):
        u = sr.mix64((key + ((i >> 1) if paired_end else i)) & sr.MASK) % total
        c = int(np.searchsorted(vstart, u, side="right") - 1)
        s = int(off[c]) + (u - int(vstart[c]))
        rev = paired_end and (i & 1)
        p, step = (s + span - 1, -1) if rev else (s, 1)
        r = sr.mix64((ekey + i) & sr.MASK)
        ins = dels = 0
        for j in range(L):
            b = int(bases[p])
            if rev:
                b = int(sr.COMP[b])
            e = 0
            if errors:
                d = sr.mix64((r + j * sr.GAMMA) & sr.MASK)
                if (d >> 32) < thr[min(j, sr.NTHR - 1)]:
                    kind = (d >> 16) & 0xFFFF
                    x = int(sr.ACGT[d & 3])
                    e = 1 if kind < sr.SUB else 2 if kind < sr.INS else 3
            if e == 0:
                out.append(b)
            elif e == 1:
                out.append(x)
            elif e == 2:
                out += bytes((x, b))
                ins += 1
            else:
                dels += 1
            p += step
        offs.append(len(out))
        events.append((ins, dels))
    return np.frombuffer(bytes(out), dtype=np.uint8), np.array(offs, dtype=np.int64), events
