"""Reads built for the corners of SEG (Seg::segseq / Seg::trim as k_translate_seg and the per-frame forms of csrc/mc_core.h restate
them), and the oracle's side of the comparison: rs_translate6() of oracle/rapsearch_port.c through ctypes.

Proteins are put together from low-complexity chunks and reverse-translated with ONE codon per residue (CODON), so that the other
five frames of a read are low-complexity too.  Everything is drawn from a 64-bit LCG of this module: a set depends on (L, n, seed,
families) alone.  Read i carries its designed protein at base offset i % 3, so every forward frame gets it in turn."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

AA20 = "ACDEFGHIKLMNPQRSTVWY"
CODON = {"A": "GCT", "C": "TGT", "D": "GAT", "E": "GAA", "F": "TTT", "G": "GGT", "H": "CAT", "I": "ATT", "K": "AAA", "L": "CTG",
         "M": "ATG", "N": "AAT", "P": "CCT", "Q": "CAA", "R": "CGT", "S": "TCT", "T": "ACT", "V": "GTT", "W": "TGG", "Y": "TAT"}

# read 2272 of the 510-bp set that first showed the dropped remainder: "A" + the codons of this protein, cut to the read length.
# Frame 1's last masked block is 28 residues long; a work list of eight entries that also lists the remainders shorter than the
# window loses the remainder with CMGCMGCMG and masks only the block's right 19 residues.
WITNESS_PROTEIN = ("HHHHHHHHNGCMDFENNNNNNNNCGPQFKEDDDDDDDDRTYVIGNDDDDDDDDNMTAIEPPPPPPPPPWRGCEIYIIIIIIIIWQFSHTEPPPPPPPPQMCSFVNRRRRRRRRANIGVLTGGGG"
                   "GGGGYEPTWCSCMGCMGCMGYYYYRYRRRRRRRRYRRYRQGSQSG")
WITNESS_FRAME = 1

FAMILIES = ("periodic", "mosaic", "long", "control")
WEIGHTS = {"periodic": 25, "mosaic": 45, "long": 15, "control": 15}     # periodic: a quarter of a full set

MC_INV = 20
MC_FP = 172                                                          # MC_MAXAA + 2: the row of tests/emul/seg_forms
# The oracle's residue codes, (murphy10 group << 4) | (1 + place in the group), and the product's dense codes (place in
# ARNDCQEGHILKMFPSTWYV); the oracle's 0xA0 (stop, unknown codon, masked) is MC_INV.
ORACLE_TO_DENSE = {0x01: 0,                                            # A
                   0x11: 11, 0x12: 1,                                  # K R
                   0x21: 6, 0x22: 3, 0x23: 2, 0x24: 5,                 # E D N Q
                   0x31: 4, 0x41: 7, 0x51: 8,                          # C G H
                   0x61: 9, 0x62: 10, 0x63: 19, 0x64: 12,              # I L V M
                   0x71: 13, 0x72: 18, 0x73: 17,                       # F Y W
                   0x81: 14, 0x91: 15, 0x93: 16}                       # P S T   (0x92 is the '/' of the group string "S/T": no residue)


class Lcg:
    """Knuth's MMIX generator; the high bits are used."""

    def __init__(self, seed):
        self.s = (int(seed) * 0x9E3779B97F4A7C15 + 0x1234567) & 0xFFFFFFFFFFFFFFFF
        for _ in range(4):
            self.next()

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self.s >> 33

    def below(self, n):
        return self.next() % n

    def between(self, lo, hi):
        return lo + self.next() % (hi - lo + 1)

    def pick(self, seq):
        return seq[self.next() % len(seq)]

    def perm(self, seq):
        a = list(seq)
        for i in range(len(a) - 1, 0, -1):
            j = self.next() % (i + 1)
            a[i], a[j] = a[j], a[i]
        return a


def _chunk(r):
    kind = r.below(6)
    if kind == 0:
        return r.pick(AA20) * r.between(3, 11)
    if kind == 1:
        ab = r.perm(AA20)[:2]
        return "".join(r.pick(ab) for _ in range(r.between(6, 19)))
    if kind == 2:
        ab = r.perm(AA20)[:r.between(3, 5)]
        return "".join(r.pick(ab) for _ in range(r.between(8, 23)))
    if kind == 3:
        return "".join(r.perm(AA20)[:r.between(6, 12)])
    if kind == 4:
        return "".join(r.perm(AA20)[:r.between(2, 3)]) * r.between(2, 6)
    return "".join(r.pick(AA20) for _ in range(r.between(4, 13)))


def mosaic(r, naa):
    p = ""
    while len(p) < naa:
        p += _chunk(r)
    return p[:naa]


def periodic(r, naa):
    """Repeats of (a run of 5-8 identical residues, 7-11 distinct ones) until 40 residues before the end, then a mosaic tail: every
    repeat is a short stretch whose trimmed window leaves a remainder to its left - what fills the work list."""
    p = ""
    while len(p) < naa - 40:
        a = r.perm(AA20)
        p += a[0] * r.between(5, 8) + "".join(a[1:1 + r.between(7, 11)])
    return (p + mosaic(r, naa))[:naa]


def long_stretch(r, naa):
    """One stretch of 16 ... min(170, naa) residues - a homopolymer, or two or three letters - and distinct residues behind it.
    Half of them fill the whole frame.  Over 101 residues Seg::trim's minlen becomes n - 100."""
    top = min(170, naa)
    n = top if top < 16 or r.below(2) else r.between(16, top)
    ab = r.perm(AA20)[:r.between(1, 3)]
    p = "".join(r.pick(ab) for _ in range(n))
    while len(p) < naa:
        p += "".join(r.perm(AA20))
    return p[:naa]


def encode(protein, L, offset, r):
    """`offset` random bases, then the protein's codons, cut (or filled with random bases) to L."""
    s = "".join(r.pick("ACGT") for _ in range(offset)) + "".join(CODON[a] for a in protein)
    while len(s) < L:
        s += r.pick("ACGT")
    return np.frombuffer(s[:L].encode(), np.uint8)


def witness(L):
    """The witness read, cut to L.  The 169 residues are the whole of frame 1 at 510 bp (bases 1 ... 507); the two bases behind them
    belong to no codon of that frame and are set to GT here."""
    s = "A" + "".join(CODON[a] for a in WITNESS_PROTEIN) + "GT"
    assert L <= len(s) == 510
    return np.frombuffer(s[:L].encode(), np.uint8)


_genome = []


def control_reads(n, L, seed):
    """Marker-derived reads (synth.sample_reads): frames with little to mask."""
    from microbecensus_amd import _native, synth
    if not _genome:
        _, seqs = _native.load_markers()
        _genome.append(synth.build_genomes(seqs, total_bp=120_000, seed=31, marker_gene_fraction=0.3))
    return synth.sample_reads(_genome[0], n, L, seed=seed)


_DIRTY = "NnacgtRYKMSWBDHVU*-"


def make_reads(L, n, seed, families=FAMILIES, dirty=True, with_witness=True):
    """(n, L) uint8.  Read 0 is the witness (cut to L) when with_witness; a tenth of the other reads get 1-4 dirty bytes."""
    r = Lcg(seed * 1000003 + L)
    fams = [f for f in FAMILIES if f in families]
    assert fams and n >= 1
    cum, t = [], 0
    for f in fams:
        t += WEIGHTS[f]
        cum.append(t)
    out = np.empty((n, L), np.uint8)
    naa = L // 3 + 1
    which = []
    for i in range(n):
        x = r.below(t)
        which.append(fams[next(k for k, c in enumerate(cum) if x < c)])
    nctl = which.count("control")
    ctl = iter(control_reads(nctl, L, seed + 7)) if nctl else iter(())
    for i in range(n):
        f = which[i]
        if f == "control":
            out[i] = next(ctl)
        else:
            prot = periodic(r, naa) if f == "periodic" else mosaic(r, naa) if f == "mosaic" else long_stretch(r, naa)
            out[i] = encode(prot, L, i % 3, r)
        if dirty and r.below(10) == 0:
            for _ in range(r.between(1, 4)):
                out[i, r.below(L)] = ord(r.pick(_DIRTY))
    if with_witness:
        out[0] = witness(L)
    return out


def masked_by_oracle(reads, want=None):
    """(n, 6, MC_FP) bool: the residues the oracle masked - 0xA0 in its output where the plain translation has a residue (a stop or
    an unknown codon is 0xA0 in both)."""
    if want is None:
        want, _ = oracle_frames(reads)
    return (want == MC_INV) & (translate6(reads) != MC_INV)


def sparse_set(L, n, seed):
    """One periodic read in ten (read 3 of every workgroup's ten) among control reads ON WHICH THE ORACLE MASKS NOTHING: marker-derived
    reads are not free of low-complexity windows (at 300 bp nine in ten have one in some frame), so the filler is what is left of
    them after the oracle has looked.  A wave then has stretches pending in the six frames of one read and in no other lane."""
    r = Lcg(seed * 7919 + L)
    clean, have, k = [], 0, 0
    while have < n:
        c = control_reads(2000, L, seed + 11 + k)
        c = c[~masked_by_oracle(c).any((1, 2))]
        clean.append(c)
        have += len(c)
        k += 1
        assert k <= 20, "control reads without a masked residue are too rare at %d bp" % L
    out = np.concatenate(clean)[:n].copy()
    for i in range(3, n, 10):
        out[i] = encode(periodic(r, L // 3 + 1), L, i % 3, r)
    return out


# ---- where the launch changes the kernel's form: the expression of mc_translate_launch (csrc/mc_stages.h) restated -----------
def launch_stages_reads(L):
    """True where the launch stages a workgroup's reads in LDS (while that costs no resident workgroup).  The GPU tests hold this
    against what the launch says it did (mc_debug_stage 5) at every length they run."""
    fp = ((L // 3 + 2) + 3) & ~3
    nlnf = max(fp + 2, 24)                                           # MC_TS_NLNF
    stride = (((fp + 76 + 3) >> 2) | 1) << 2                         # MC_TS_STRIDE
    stage = lambda l: (max(10 * l, 1488) + 15) & ~15                 # MC_TS_STAGE  # noqa: E731
    rest = nlnf * 8 + 64 * stride
    cu_lds = 160 * 1024 - 1024
    return cu_lds // (stage(L) + rest) >= cu_lds // (stage(0) + rest)


# staging costs a resident workgroup from 189 bp on; at 237 and 238 bp it is free once more (the direct form loses a workgroup
# there too), and from 239 bp on the launch never stages again
SWITCHES = [189, 237, 239]


# ---- the oracle's side -------------------------------------------------------------------------------------------------------
_lib = []


def oracle_lib():
    if not _lib:
        lib = C.CDLL(os.path.join(REPO, "oracle", "librapsearch_port.so"))
        lib.rs_translate6.restype = None
        lib.rs_translate6.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_int)]
        _lib.append(lib)
    return _lib[0]


def oracle_frames(reads):
    """rs_translate6() on every read: (n, 6, MC_FP) in the product's dense codes, MC_INV behind each frame's length, and the six
    frame lengths.  A code outside ORACLE_TO_DENSE and 0xA0 would be an error of the map: it raises."""
    lib = oracle_lib()
    n, L = reads.shape
    rows = np.full((n, 6, MC_FP), 0xA0, np.uint8)
    lens = (C.c_int * 6)()
    ptrs = (C.POINTER(C.c_uint8) * 6)()
    for i in range(n):
        for f in range(6):
            ptrs[f] = rows[i, f].ctypes.data_as(C.POINTER(C.c_uint8))
        lib.rs_translate6(reads[i].tobytes(), L, ptrs, lens)
        assert [lens[f] for f in range(6)] == [(L - f % 3) // 3 for f in range(6)]
    lut = np.full(256, 255, np.uint8)
    lut[0xA0] = MC_INV
    for k, v in ORACLE_TO_DENSE.items():
        lut[k] = v
    out = lut[rows]
    assert not (out == 255).any()
    return out, [(L - f % 3) // 3 for f in range(6)]


def blocks_of(masked_row):
    """Lengths of the runs of True in a 1-D boolean array."""
    d = np.diff(np.concatenate(([0], masked_row.astype(np.int8), [0])))
    return np.flatnonzero(d == -1) - np.flatnonzero(d == 1)


_AA64 = "FFLLSSSSYY..CC.WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"      # T, C, A, G = 0 .. 3


def translate6(reads):
    """The six frames before any masking, (n, 6, MC_FP) dense codes: what tells a masked residue from a stop or an unknown codon in
    the oracle's output (both are 0xA0 there).  Only the conditions on the sets use it, no comparison does."""
    n, L = reads.shape
    fwd = np.full(256, -1, np.int64)
    rc = np.full(256, -1, np.int64)
    for k, c in enumerate(b"TCAG"):
        fwd[c] = k
    for c, k in ((ord("A"), 0), (ord("G"), 1), (ord("T"), 2), (ord("U"), 2), (ord("C"), 3)):
        rc[c] = k
    dense = np.array([("ARNDCQEGHILKMFPSTWYV".index(a) if a != "." else MC_INV) for a in _AA64], np.uint8)
    out = np.full((n, 6, MC_FP), MC_INV, np.uint8)
    for f in range(6):
        o, m = f % 3, (L - f % 3) // 3
        idx = fwd[reads] if f < 3 else rc[reads[:, ::-1]]
        tri = idx[:, o:o + 3 * m].reshape(n, m, 3)
        cod = dense[(16 * tri[:, :, 0] + 4 * tri[:, :, 1] + tri[:, :, 2]) & 63]
        out[:, f, :m] = np.where((tri < 0).any(2), MC_INV, cod)
    return out


def check_conditions(L, reads, want, lens):
    """What a full set (make_reads with every family) must contain, on the oracle's output alone.  Returns the figures."""
    plain = translate6(reads)
    assert ((want == plain) | (want == MC_INV)).all()               # the oracle only ever replaces residues by the invalid code
    masked = (want == MC_INV) & (plain != MC_INV)
    blocks = [blocks_of(masked[i, f, :lens[f]]) for i in range(len(reads)) for f in range(6)]
    # SEG does not run on a frame under 8 residues (window 8 > n), so such frames cannot count against the share: from 26 bp on
    # every frame has 8, and the share is that of all residues; under 24 bp no frame has, and nothing may be masked at all
    able = [f for f in range(6) if lens[f] >= 8]
    total = sum(lens[f] for f in able) * len(reads)
    share = masked[:, able].sum() / total if able else 0.0
    ten = np.mean([len(b) >= 10 for b in blocks])
    big = sum(bool((b > 100).any()) for b in blocks)
    mid = sum(bool(((b >= 16) & (b <= 100)).any()) for b in blocks)
    if able:
        assert share >= 1 / 3, (L, share)
    else:
        assert not masked.any()
    if L >= 450:
        assert ten >= 0.01, (L, ten)
    if L >= 340:
        assert big >= 1, L
    if L >= 60:
        assert mid >= 1, L
    return share, ten, big, mid
