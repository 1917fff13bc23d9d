"""The cases of the gene bootstrap's unit tests, built in one place: tests/test_gpu_geneboot_units.py runs them on the device
(tests/emul/device_geneboot.hip) and tests/test_geneboot_host.py on the CPU (tests/emul/geneboot.cpp: the rules of csrc/mc_geneboot.h
under g++).  Both read the same files of sections (order_cases.write_sections) and are compared with tests/geneboot_restated.py, whose
answer is computed once per case.

A case: name, nseq, rows (an mc_row array), cuts (the row index behind each launch's last row), cut (the cut-offs), B, seed, scale
(B doubles) and capacity (None: exactly the number of assigned reads - the list is full to its last slot and nothing is dropped)."""
import numpy as np

import abundance_restated as R
import curve_cases as cc
import geneboot_restated as GR

BS = (1, 63, 64, 65, 257, 4096)         # replicate tiles of 64 and one over; a sort padded from one over a power of two; the limits


def _scale(B, kind, seed=1):
    rng = np.random.default_rng(1000 * B + seed)
    s = rng.uniform(0.5, 2.0, B) * 2.0 ** rng.integers(-30, 5, B)
    if kind == "holes":                                            # NaN, 0, negative and infinite entries: m < B
        for k, bad in zip(range(0, B, 3), [np.nan, 0.0, -1.5, np.inf, -0.0, -np.inf] * B):
            s[k] = bad
    elif kind == "one":
        s[:] = np.nan
        s[B // 2] = 0.375
    elif kind == "none":
        s[:] = np.nan
        s[1::2] = 0.0
    elif kind == "constant":
        s[:] = 0.5
    return s.astype(np.float64)


def _case(name, nseq, spec, B, scale="plain", cuts=None, cut=None, seed=20240917, capacity=None, launch=True):
    rows = spec if isinstance(spec, np.ndarray) else cc.rows_of(spec)
    return {"name": name, "nseq": int(nseq), "rows": rows, "cuts": list(cuts) if cuts else [len(rows)], "cut": cut or {}, "B": int(B), "seed": int(seed),
            "scale": _scale(B, scale), "capacity": capacity, "launch": launch}


def _mix(nseq=5, n=45, first=0):
    """reads of the even genes (the odd ones have none), with reads without rows between them and a second, weaker row on some"""
    spec = []
    for k in range(n):
        q = first + 2 * k + (k % 3 == 0)
        g = 2 * (k % 3) if 2 * (k % 3) < nseq else 0
        spec.append((q, g, k % 20, k % 20 + 25, 50.0 + k % 7))
        if k % 4 == 1:
            spec.append((q, (g + 1) % nseq, 0, 20, 30.0))
    return spec


def cases():
    out = []
    for B in BS:
        out.append(_case("b%d" % B, 5, _mix(), B, scale="holes" if B >= 63 else "plain"))
    for nseq in (1, 3, 4, 5):                                       # genes without reads between genes with reads (from three genes on)
        out.append(_case("genes%d" % nseq, nseq, _mix(nseq, 20 + nseq), 64))
    # one gene holds every read, and more entries than two tiles
    n = 200
    assert GR.per_tile(n, 64) == 64
    out.append(_case("one_gene", 3, [(7 * k, 1, 0, 30) for k in range(n)], 64))
    # a tile boundary exactly on a gene boundary: 64 reads of gene 0, none of gene 1, 64 of gene 2, 7 of gene 3; two replicate tiles
    assert GR.per_tile(135, 65) == 64
    spec = sorted([(3 * k, 0, 0, 30) for k in range(64)] + [(3 * k + 1, 2, 0, 30) for k in range(64)] + [(3 * k + 2, 3, 0, 30) for k in range(7)])
    out.append(_case("boundary", 4, spec, 65))
    # three launches with cuts between reads: reads that straddle a workgroup boundary, a top row that fails a cut-off, a tie, a read with no
    # passing row, subjects not below nseq (curve_cases' rows); then a non-zero first id; then the largest id
    rows, lengths = cc._straddle_case()
    more = cc.rows_of([(5000 + k, k % 4, 0, 30) for k in range(9)])
    last = cc.rows_of([(2 ** 31 - 3, 1, 0, 30), (2 ** 31 - 1, 3, 0, 30, 60.0), (2 ** 31 - 1, 2, 0, 30, 61.0)])
    allrows = np.concatenate([rows, more, last])
    for cut in ({}, dict(min_ident=60, min_aln=25)):
        out.append(_case("launches_%d" % len(cut), len(lengths), allrows, 63, cuts=[len(rows), len(rows) + len(more), len(allrows)], cut=cut))
    out.append(_case("m_one", 5, _mix(), 64, scale="one"))
    out.append(_case("m_none", 5, _mix(), 65, scale="none"))
    # equal values across replicates: a constant scale and small, tied counts
    out.append(_case("tied", 3, [(0, 0, 0, 30), (1, 0, 0, 30), (5, 2, 0, 30)], 257, scale="constant"))
    # capacity one short of the assigned reads: dropped == 1 and nothing behind the list
    short = _case("short", 5, _mix(), 64)
    short["capacity"] = len(expect(short)["q"]) - 1
    out.append(short)
    # the switch off: the launch is handed no list and must leave list memory as it was
    out.append(_case("off", 5, _mix(), 64, launch=False))
    return out


_EXPECT = {}


def expect(c):
    """the restatement's answer of a case, computed once and shared: q, s (the assigned reads), counts [nseq, B], stats [nseq, 6], m, and
    abundance_restated's count table"""
    if c["name"] not in _EXPECT:
        rows = R.rows_from_array(c["rows"])
        q, s = GR.assignments(rows, c["nseq"], **c["cut"])
        cm = GR.counts(q, s, c["nseq"], c["B"], c["seed"])
        ab = R.abundance(rows, max(c["nseq"], int(c["rows"]["subject"].max()) + 1), **c["cut"])
        _EXPECT[c["name"]] = {"q": q, "s": s, "counts": cm, "stats": GR.stats(cm, c["scale"]), "m": int(GR.used(c["scale"]).sum()), "ab": ab}
    return _EXPECT[c["name"]]


def capacity(c):
    return len(expect(c)["q"]) if c["capacity"] is None else c["capacity"]


def sections_in(c):
    pars = np.zeros(1, cc.PARS)
    cut = c["cut"]
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    meta = np.int32([c["nseq"], c["B"], capacity(c), 1 if c["launch"] else 0])
    return [pars, meta, c["rows"], np.array(c["cuts"], np.uint32), c["scale"], np.array([c["seed"]], np.uint64)]


def compare(c, counts, stats):
    """counts [nseq x B] and stats [nseq x 6] of a run of case c - from the device or the CPU build - against the restatement: the
    integers exactly, the doubles bit for bit; then the statement's invariants"""
    e = expect(c)
    counts = np.asarray(counts, np.int64).reshape(c["nseq"], c["B"])
    stats = np.asarray(stats, np.float64).reshape(c["nseq"], 6)
    assert np.array_equal(counts, e["counts"]), "replicate counts: first difference at %s" % (np.argwhere(counts != e["counts"])[:1].tolist(),)
    assert GR.same_bits(stats, e["stats"]), "the six doubles: first difference at %s" % (np.argwhere(stats.view(np.uint64) != e["stats"].view(np.uint64))[:1].tolist(),)
    import boot_restated as br
    w = br.weights(c["seed"], np.arange(c["B"], dtype=np.uint64)[:, None], e["q"].astype(np.uint64)[None, :]) if len(e["q"]) else np.zeros((c["B"], 0), np.int64)
    assert np.array_equal(counts.sum(axis=0), w.sum(axis=1)), "the sum over the genes is not the sum of the assigned reads' weights"
    noreads = np.bincount(e["s"], minlength=c["nseq"]) == 0
    assert not counts[noreads].any()
    if e["m"] == 0:
        assert np.isnan(stats).all()
    else:
        assert not stats[noreads].any() and (stats[:, 2] <= stats[:, 3]).all() and (stats[:, 3] <= stats[:, 4]).all() and (stats[:, 4] <= stats[:, 5]).all()
    return e
