"""The cases of the tie bootstrap's unit tests, built in one place: tests/test_gpu_tieboot_units.py runs them on the device
(tests/emul/device_tieboot.hip) and tests/test_tieboot_host.py on the CPU (tests/emul/tieboot.cpp: the rules of csrc/mc_tieboot.h and the
walk of csrc/mc_ties.h under g++).  Both read the same files of sections (order_cases.write_sections) and are compared with
tests/tieboot_restated.py, whose answer is computed once per case.

A case: name, nseq, rows (an mc_row array), cuts (the row index behind each launch's last row), cut (the cut-offs), B, seed, scale (B
doubles), capacity (None: exactly the number of entries - the list is full to its last slot and nothing is dropped), launch (False: the
launches are handed no list) and idmap (None, or (perm, base): a row's query is a position, the read's id base + perm[query])."""
import numpy as np

import abundance_restated as R
import coverage_restated as V
import geneboot_cases as gc
import geneboot_restated as GR
import ties_cases as tc
import ties_restated as T
import tieboot_restated as TR

BS = gc.BS                              # (1, 63, 64, 65, 257, 4096)
PER_TILE = 64                           # mc_gb_per_tile of every case here: the fewest entries a tile has


def _case(name, nseq, spec, B, scale="plain", cuts=None, cut=None, seed=20240917, capacity=None, launch=True, idmap=None):
    rows = spec if isinstance(spec, np.ndarray) else tc.rows_of(spec)
    return {"name": name, "nseq": int(nseq), "rows": rows, "cuts": list(cuts) if cuts else [len(rows)], "cut": cut or {}, "B": int(B), "seed": int(seed),
            "scale": gc._scale(B, scale), "capacity": capacity, "launch": launch, "idmap": idmap}


def _k500():
    """read 3: 500 tied rows over 500 subjects, the limit - 2^32 = 500 x 8589934 + 296, the remainder to subject 499, the first row's;
    read 9: one row"""
    return [(3, 499 - k, 0, 5, 77.0) for k in range(500)] + [(9, 250, 0, 5)]


def _gaps():
    """7 genes; entries of genes 0, 2, 3 and 6 only: genes without entries between genes with entries, and at the end none"""
    spec = []
    for q in range(40):
        spec += [(2 * q, 0, 0, 5), (2 * q, 3, 0, 5)] if q % 3 == 0 else [(2 * q, 2, 0, 5), (2 * q, 6, 0, 5), (2 * q, 3, 0, 5)] if q % 3 == 1 else [(2 * q, 6, 0, 5)]
    return spec


def _one_gene():
    """gene 1 is in every tied set: alone, with gene 0 or with gene 2 - its slice has more entries than two tiles"""
    spec = []
    for q in range(200):
        spec += [(7 * q, 1, 0, 5)] if q % 3 == 0 else [(7 * q, 0, 0, 5), (7 * q, 1, 0, 5)] if q % 3 == 1 else [(7 * q, 1, 0, 5), (7 * q, 2, 0, 5), (7 * q, 1, 6, 9)]
    return spec


def _workgroups():
    """More than 256 reads over four workgroups of 256 threads.  Rows 0 .. 254: one read a row (k = 1).
    Row 255: read 255 begins at thread 255 of workgroup 0 with three tied rows (two of them in workgroup 1).  Rows 258 .. 511: reads whose
    one row names subject nseq - workgroup 1 has no read that adds anything.  Row 512: a read of two tied rows begins at thread 0 of
    workgroup 2; behind it reads of 1, 2 and 3 tied rows up to row 799, the last workgroup partly filled."""
    nseq = 6
    spec = [(q, q % nseq, 0, 5) for q in range(255)]
    spec += [(255, 4, 0, 5, 61.0), (255, 1, 0, 5, 61.0), (255, 5, 0, 5, 61.0)]
    spec += [(300 + k, nseq, 0, 5) for k in range(512 - 258)]
    q = 1000
    while len(spec) < 800:
        n = 2 if len(spec) == 512 else 1 + q % 3
        n = min(n, 800 - len(spec))
        spec += [(q, (q + j) % nseq, 0, 5, 58.0) for j in range(n)]
        q += 1
    assert len(spec) == 800 and spec[255][0] == 255 and spec[254][0] == 254 and spec[512][0] != spec[511][0] and spec[513][0] == spec[512][0]
    return nseq, spec


def cases():
    out = []
    for B in BS:                                                   # ties_cases' small shapes: k = 1, 2, 3, 6 and 7, a subject that ties twice, tied rows not adjacent, ...
        out.append(_case("b%d" % B, len(tc.B_LENGTHS), tc.B_ROWS, B, scale="holes" if B >= 63 else "plain", cut=tc.CUT))
    out.append(_case("k500", 500, _k500(), 64))
    out.append(_case("gaps", 7, _gaps(), 64))
    out.append(_case("one_gene", 3, _one_gene(), 64))
    nseq, spec = _workgroups()
    out.append(_case("workgroups", nseq, spec, 65))
    # three launches, the cuts between reads
    rows = tc.rows_of(tc.B_ROWS)
    cuts = [int(np.searchsorted(rows["query"], 5)), int(np.searchsorted(rows["query"], 10)), len(rows)]
    out.append(_case("launches", len(tc.B_LENGTHS), rows, 63, cuts=cuts, cut=tc.CUT))
    out.append(_case("m_one", len(tc.B_LENGTHS), tc.B_ROWS, 64, scale="one", cut=tc.CUT))
    out.append(_case("m_none", len(tc.B_LENGTHS), tc.B_ROWS, 65, scale="none", cut=tc.CUT))
    # no read ties (geneboot_cases' rows: a second, weaker row on some reads): the gene bootstrap's figures bit for bit
    out.append(_case("no_ties", 5, gc._mix(), 64))
    # capacity: one entry short; zero; the switch off (the launch is handed no list and must leave list memory as it was)
    for name, cap in (("short", -1), ("zero", 0)):
        c = _case(name, len(tc.B_LENGTHS), tc.B_ROWS, 64, cut=tc.CUT)
        c["capacity"] = len(expect(c)["q"]) + cap if cap else 0
        out.append(c)
    out.append(_case("off", len(tc.B_LENGTHS), tc.B_ROWS, 64, cut=tc.CUT, launch=False))
    # a class run's ids: the rows carry positions 0 .. 13, the ids are base + perm[position]
    perm = np.random.default_rng(5).permutation(40).astype(np.uint32)
    out.append(_case("idmap", len(tc.B_LENGTHS), tc.B_ROWS, 64, cut=tc.CUT, idmap=(perm, 123456)))
    return out


_EXPECT = {}


def expect(c):
    """the restatement's answer of a case, computed once and shared: q, s, share (the entries), k (per read), shares [nseq, B], stats
    [nseq, 6], m; counts: the gene bootstrap's replicate counts of the same rows; ab, ties: abundance_restated's and ties_restated's"""
    if c["name"] not in _EXPECT:
        rows8, rows6, nseq = V.rows_from_array(c["rows"]), R.rows_from_array(c["rows"]), c["nseq"]
        ids = None if c["idmap"] is None else (lambda pos, perm=c["idmap"][0], base=c["idmap"][1]: base + int(perm[pos]))
        q, s, sh, ks = TR.entries(rows8, nseq, ids=ids, **c["cut"])
        cs = TR.shares(q, s, sh, nseq, c["B"], c["seed"])
        gq, gs = GR.assignments(rows6, nseq, **c["cut"])
        if ids is not None:
            gq = np.array([ids(x) for x in gq.tolist()], np.int64)
        _EXPECT[c["name"]] = {"q": q, "s": s, "share": sh, "k": ks, "shares": cs, "stats": TR.stats(cs, c["scale"]), "m": int(TR.used(c["scale"]).sum()),
                              "counts": GR.counts(gq, gs, nseq, c["B"], c["seed"]), "gq": gq, "gs": gs,
                              "ab": R.abundance(rows6, max(nseq, int(c["rows"]["subject"].max()) + 1), **c["cut"]), "ties": T.ties(rows8, [1] * nseq, **c["cut"])}
    return _EXPECT[c["name"]]


def capacity(c):
    return len(expect(c)["q"]) if c["capacity"] is None else c["capacity"]


def sections_in(c):
    pars = np.zeros(1, tc.PARS)
    cut = c["cut"]
    pars[0] = (cut.get("min_ident", 0), cut.get("min_aln", 0), cut.get("min_bits", 0.0), cut.get("max_loge", 1.0))
    meta = np.int32([c["nseq"], c["B"], capacity(c), 1 if c["launch"] else 0])
    perm, base = c["idmap"] if c["idmap"] is not None else (np.zeros(0, np.uint32), 0)
    return [pars, meta, c["rows"], np.array(c["cuts"], np.uint32), c["scale"], np.array([c["seed"]], np.uint64), np.asarray(perm, np.uint32), np.array([base], np.int64)]


def entry_set(q, s, share):
    """the entries as a sorted list of (q, gene, share): a multiset"""
    return sorted(zip(np.asarray(q).tolist(), np.asarray(s).tolist(), np.asarray(share).tolist()))


def compare(c, shares, stats):
    """shares [nseq x B] and stats [nseq x 6] of a run of case c - from the device or the CPU build - against the restatement: the
    integers exactly, the doubles bit for bit; then the statement's invariants"""
    e = expect(c)
    shares = np.asarray(shares, np.uint64).reshape(c["nseq"], c["B"])
    stats = np.asarray(stats, np.float64).reshape(c["nseq"], 6)
    assert np.array_equal(shares, e["shares"]), "replicate shares: first difference at %s" % (np.argwhere(shares != e["shares"])[:1].tolist(),)
    assert GR.same_bits(stats, e["stats"]), "the six doubles: first difference at %s" % (np.argwhere(stats.view(np.uint64) != e["stats"].view(np.uint64))[:1].tolist(),)
    invariants(c, shares, stats)
    return e


def invariants(c, shares, stats):
    """the statement's two invariants on a share matrix and its six doubles: the shares of every replicate add up to 2^32 x the gene
    bootstrap's counts; a case without a tied read IS the gene bootstrap: cs = c x 2^32 and the doubles are its doubles, bit for bit"""
    e = expect(c)
    total = [sum(int(v) for v in shares[:, b]) for b in range(c["B"])]                 # (Python integers: 2^32 x the counts may pass 2^63)
    assert total == [int(v) * TR.ONE for v in e["counts"].sum(axis=0)], "the shares of a replicate do not add up to 2^32 x its counts"
    nocand = e["ties"]["candidates"] == 0
    assert not shares[nocand].any()
    if e["m"] == 0:
        assert np.isnan(stats).all()
    else:
        assert not stats[nocand].any() and (stats[:, 2] <= stats[:, 3]).all() and (stats[:, 3] <= stats[:, 4]).all() and (stats[:, 4] <= stats[:, 5]).all()
    if max(e["k"], default=1) == 1:
        assert np.array_equal(shares, e["counts"].astype(np.uint64) << np.uint64(32)), "no read ties, and cs is not c x 2^32"
        assert GR.same_bits(stats, GR.stats(e["counts"], c["scale"])), "no read ties, and the six doubles are not the gene bootstrap's"
