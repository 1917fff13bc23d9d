"""The cases of the group bootstrap's unit tests, built in one place on top of tests/geneboot_cases.py' rows: tests/test_gpu_groupboot_units.py
runs them on the device (tests/emul/device_groupboot.hip) and tests/test_groupboot_host.py on the CPU (tests/emul/groupboot.cpp: the rules
of csrc/mc_groupboot.h under g++).  Both are compared with tests/groupboot_restated.py, whose answer is computed once per case.

A case is a gene-bootstrap case (geneboot_cases._case: nseq, rows, B, seed, scale) plus group_of (int32 per gene), ngroups, gene_kb
(float64 per gene, 3 x length_aa / 1000) and counts_first: whether the owner's FIRST call asks for the group replicate counts (its second call, behind a gene
bootstrap, asks the opposite: both output forms and both calling orders in every case)."""
import numpy as np

import geneboot_cases as gc
import geneboot_restated as GR
import groupboot_restated as GRR

BS = gc.BS                              # 1, 63, 64, 65, 257, 4096: geneboot_cases' replicate tiles and sort paddings
LEN_SHORT, LEN_LONG = 1, 65535          # a 1-residue and a 65,535-residue gene: gene_kb 0.003 and 196.605


def _rows(per_gene):
    """reads of the genes: per_gene[s] reads of gene s, the genes' reads interleaved by ascending read id"""
    spec, q = [], 0
    for k in range(max(per_gene)):
        for s, n in enumerate(per_gene):
            if k < n:
                spec.append((q, s, k % 20, k % 20 + 25, 50.0 + k % 7))
                q += 1 + (k + s) % 3
    return spec


def _lengths(nseq, seed):
    """gene lengths of 1 .. 65,535 residues"""
    return np.random.default_rng(77 + seed).integers(1, 65536, nseq)


def gene_kb(length_aa):
    """as the front end passes it: 3 x length_aa / 1000"""
    return 3.0 * np.asarray(length_aa, dtype=np.float64) / 1000.0


def _case(name, per_gene, group_of, B, scale="plain", lengths=None, counts_first=True):
    nseq = len(per_gene)
    c = gc._case("grp_" + name, nseq, _rows(per_gene), B, scale=scale)
    group_of = np.asarray(group_of, np.int32)
    assert len(group_of) == nseq and group_of.min() == 0 and set(group_of.tolist()) == set(range(int(group_of.max()) + 1))
    c.update({"group_of": group_of, "ngroups": int(group_of.max()) + 1, "length_aa": np.asarray(lengths if lengths is not None else _lengths(nseq, B), np.int64), "counts_first": bool(counts_first)})
    c["gene_kb"] = gene_kb(c["length_aa"])
    return c


def cases():
    out = []
    for k, B in enumerate(BS):          # genes 0, 1, 2, 4, 5 with reads, 3 without; three groups that interleave; unused replicates from 63 on
        out.append(_case("b%d" % B, [9, 4, 7, 0, 12, 3], [0, 1, 0, 1, 2, 2], B, scale="holes" if B >= 63 else "plain", counts_first=k % 2 == 0))
    # one group holds every gene (ngroups == 1): the serial walk over all members, one of them without reads
    out.append(_case("one_group", [5, 0, 8, 3, 6], [0, 0, 0, 0, 0], 65))
    # every gene its own group (ngroups == nseq), one of them without reads
    out.append(_case("singletons", [5, 0, 8, 3, 6], [0, 1, 2, 3, 4], 64, counts_first=False))
    # two groups whose members interleave in gene order, all with reads
    out.append(_case("interleave", [4, 6, 5, 7, 3, 9], [0, 1, 0, 1, 0, 1], 65))
    # a group whose members all have no reads, between two that have
    out.append(_case("empty_between", [6, 0, 0, 5, 4], [0, 1, 1, 2, 2], 64))
    # a group of one member with reads and four without, beside another group
    out.append(_case("one_of_five", [0, 0, 7, 0, 0, 5], [0, 0, 0, 0, 0, 1], 64, counts_first=False))
    # a group of 70 members with reads - more than a wave's worth - beside a group of five
    out.append(_case("seventy", [1 + k % 4 for k in range(75)], [0] * 35 + [1] * 5 + [0] * 35, 65, scale="holes"))
    # no used replicate, and one
    out.append(_case("m_none", [9, 4, 7, 0, 12, 3], [0, 1, 0, 1, 2, 2], 65, scale="none"))
    out.append(_case("m_one", [9, 4, 7, 0, 12, 3], [0, 1, 0, 1, 2, 2], 64, scale="one", counts_first=False))
    # gene_kb of 0.003 and 196.605 in one group of four: terms of very different magnitudes, so that the addition order shows in the bits
    out.append(_case("kb_mixed", [40, 3, 17, 29], [0, 0, 0, 0], 64, lengths=[LEN_SHORT, LEN_LONG, 100, 1000]))
    return out


_EXPECT = {}


def expect(c):
    """the restatement's answer of a case, computed once and shared: the gene case's (geneboot_cases.expect) plus y and C [ngroups, B], stats
    [ngroups, 6], live (the groups with reads, ascending) and the plan"""
    if c["name"] not in _EXPECT:
        e = dict(gc.expect(c))
        e["y"], e["C"] = GRR.values(e["counts"], c["scale"], c["group_of"], c["ngroups"], c["gene_kb"])
        e["gstats"] = GRR.stats(e["y"], c["scale"])
        e["reads"] = np.bincount(e["s"], minlength=c["nseq"])
        e["plan"] = GRR.plan(e["reads"], c["group_of"], c["ngroups"], c["gene_kb"])
        e["live"] = np.flatnonzero(e["plan"][0] >= 0)
        _EXPECT[c["name"]] = e
    return _EXPECT[c["name"]]


def sections_in(c):
    """the gene harness' sections (geneboot_cases.sections_in) and behind them group_of, (ngroups, counts_first) and gene_kb"""
    return gc.sections_in(c) + [c["group_of"], np.int32([c["ngroups"], 1 if c["counts_first"] else 0]), c["gene_kb"]]


def compare(c, y, C, stats):
    """y and C [ngroups x B] (either may be None: not asked for) and stats [ngroups x 6] of a run of case c - from the device or the CPU
    build - against the restatement: the integers exactly, the doubles bit for bit; then the statement's invariants"""
    e = expect(c)
    ng, B = c["ngroups"], c["B"]
    stats = np.asarray(stats, np.float64).reshape(ng, 6)
    if C is not None:
        C = np.asarray(C, np.int64).reshape(ng, B)
        assert np.array_equal(C, e["C"]), "group replicate counts: first difference at %s" % (np.argwhere(C != e["C"])[:1].tolist(),)
        assert np.array_equal(C.sum(axis=0), e["counts"].sum(axis=0)), "the sum over the groups is not the sum over the genes"
    if y is not None:
        y = np.asarray(y, np.float64).reshape(ng, B)
        assert GR.same_bits(y, e["y"]), "group replicate values: first difference at %s" % (np.argwhere(y.view(np.uint64) != e["y"].view(np.uint64))[:1].tolist(),)
    assert GR.same_bits(stats, e["gstats"]), "the six doubles: %s against %s" % (stats.tolist(), e["gstats"].tolist())
    dead = e["plan"][0] < 0
    if e["m"] == 0:
        assert np.isnan(stats).all()
    else:
        assert not stats[dead].any() and (stats[:, 2] <= stats[:, 3]).all() and (stats[:, 3] <= stats[:, 4]).all() and (stats[:, 4] <= stats[:, 5]).all()
    return e
