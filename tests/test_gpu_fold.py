"""Long genes end to end on the GPU (csrc/mc_fold.h, csrc/k_fold.h, abundance.split_genes, gene_abundance.py --long-genes).

(a) Split against unsplit: the golden example reads against every second packaged marker - 8,359 genes, every one of at most 2,047 residues,
525 of them longer than 768 (all 16,717 markers cut at (768, 512) put more than 2,047 postings into one seed bucket and the engine refuses
them: the overlaps add postings, README) - searched once as they are and once cut by split_genes(seg_len=768, overlap=V), the engine opened on the segments with the genes' statistics and the fold
set; both with ties and coverage.  The figures that do not depend on the row order among tied genes are equal integer for integer, and the
split run's own tables are exactly what abundance_restated and coverage_restated make of its host rows folded in numpy.
(b) A FASTA with one synthetic gene of about 3,000 residues, three markers joined: refused without the switch; with it the gene is counted
as one, its unique reads are those of the three markers, and its coverage reaches into all three parts."""
import os

import numpy as np
import pytest

import abund_inputs as AI
import abundance_table_cases as TC
import abundance_restated as R
import coverage_restated as CV
import fold_restated as FR
import order_cases as oc
import ties_restated as TR
from microbecensus_amd import _native, abundance

pytestmark = pytest.mark.gpu

SEG = 768
CUT = dict(min_ident=0, min_aln=0, min_bits=0.0)


def _run(eng, reads, rows=False):
    eng.set_run(100)
    eng.set_abundance(True, **CUT)
    eng.set_coverage(True)
    eng.set_ties(True)
    got = eng.search(reads)[0].copy() if rows else eng.search(reads) and None
    out = {"ab": eng.abundance(), "cov": eng.coverage(), "ti": eng.ties(), "tcov": eng.ties_coverage(), "rows": got}
    return out


@pytest.fixture(scope="module")
def runs():
    names, seqs = TC.long_gene_markers()
    reads = AI.example_reads()
    sp = abundance.split_genes(names, seqs, seg_len=SEG, overlap=FR.V)
    eng = _native.Engine(device=0, names=names, seqs=seqs, marker_family=[0] * len(names), nfam=1)
    try:
        un = _run(eng, reads, rows=True)
    finally:
        eng.close()
    eng = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * len(sp["seg_names"]), nfam=1, stats=sp["stats"])
    try:
        eng.set_gene_fold(sp["seg_gene"], sp["seg_off"], sp["gene_len"])
        assert eng.abundance_count() == len(names)
        split = _run(eng, reads, rows=True)
        split["fold"] = eng.gene_fold_stats()
    finally:
        eng.close()
    return {"names": names, "seqs": seqs, "sp": sp, "un": un, "split": split}


def test_split_against_unsplit_the_order_free_figures_are_equal(runs):
    un, sp, fold = runs["un"], runs["split"], runs["split"]["fold"]
    print("genes %d, split %d, segments %d; assigned %d / %d, ambiguous %d / %d, edge_rows %d, k_fold %.3f ms, rows %d / %d" % (
        len(runs["names"]), runs["sp"]["genes_split"], len(runs["sp"]["seg_names"]), un["ab"]["assigned"], sp["ab"]["assigned"], un["ti"]["ambiguous"], sp["ti"]["ambiguous"],
        fold["edge_rows"], fold["ms"], len(un["rows"]), len(sp["rows"])))
    assert runs["sp"]["genes_split"] >= 20 and fold["ngenes"] == len(runs["names"])
    for k in ("unique", "candidates", "share"):
        bad = np.flatnonzero(un["ti"][k] != sp["ti"][k])
        print("%s: %d genes differ %s" % (k, len(bad), [(runs["names"][g], int(un["ti"][k][g]), int(sp["ti"][k][g])) for g in bad[:10]]))
    bad = np.flatnonzero(un["tcov"]["covered_any"] != sp["tcov"]["covered_any"])
    print("covered_any: %d genes differ %s" % (len(bad), [(runs["names"][g], int(un["tcov"]["covered_any"][g]), int(sp["tcov"]["covered_any"][g])) for g in bad[:10]]))
    assert un["ab"]["assigned"] == sp["ab"]["assigned"] and un["ab"]["searched"] == sp["ab"]["searched"], "reads_assigned"
    assert un["ti"]["ambiguous"] == sp["ti"]["ambiguous"], "reads_ambiguous"
    assert np.array_equal(un["ti"]["unique"], sp["ti"]["unique"]), "unique_reads"
    assert np.array_equal(un["ti"]["candidates"], sp["ti"]["candidates"]), "candidate_reads"
    # shared_reads: a read tied among k genes gives each floor(2^32 / k) units and the remainder, 2^32 mod k < k units of 2^-32, to the
    # FIRST tied gene in row order (csrc/mc_ties.h, "floor(2^32 / k) to every tied subject"; ties_restated.ties: share[members[0][0]] += ONE - k * each) -
    # the one part of the tie accounting that does depend on the row order among tied genes.  So: the sum is exact, and a gene differs by no
    # more than the remainders of the tied sets it is in.  The reads concerned are printed and held to at most 1 % of the assigned reads.
    sets = TR.tied_sets(CV.rows_from_array(un["rows"]), len(runs["names"]), **CUT)
    rec = FR.records(runs["sp"]["gene_len"], SEG, FR.V)[0]
    first_split = {q: members[0][0] for q, members in TR.tied_sets(CV.rows_from_array(FR.fold(sp["rows"], rec)), len(runs["names"]), **CUT)}
    slack, moved = np.zeros(len(runs["names"]), np.int64), 0
    for q, members in sets:
        rem = TR.ONE - len(members) * (TR.ONE // len(members))
        moved += rem > 0 and first_split.get(q) != members[0][0]          # (the reads whose remainder went to another gene of the same tied set)
        for g, _, _ in members:
            slack[g] += rem
    diff = un["ti"]["share"].astype(np.int64) - sp["ti"]["share"].astype(np.int64)
    print("shared_reads: %d reads placed their remainder on another gene (%.2f %% of the assigned), %d genes differ, by at most %d units of 2^-32" % (
        moved, 100.0 * moved / un["ab"]["assigned"], int((diff != 0).sum()), int(np.abs(diff).max())))
    assert int(un["ti"]["share"].sum()) == int(sp["ti"]["share"].sum()) and (np.abs(diff) <= slack).all() and moved <= 0.01 * un["ab"]["assigned"], "shared_reads"
    assert np.array_equal(un["tcov"]["covered_any"], sp["tcov"]["covered_any"]), "covered_any_aa"


def test_the_split_runs_tables_are_the_restatements_of_its_folded_rows(runs):
    """reads, aligned_aa and covered_aa depend on the row order among tied genes: the split run is held to its OWN rows, folded in numpy"""
    sp, spl = runs["sp"], runs["split"]
    rec = FR.records(sp["gene_len"], SEG, FR.V)[0]
    assert np.array_equal(rec["gene"], sp["seg_gene"]) and np.array_equal(rec["off"], sp["seg_off"])
    folded = FR.fold(spl["rows"], rec)
    assert len(folded) and folded["subject"].max() < len(runs["names"]) and FR.edge_rows(spl["rows"], rec) == spl["fold"]["edge_rows"]
    ab = R.abundance(R.rows_from_array(folded), len(runs["names"]), **CUT)
    assert np.array_equal(ab["reads"], spl["ab"]["reads"]) and np.array_equal(ab["aligned"], spl["ab"]["aligned"]) and ab["assigned"] == spl["ab"]["assigned"]
    cov = CV.coverage(CV.rows_from_array(folded), sp["gene_len"], **CUT)
    assert np.array_equal(cov["covered"], spl["cov"]["covered"]) and np.array_equal(cov["spanned"], spl["cov"]["spanned"])
    # the same alignments, the same statistics: every row of the unsplit run is among the folded rows, bits and loge included
    # Left out: the reads that hold MC_MAX_M8 = 500 rows in either run - the engine keeps a read's first 500 rows (rapsearch -v 500,
    # csrc/mc_core.h "#define MC_MAX_M8 500"), the overlaps add rows of their own, so WHICH 500 survive depends on the database's layout.
    # They are printed and held to at most 1 % of the assigned reads.
    full = {int(q) for r in (runs["un"]["rows"], folded) for q, n in zip(*np.unique(r["query"], return_counts=True)) if n >= oc.MAX_M8}
    key = lambda r: {k for k in zip(*(r[f].tolist() for f in ("query", "subject", "sstart", "send", "alnlen", "nmatch", "bits", "loge"))) if k[0] not in full}
    missing = key(runs["un"]["rows"]) - key(folded)
    print("rows of the unsplit run that the folded rows lack: %d of %d; reads at the 500-row cap, left out: %s (%.2f %% of the assigned reads)" % (
        len(missing), len(runs["un"]["rows"]), sorted(full), 100.0 * len(full) / spl["ab"]["assigned"]))
    assert not missing and len(full) <= 0.01 * spl["ab"]["assigned"]


def test_three_markers_joined_are_counted_as_one_long_gene(runs, tmp_path):
    names, seqs, un = runs["names"], runs["seqs"], runs["un"]
    # three markers of about 1,000 residues with the most unique reads
    order = TC.pick_joined(seqs, un["ti"]["unique"])
    assert len(order) == 3 and all(un["ti"]["unique"][g] > 0 for g in order)
    assert [names[g] for g in order] == TC.recorded()["long_joined"]         # (the `long` case of the recorded tables joins the same three)
    genes, joined, keep = TC.write_joined_genes(tmp_path / "genes.faa", names, seqs, order)
    assert 2400 <= len(joined) <= 3549
    fq = os.path.join(AI.GOLD, "inputs", "example.fq.gz")
    base = {"seqfiles": [fq], "genes": genes, "nreads": 10000, "read_length": 100, "device": 0, "ags": 3.0e6, "ties": True, "coverage": True, "depth_out": str(tmp_path / "depth.tsv")}
    with pytest.raises(abundance.AbundanceError, match="Gene joined is %d residues long: longer than 2047" % len(joined)):
        abundance.run_abundance(dict(base, outfile=str(tmp_path / "off.tsv")))
    table, args = abundance.run_abundance(dict(base, outfile=str(tmp_path / "on.tsv"), long_genes=True))
    header, body = abundance.read_table(str(tmp_path / "on.tsv"))
    assert header["long_genes"] == "on" and header["genes_split"] == "1" and int(header["segments"]) == len(keep) + len(FR.segments(len(joined))) and "edge_rows" in header
    assert table["gene"][0] == "joined" and int(table["length_aa"][0]) == len(joined) and len(table["gene"]) == len(keep) + 1 and body[0][0] == "joined"
    # the reads whose tied set lies within the three markers (one of them, or several of them) in the unsplit run of the example reads
    sets = TR.tied_sets(CV.rows_from_array(un["rows"]), len(names), **CUT)
    want = sum(1 for q, members in sets if {s for s, _, _ in members} <= set(order))
    print("joined: %d residues, reads %d, unique %d, the three markers' own %d %s, covered %d, edge_rows %s" % (
        len(joined), table["reads"][0], table["unique_reads"][0], want, [int(un["ti"]["unique"][g]) for g in order], table["covered_aa"][0], header["edge_rows"]))
    assert int(table["unique_reads"][0]) == want and int(table["reads"][0]) >= want
    depth, at = table["depth"][:len(joined)], 0
    for g in order:
        assert depth[at:at + len(seqs[g])].any(), "no read covers the part of marker %s" % names[g]
        at += len(seqs[g])
    assert int(table["covered_aa"][0]) == int((depth > 0).sum())


def test_set_gene_fold_refuses_naming_the_value():
    """mc_set_gene_fold on a small engine: a map that does not ascend, an offset off its step, lengths that do not fit the segments, a gene
    beyond 65,535 residues, the counts on with tables of another size; and off again, the tables are the index's"""
    rng = np.random.default_rng(17)
    lens = [50, 2000, 100]
    seqs = ["".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), n)) for n in lens]
    sp = abundance.split_genes(["a", "b", "c"], seqs)
    nsegs = len(sp["seg_names"])
    assert nsegs == 5 and sp["seg_off"].tolist() == [0, 0, 680, 1360, 0]
    eng = _native.Engine(device=0, names=sp["seg_names"], seqs=sp["seg_seqs"], marker_family=[0] * nsegs, nfam=1, stats=sp["stats"])
    try:
        sg, so, gl = sp["seg_gene"], sp["seg_off"], sp["gene_len"]
        for bad, text in (((np.int32([1, 0, 0, 0, 2]), so, gl), r"seg_gene\[0\] = 1 behind gene -1: the map does not ascend"),
                          ((np.int32([0, 2, 2, 2, 2]), so, gl), r"seg_gene\[1\] = 2 behind gene 0"),
                          ((sg, np.int32([0, 0, 680, 1361, 0]), gl), r"seg_off\[3\] = 1361 is not 2 steps of 680 into gene 1"),
                          ((sg, np.int32([0, 5, 680, 1360, 0]), gl), r"seg_off\[1\] = 5 is not 0 steps"),
                          ((sg, so, np.int32([50, 2001, 100])), r"segment 3 of 640 residues at seg_off 1360 does not fit gene 1 of gene_len 2001"),
                          ((sg, so, np.int32([50, 65536, 100])), r"gene_len\[1\] = 65536 lies outside 1 .. 65535"),
                          ((sg, so, np.int32([50, 2000])), r"seg_gene\[4\] = 2 lies outside 0 .. 1")):
            with pytest.raises(RuntimeError, match=text):
                eng.set_gene_fold(*bad)
            assert eng.gene_fold_stats()["ngenes"] == 0 and eng.abundance_count() == nsegs
        eng.set_run(100)
        eng.set_abundance(True)
        with pytest.raises(RuntimeError, match="abundance counting is on with tables of 5 sequences and 3174 residues, the fold asks for 3 and 2150"):
            eng.set_gene_fold(sg, so, gl)
        eng.set_abundance(False)
        eng.set_gene_fold(sg, so, gl)
        assert eng.gene_fold_stats() == {"ngenes": 3, "edge_rows": 0, "ms": 0.0} and eng.abundance_count() == 3
        eng.set_abundance(True)
        eng.set_coverage(True)
        assert len(eng.abundance()["reads"]) == 3 and len(eng.coverage_depth()) == 2150
        with pytest.raises(RuntimeError, match="abundance counting is on with tables of 3 sequences and 2150 residues, the fold asks for 5 and 3174"):
            eng.set_gene_fold(None)
        eng.set_abundance(False)
        eng.set_gene_fold(None)
        assert eng.gene_fold_stats()["ngenes"] == 0 and eng.abundance_count() == nsegs
    finally:
        eng.close()
