"""Long genes, host side (no GPU): the segmenter of abundance.split_genes and of csrc/mc_fold.h (g++ build, tests/emul/fold.cpp) against
the numpy statement (tests/fold_restated.py) - cover, overlap, the segment argument exhaustively at a small size -, the fold of rows and the
edge rows of the g++ build against numpy, the statistics pair of the host index (tests/emul/fold_tables.cpp), every refusal before an engine
is opened, the tables with the switch off byte for byte, and the new symbols of the ABI."""
import os
import subprocess

import numpy as np
import pytest

import fold_restated as FR
import order_cases as oc
from microbecensus_amd import _native, abundance
from microbecensus_amd._native import ROW_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
S = FR.L - FR.V
LENGTHS = sorted({1, 2047, 2048, 2047 + S, 2047 + S + 1, 65535, FR.L - 1, FR.L, FR.L + 1, FR.L + S, FR.L + S + 1, FR.L + 2 * S, FR.L + 2 * S + 1})


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fold") / "fold")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "emul", "fold.cpp")])
    return exe


def _emul_segments(exe, seg_len, overlap, lengths):
    out = {}
    for line in subprocess.check_output([exe, "segs", str(seg_len), str(overlap)] + [str(x) for x in lengths], text=True).splitlines():
        c = line.split()
        out[int(c[0])] = [tuple(int(x) for x in s.split(":")) for s in c[2:]]
        assert len(out[int(c[0])]) == int(c[1])
    return out


def test_constants_are_stated_once(emul):
    got = [int(x) for x in subprocess.check_output([emul, "consts"], text=True).split()]
    assert got[:4] == [FR.L, FR.V, FR.MAX_GENE, FR.MAX_SEGS] == [abundance.SEG_LEN, abundance.SEG_OVERLAP, abundance.MAX_LONG_GENE_LEN, abundance.MAX_SEGMENTS]
    assert FR.V % 64 == 0 and FR.V >= 3 * got[4] and FR.V - 64 < 3 * got[4] and FR.MAX_GENE == 65535 and FR.MAX_SEGS == 32767 and 0 < S


@pytest.mark.parametrize("seg_len,overlap", [(FR.L, FR.V), (768, FR.V), (13, 5)])
def test_segments_cover_the_gene_and_overlap_by_exactly_v(emul, seg_len, overlap):
    lengths = LENGTHS if seg_len > 13 else list(range(1, 80))
    cxx = _emul_segments(emul, seg_len, overlap, lengths)
    for n in lengths:
        sg = FR.segments(n, seg_len, overlap)
        assert [o for o, _ in sg] == abundance.segment_offsets(n, seg_len, overlap) == [s[0] for s in cxx[n]] and [m for _, m in sg] == [s[1] for s in cxx[n]]
        assert sg[0][0] == 0 and sg[-1][0] + sg[-1][1] == n and all(1 <= m <= seg_len for _, m in sg)
        assert (len(sg) == 1) == (n <= seg_len)
        for (o0, m0), (o1, m1) in zip(sg, sg[1:]):
            assert m0 == seg_len and o0 + m0 - o1 == overlap and o0 + m0 < n, "inner segments are whole, overlap by V and end before the gene"
        assert len(sg) == 1 or sg[-1][1] > overlap, "the last segment reaches past the one before it"
        # the edges of the records: lo on all but the first, hi on all but the last
        assert [s[2] for s in cxx[n]] == [-1] + [0] * (len(sg) - 1) and [s[3] for s in cxx[n]] == [m - 1 for _, m in sg[:-1]] + [-1]


def test_every_short_span_lies_in_the_stated_segment_exhaustively(emul):
    """seg_len 13, overlap 5: every gene of 1 .. 60 residues, every span of at most V + 1 residues - in g++'s build and in numpy"""
    total = 0
    for n in range(1, 61):
        bad, checked = (int(x) for x in subprocess.check_output([emul, "spans", "13", "5", str(n)], text=True).split())
        sg, mine = FR.segments(n, 13, 5), 0
        for a in range(n):
            for b in range(a, min(n, a + 6)):
                o, m = sg[FR.seg_of(a, n, 13, 5)]
                assert o <= a and b <= o + m - 1, (n, a, b)
                mine += 1
        assert bad == 0 and checked == mine
        total += checked
    assert total > 9000
    # and at the library's constants, on the segment boundaries of a gene of three segments: the widest span, and one residue wider fails
    n = FR.L + 2 * S
    sg = FR.segments(n)
    for a in (0, S - 1, S, 2 * S - 1, 2 * S, n - FR.V - 1):
        o, m = sg[FR.seg_of(a, n)]
        assert o <= a and a + FR.V <= o + m - 1
    o, m = sg[FR.seg_of(S - 1, n)]
    assert S - 1 + FR.V + 1 > o + m - 1, "a span of V + 2 residues from the last residue before a step leaves its segment: V + 1 is sharp"


def test_the_fold_of_the_header_equals_the_numpy_statement(emul, tmp_path):
    rng = np.random.default_rng(11)
    lens = [1, 64, 2047, 2048, 2049, 5000, 65535, 700, FR.L, FR.L + 1]
    rec, seg_gene, seg_off, seg_res = FR.records(lens)
    assert len(rec) == sum(len(FR.segments(n)) for n in lens)
    rows = FR.random_rows(rng, 5000, len(rec), seg_res, low=-2)
    oc.write_sections(tmp_path / "in", [np.int32([len(rec)]), rec, rows])
    subprocess.check_call([emul, "rows", str(tmp_path / "in"), str(tmp_path / "out")])
    out = oc.read_sections(tmp_path / "out")
    got, want = np.frombuffer(out[0], ROW_DTYPE), FR.fold(rows, rec)
    assert FR.same_rows(got, want)
    assert int(np.frombuffer(out[1], "<i8")[0]) == FR.edge_rows(rows, rec) > 0
    inside = (rows["subject"] >= 0) & (rows["subject"] < len(rec))
    assert np.array_equal(got[~inside], rows[~inside]) and (~inside).sum() > 100, "subjects out of range are copied unchanged"
    glen = np.array(lens)[got["subject"][inside]]
    assert (got["sstart"][inside] >= 0).all() and (got["send"][inside] < glen).all(), "folded spans lie inside their genes"


def test_split_genes_makes_the_segments_and_the_three_maps():
    rng = np.random.default_rng(5)
    lens = [10, FR.L, FR.L + 1, 3000, 1, 65535]
    seqs = ["".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), n)) for n in lens]
    names = ["g%d" % i for i in range(len(lens))]
    sp = abundance.split_genes(names, seqs)
    rec, seg_gene, seg_off, seg_res = FR.records(lens)
    assert np.array_equal(sp["seg_gene"], seg_gene) and np.array_equal(sp["seg_off"], seg_off) and sp["gene_len"].tolist() == lens
    assert [len(s) for s in sp["seg_seqs"]] == seg_res.tolist() and sp["stats"] == (sum(lens), len(lens)) and sp["genes_split"] == 3
    for nm, sq, g, o in zip(sp["seg_names"], sp["seg_seqs"], sp["seg_gene"], sp["seg_off"]):
        assert seqs[g][o:o + len(sq)] == sq and nm == (names[g] if lens[g] <= FR.L else "%s|%d" % (names[g], o))
    assert len(set(sp["seg_names"])) == len(sp["seg_names"])
    small = abundance.split_genes(names[:2], seqs[:2])
    assert small["seg_names"] == names[:2] and small["seg_seqs"] == seqs[:2] and small["genes_split"] == 0


def _fasta(path, lens):
    with open(path, "w") as f:
        for i, n in enumerate(lens):
            f.write(">g%d\n%s\n" % (i, "ACDEFGHIKL" * (n // 10) + "A" * (n % 10)))
    return str(path)


def test_refusals_before_any_gpu_work(tmp_path):
    with pytest.raises(abundance.AbundanceError, match="Gene g1 is 2048 residues long: longer than 2047"):
        abundance.read_genes(_fasta(tmp_path / "a.faa", [5, 2048]))
    names, seqs = abundance.read_genes(_fasta(tmp_path / "a.faa", [5, 2048, 65535]), long_genes=True)
    assert [len(s) for s in seqs] == [5, 2048, 65535]
    with pytest.raises(abundance.AbundanceError, match="Gene g2 is 65536 residues long: longer than 65535"):
        abundance.read_genes(_fasta(tmp_path / "b.faa", [5, 2048, 65536]), long_genes=True)
    with pytest.raises(abundance.AbundanceError, match="Gene g0 is 65536 residues long: longer than 65535"):
        abundance.split_genes(["g0"], ["A" * 65536])
    per = len(FR.segments(65535))
    k = FR.MAX_SEGS // per                                            # k genes fit, gene k is the one at which the total is passed
    with pytest.raises(abundance.AbundanceError, match=r"Gene g%d \(65535 residues, %d segments\) takes the database past 32767 segments: %d before it" % (k, per, k * per)):
        abundance.split_genes(["g%d" % i for i in range(k + 2)], ["A" * 65535] * (k + 2))
    args = {"seqfiles": ["x.fq"], "genes": _fasta(tmp_path / "a.faa", [5, 2048]), "long_genes": "yes"}
    with pytest.raises(abundance.AbundanceError, match="long_genes 'yes' is not a switch"):
        abundance.check_request(args)
    args["long_genes"] = False
    with pytest.raises(abundance.AbundanceError, match="Gene g1 is 2048 residues long: longer than 2047"):
        abundance.check_request(args)
    args["long_genes"] = True
    names, seqs = abundance.check_request(args)[:2]
    assert names == ["g0", "g1"] and args["gene_fold"]["genes_split"] == 1 and len(args["gene_fold"]["seg_names"]) == 1 + len(FR.segments(2048))


TABLE = {"gene": ["g1", "g2", "g3"], "length_aa": np.array([120, 300, 2047], np.int64), "reads": np.array([5, 0, 7], np.int64), "aligned_aa": np.array([150, 0, 231], np.int64),
         "rpkg": np.array([1.5, 0.0, 0.25]), "sampled_reads": 1000, "trimmed_length": 100, "ags": 3000000.0, "ags_source": "--ags", "genome_equivalents_sampled": 0.0333,
         "reads_assigned": 12}
ARGS = {"seqfiles": ["a.fq"], "genes": "genes.faa", "min_ident": 0, "min_aln": 0, "min_bits": 0.0}


def test_switch_off_the_table_is_byte_for_byte_what_it_was(tmp_path):
    """the fixed table written without the switch: the text as it was before the switch existed, spelled out; with table['long_genes'] four
    header lines more and every other byte the same"""
    abundance.write_table(str(tmp_path / "off.tsv"), dict(ARGS), dict(TABLE))
    off = open(tmp_path / "off.tsv").read()
    assert off == ("# metagenome:\ta.fq\n# genes:\tgenes.faa\n# sampled_reads:\t1000\n# trimmed_length:\t100\n# min_ident:\t0\n# min_aln:\t0\n# min_bits:\t0.0\n"
                   "# average_genome_size:\t3000000.0\n# ags_source:\t--ags\n# genome_equivalents_sampled:\t0.0333\n# reads_assigned:\t12\n"
                   "gene\tlength_aa\treads\taligned_aa\trpkg\ng1\t120\t5\t150\t1.5\ng2\t300\t0\t0\t0.0\ng3\t2047\t7\t231\t0.25\n")
    abundance.write_table(str(tmp_path / "none.tsv"), dict(ARGS), dict(TABLE, long_genes=None))
    assert open(tmp_path / "none.tsv").read() == off
    abundance.write_table(str(tmp_path / "on.tsv"), dict(ARGS), dict(TABLE, long_genes={"genes_split": 2, "segments": 9, "edge_rows": 0}))
    on = open(tmp_path / "on.tsv").read().splitlines(True)
    more = ["# long_genes:\ton\n", "# genes_split:\t2\n", "# segments:\t9\n", "# edge_rows:\t0\n"]
    assert on[11:15] == more and on[:11] + on[15:] == off.splitlines(True)


def test_the_statistics_pair_gives_the_tables_of_the_unsplit_index(tmp_path):
    """genes of up to 2,047 residues cut at (300, 100): the segment index with the genes' totals has the unsplit index's length adjustment,
    search space and every bits / loge entry, bit for bit; without the pair it has not; the pair changes nothing else"""
    exe = str(tmp_path / "fold_tables")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "emul", "fold_tables.cpp")])
    names, seqs = _native.load_markers()
    pick = [i for i in np.argsort([-len(s) for s in seqs])[:40]] + list(range(0, 400, 10))
    with open(tmp_path / "g.faa", "w") as f:
        for i in pick:
            f.write(">%s\n%s\n" % (names[i], seqs[i]))
    for read_len in (100, 150):
        out = dict(l.split(None, 1) for l in subprocess.check_output([exe, str(tmp_path / "g.faa"), "300", "100", str(read_len)], text=True).splitlines())
        assert out["stats"] == "1" and out["unset_differs"] == "1" and out["rest"] == "1", out
        assert int(out["segments"].split()[4]) >= 40


def test_abi_symbols():
    for s in ("mc_open_stats", "mc_set_gene_fold", "mc_gene_fold_stats", "mc_abundance_count", "mc_abundance_residues"):
        assert s in _native.EXPORTED_SYMBOLS
    for m in ("set_gene_fold", "gene_fold_stats", "abundance_count"):
        assert hasattr(_native.Engine, m)
