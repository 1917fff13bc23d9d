"""Reads of mixed lengths on the device (mc_search_varlen): bucketed by length, every bucket through the fixed-length pipeline at its
own length, results in the caller's order.  Checked against the reference's rapsearch on a mixed-length file
(tests/golden/varlen_reads.*, tests/golden/make_varlen_golden.py), against mc_search on batches of one length, and at size against
per-length mc_search runs of each length's subset."""
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from microbecensus_amd import _native, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
STAT_COUNTS = ["reads", "seed_tasks", "gap_tasks", "hsps", "rows", "reads_with_rows", "classified", "bucket_lookups", "key_probes",
               "seed_exact_asks", "seed_wild_asks", "seed_pair_asks", "seed_probes", "range_splits"]


def _golden_reads():
    fasta = gzip.open(os.path.join(GOLD, "varlen_reads.fa.gz"), "rb").read()
    return fasta, fasta.splitlines()[1::2]


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine(device=0)
    yield e
    e.close()


def _same(a, b):
    """structured arrays equal field by field (the row record has padding bytes, which nobody writes)"""
    return a.dtype == b.dtype and len(a) == len(b) and all((a[f] == b[f]).all() for f in a.dtype.names)


def _as_varlen(reads2d, lens):
    """(bases, offsets) of the first lens[i] bases of row i of a 2-D read array."""
    mask = np.arange(reads2d.shape[1])[None, :] < lens[:, None]
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return np.ascontiguousarray(reads2d[mask]), off


def _per_length(eng, reads2d, lens):
    """rows of every length's subset searched by mc_search at that length, query = the read's index in the whole batch; in
    ascending read id, a read's rows in their order."""
    parts = []
    for L in np.unique(lens):
        if L < 18:
            continue
        idx = np.nonzero(lens == L)[0]
        eng.set_run(int(L))
        rows, _ = eng.search(reads2d[idx, :L])
        rows["query"] = idx[rows["query"]]
        parts.append(rows)
    rows = np.concatenate(parts)
    return rows[np.argsort(rows["query"], kind="stable")]


def test_rapsearch_executable_on_mixed_lengths(tmp_path):
    """scripts/rapsearch_mi355x on the golden file of 4,000 reads of 12..510 bases: the m8 body is the reference's, byte for byte."""
    meta = json.load(open(os.path.join(GOLD, "varlen_reads.json")))
    fasta, _ = _golden_reads()
    fa = tmp_path / "reads.fa"
    fa.write_bytes(fasta)
    from microbecensus_amd import microbe_census as mc
    out = str(tmp_path / "out")
    subprocess.check_call([os.path.join(REPO, "scripts", "rapsearch_mi355x"), "-q", str(fa), "-d", mc._rapdb_for_external_search(), "-o", out,
                           "-z", "1", "-e", "1", "-t", "n", "-p", "f", "-b", "0"], stdout=subprocess.DEVNULL, timeout=300)
    lines = open(out + ".m8", "rb").readlines()
    assert [l[:1] for l in lines[:5]] == [b"#"] * 5
    assert hashlib.md5(b"".join(lines[5:])).hexdigest() == meta["m8_md5"]


def test_search_varlen_rows_are_the_reference_rows(eng, tmp_path):
    """Engine.search_varlen on the golden reads: the m8 the handle writes is the reference's; reads under 18 bases have no rows;
    every best hit belongs to a read with rows."""
    _, seqs = _golden_reads()
    want = gzip.open(os.path.join(GOLD, "varlen_reads.m8.gz"), "rb").read()
    eng.set_run(150)
    rows, best = eng.search_varlen(seqs)
    st = eng.stats()
    out = str(tmp_path / "v.m8")
    eng.write_m8(out)
    assert open(out, "rb").read() == want
    assert st["reads"] == len(seqs) and st["rows"] == len(rows) == want.count(b"\n")
    lens = np.array([len(s) for s in seqs])
    assert (lens[rows["query"]] >= 18).all() and (np.diff(rows["query"]) >= 0).all()
    assert set(best["read"].tolist()) <= set(rows["query"].tolist()) and (np.diff(best["read"]) > 0).all()
    rows2, best2 = eng.search_varlen(seqs, first_read_id=1000)      # ids offset, nothing else
    assert (rows2["query"] == rows["query"] + 1000).all() and (best2["read"] == best["read"] + 1000).all()


@pytest.mark.parametrize("case", ["config1_example_fq", "synth_150bp"])
def test_one_length_batch_is_mc_search(eng, case):
    """A batch whose reads all have the run's length: rows, best hits and statistics those of mc_search."""
    if case == "config1_example_fq":
        seqs = gzip.open(os.path.join(GOLD, "config1_example_fq.reads.fa.gz"), "rb").read().splitlines()[1::2]
        L = len(seqs[0])
        reads = np.frombuffer(b"".join(seqs), np.uint8).reshape(len(seqs), L)
    else:
        names, mseqs = _native.load_markers()
        genome = synth.build_genomes(mseqs, total_bp=400_000, seed=7, marker_gene_fraction=0.2)
        L, reads = 150, synth.sample_reads(genome, 20_000, 150, seed=5)
    eng.set_run(L)
    rows, best = eng.search(reads)
    st = eng.stats()
    lens = np.full(len(reads), L, np.int64)
    rows2, best2 = eng.search_varlen(_as_varlen(reads, lens))
    st2 = eng.stats()
    assert len(rows) > 0 and _same(rows, rows2) and _same(best, best2)
    assert {k: st[k] for k in STAT_COUNTS} == {k: st2[k] for k in STAT_COUNTS}


def test_search_varlen_at_size_equals_per_length_searches(eng):
    """2 M reads of 60..300 bases (about 8,300 per length): search_varlen's rows are, by original id, those of mc_search over each
    length's subset at that length; the fixed-length path afterwards is unchanged."""
    gr = synth.GenomeReads(device="cpu", seed=31)
    n = 2_000_000
    reads = gr.single(n, 300).numpy()
    lens = np.random.RandomState(5).randint(60, 301, n).astype(np.int64)
    eng.set_run(150)
    rows, best = eng.search_varlen(_as_varlen(reads, lens))
    st = eng.stats()
    print("varlen", st)
    assert st["reads"] == n and len(rows) > 100_000 and len(best) > 0
    want = _per_length(eng, reads, lens)
    assert len(rows) == len(want)
    assert _same(rows, want)
    eng.set_run(150)                                                   # the fixed path after a varlen run: the reads of length 150, as before
    idx = np.nonzero(lens == 150)[0]
    r150, b150 = eng.search(reads[idx, :150])
    r150["query"] = idx[r150["query"]]
    b150["read"] = idx[b150["read"]]
    assert _same(r150, rows[lens[rows["query"]] == 150])
    assert len(b150) > 0 and _same(b150, best[lens[best["read"]] == 150])     # classified at set_run()'s length, as mc_search does


def test_search_varlen_pool_overflow(eng):
    """A marker-dense batch whose largest bucket overflows the pools of its range: the bucket is run in halves, the rows those of
    per-length mc_search runs (which halve the same way)."""
    names, mseqs = _native.load_markers()
    genome = synth.build_genomes(mseqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0)
    n = 70_000
    reads = synth.sample_reads(genome, n, 200, seed=9)
    rs = np.random.RandomState(11)
    lens = np.where(rs.rand(n) < 0.9, 150, rs.randint(12, 201, n)).astype(np.int64)
    eng.set_run(150)
    rows, best = eng.search_varlen(_as_varlen(reads, lens))
    st = eng.stats()
    print("dense varlen", st)
    assert st["range_splits"] > 0, "no bucket overflowed: the test no longer exercises the halving inside a bucket"
    want = _per_length(eng, reads, lens)
    assert len(rows) == len(want) and _same(rows, want)


def test_search_varlen_refusals(eng):
    eng.set_run(100)
    ok = b"ACGT" * 25
    for seqs, msg in (([ok, b"A" * 511, ok], "read 1 is 511 bases long"), ([ok, ok, b""], "read 2 is empty")):
        with pytest.raises(RuntimeError, match=msg):
            eng.search_varlen(seqs)
    rows, best = eng.search_varlen([b"ACGTACGTAC", b"ACGTAC"])             # reads under 18 bases: no rows, nothing searched
    assert len(rows) == 0 and len(best) == 0 and eng.stats()["reads"] == 2


# ---- piece boundaries, and the handle after a borrowed-length run -------------------------------------------------------------------
BOUNDARY_COUNTS = [(17, 5), (18, 1), (150, 1000), (151, 1001), (200, 2096)]       # 4,103 reads: more than one 4,096-read tile of the bucketing kernels


@pytest.fixture(scope="module")
def boundary(eng):
    """(reads2d, lens, rows of the per-length yardstick, best hits of the 150 bp reads at set_run(150)): the lengths interleaved; under a
    batch of 1,000 the buckets are one piece of 1 read, one of exactly the batch, batch + 1 and 2 x batch + 96."""
    names, mseqs = _native.load_markers()
    genome = synth.build_genomes(mseqs, total_bp=400_000, seed=7, marker_gene_fraction=0.2)
    lens = np.repeat([L for L, _ in BOUNDARY_COUNTS], [c for _, c in BOUNDARY_COUNTS]).astype(np.int64)
    np.random.RandomState(12).shuffle(lens)
    reads = synth.sample_reads(genome, len(lens), 200, seed=13)
    assert "MC_STREAM_BATCH" not in os.environ
    want = _per_length(eng, reads, lens)
    idx = np.nonzero(lens == 150)[0]
    eng.set_run(150)
    _, b150 = eng.search(reads[idx, :150])
    b150["read"] = idx[b150["read"]]
    assert len(want) > 500 and len(b150) > 0 and len(set(lens[want["query"]].tolist())) >= 3
    return reads, lens, want, b150


@pytest.mark.parametrize("batch", ["1000", None], ids=["batch-1000", "one-piece-per-length"])
def test_varlen_piece_boundaries(eng, boundary, batch, monkeypatch):
    """Buckets of 1, batch, batch + 1 and 2 x batch + 96 reads beside reads too short to search: the rows are those of per-length
    mc_search runs, the best hits of the run's own length those of mc_search, however the buckets are cut into pieces.
    _per_length yields rows only, and a per-length mc_search cannot restate the best hits of the other lengths: a mixed run classifies
    every read at mc_set_run()'s length (150), mc_search at the length it was set up for.  So only the 150 bp bucket's best hits have
    an independent yardstick; for the other lengths the test asks that they are best hits of reads with rows, ascending, and the
    same under both cuts - which compares the code with itself."""
    reads, lens, want, b150 = boundary
    if batch:
        monkeypatch.setenv("MC_STREAM_BATCH", batch)
    eng.set_run(150)
    rows, best = eng.search_varlen(_as_varlen(reads, lens))
    st = eng.stats()
    assert st["reads"] == len(lens) == 4103 and st["rows"] == len(rows)
    assert len(rows) == len(want) and _same(rows, want)
    assert _same(best[lens[best["read"]] == 150], b150)
    assert (np.diff(best["read"]) > 0).all() and set(best["read"].tolist()) <= set(rows["query"].tolist())
    if batch:                                                          # the best hits of every length do not depend on the cut either
        monkeypatch.delenv("MC_STREAM_BATCH")
        _, best_whole = eng.search_varlen(_as_varlen(reads, lens))
        assert _same(best, best_whole)


@pytest.mark.parametrize("case", ["pieces", "all-short"])
def test_handle_comes_back_after_search_varlen(eng, boundary, case, monkeypatch):
    """A fixed-length search, a varlen call, the same search again WITHOUT another set_run: identical (rows field by field: their padding bytes are nobody's; best hits byte for byte), equal counts - the run's
    length, frame pitch, tables and resident reads are the handle's again.  all-short: no piece, the tables were never switched."""
    reads, lens, _, _ = boundary
    r150 = np.ascontiguousarray(reads[lens == 150, :150])
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")
    eng.set_run(150)
    rows0, best0 = eng.search(r150)
    st0 = eng.stats()
    eng.upload(r150[:700])
    eng.run(first_read_id=5)
    res0 = eng.results()
    if case == "pieces":
        rows, _ = eng.search_varlen(_as_varlen(reads, lens))
        assert len(rows) > 0 and eng.stats()["reads"] == len(lens)
    else:
        rows, best = eng.search_varlen([b"ACGTACGTACGTACGTA", b"ACGTAC", b"A"])
        assert len(rows) == 0 and len(best) == 0 and eng.stats()["reads"] == 3
    eng.run(first_read_id=5)                                           # the resident reads are still the uploaded ones
    res1 = eng.results()
    assert len(res0[0]) > 0 and _same(res1[0], res0[0]) and res1[1].tobytes() == res0[1].tobytes()
    rows1, best1 = eng.search(r150)
    st1 = eng.stats()
    assert len(rows0) > 0 and len(best0) > 0 and _same(rows1, rows0) and best1.tobytes() == best0.tobytes()
    assert {k: st0[k] for k in STAT_COUNTS} == {k: st1[k] for k in STAT_COUNTS}
