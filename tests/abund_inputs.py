"""What test_gpu_abundance.py, test_gpu_coverage.py and test_gpu_ties.py run on, built in one place: the engine on the marker database at
100 bp, the example reads, the generic-database case and the 24,000-read marker-dense library with its MC_STREAM_BATCH sequence.  Every
module keeps a two-line fixture (or call) of its own; nothing here asserts what a test is about."""
import contextlib
import gzip
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASE = "config1_example_fq"
DENSE_CUT = dict(min_ident=40, min_aln=30)


def marker_engine():
    """(a generator, for `yield from` in a module-scoped fixture) an engine on the packaged markers, set up for 100 bp under the model"""
    from microbecensus_amd import _native
    e = _native.Engine(device=0)
    model = _native.load_model()
    e.set_run(100, model["pars"]["100"], model["families"])
    yield e
    e.close()


def example_reads():
    seqs = [l.rstrip(b"\r\n") for l in gzip.open(os.path.join(GOLD, CASE + ".reads.fa.gz"), "rb") if not l.startswith(b">")]
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), len(seqs[0]))


@contextlib.contextmanager
def generic_case():
    """18,553 sequences, 20,000 reads, the generic seed path: (engine set up for the case's read length, names, seqs, reads, meta, the
    path of the reference binary's m8); the reads are those the golden was made of, by their md5"""
    sys.path.insert(0, GOLD)
    import make_generic_db_golden as G
    from microbecensus_amd import _native
    meta = json.load(open(os.path.join(GOLD, "generic_db.json")))
    names, seqs, rd = G.case_inputs()
    assert hashlib.md5(b"".join(b">%d\n%s\n" % (i, bytes(r)) for i, r in enumerate(rd))).hexdigest() == meta["reads_md5"]
    eng = _native.Engine(device=0, names=names, seqs=seqs, marker_family=[0] * len(names), nfam=1)
    try:
        eng.set_run(meta["read_length"])
        yield eng, names, seqs, rd, meta, os.path.join(GOLD, "generic_db.m8.gz")
    finally:
        eng.close()


def dense_runs(monkeypatch, switches, take, stay=False):
    """The marker-dense library of tests/test_gpu_blindspots.py's recipe (~290 HSPs and ~100 m8 rows per read).  The size: the pools of
    a run of n reads of 150 bp hold 16 n + 2^20 rows and 58 n + 3 x 2^20 HSPs (ensure_capacity), so ~100 rows per read overflow the row
    pool from n = 12,500 on and ~290 HSPs per read the HSP pool from 13,600 on: 24,000 reads on an engine of their own (pools only
    grow) is a small size that takes the halving path with a margin - which every caller asserts on the stats handed back.
    switches(eng): what the test turns on, under DENSE_CUT; take(eng): what it keeps of a run.  The runs: ONE call; 5,000-read batches
    (which fit: no split), whose host rows are handed back; with `stay`, one call once more through mc_range_end's -2 and mc_run_range
    with the rows staying on the device.  Returns a dict: names, seqs, reads, one = (stats, taken), five = (stats, taken, rows) and,
    with `stay`, stay = (taken, the host rows the engine then has)."""
    from microbecensus_amd import _native, synth
    names, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=3_000_000, seed=404, marker_gene_fraction=1.0)
    rd = synth.sample_reads(genome, 24_000, 150, seed=405)
    out = {"names": names, "seqs": seqs, "reads": rd}
    eng = _native.Engine(device=0)
    try:
        eng.set_run(150)
        switches(eng)
        eng.search(rd)
        out["one"] = (eng.stats(), take(eng))
        eng.abundance_reset()
        monkeypatch.setenv("MC_STREAM_BATCH", "5000")
        rows5, _ = eng.search(rd)
        monkeypatch.delenv("MC_STREAM_BATCH")
        out["five"] = (eng.stats(), take(eng), rows5)
        if stay:
            eng.abundance_reset()
            monkeypatch.setenv("MC_STREAM_BATCH", "1000000")
            eng.lib.mc_set_keep_rows(eng.h, 0)
            eng.search(rd)
            eng.lib.mc_set_keep_rows(eng.h, 1)
            monkeypatch.delenv("MC_STREAM_BATCH")
            out["stay"] = (take(eng), len(eng.rows()))
    finally:
        eng.close()
    return out
