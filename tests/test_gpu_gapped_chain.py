"""The gapped extension's chain of kernels (csrc/k_gapped.h, stage B) witnessed and checked on the device: k_gapped_lds with a
36-column LDS window, k_gapped_lds with 64 columns for the flanks whose band left the first window or whose packed path statistics
overflowed, k_gapped with full-size rows in global memory for what left the second one too.  The counts of the chain
(mc_debug_stage 4: Engine.gap_counts) are held against the CPU emulation of the same per-thread code (tests/emul/mc_emul: one flank
per distinct ungapped segment, the windowed form at W1 and W2), in the product library and in a library built with windows of 16
and 24 columns, in which thousands of ordinary flanks are decided by the second launch and by the last resort - and every result
is still the reference's.  All calls go through the C ABI."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_emul import run_gapped_chain
from test_gpu_parity import golden_reads
from test_gpu_pipeline import _oracle_rows, _rows, assert_rows_equal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


def _error_reads(L, n, sub, indel):
    """the reads of test_reads_with_sequencing_errors_against_oracle (tests/test_gpu_blindspots.py) for these parameters"""
    from microbecensus_amd import _native, synth
    names, seqs = _native.load_markers()
    genome = synth.build_genomes(seqs, total_bp=600_000, seed=900 + L, marker_gene_fraction=0.3)
    clean = synth.sample_reads(genome, n, L + 24, seed=L + 7)
    return synth.mutate_reads(clean, L, sub_rate=sub, indel_rate=indel, seed=L + int(sub * 1000))


class _Sets:
    """The read sets (arrays and FASTA files) and the emulation's counts of them, each made once per module."""

    def __init__(self, d):
        self.d = d
        self.exe = str(d / "mc_emul")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", self.exe, os.path.join(HERE, "emul", "mc_emul.cpp")])
        self.faa = d / "markers.faa"
        self.faa.write_bytes(gzip.open(os.path.join(REPO, "microbecensus_amd", "data", "markers.faa.gz"), "rb").read())
        self._reads, self._counts = {}, {}

    def reads(self, name):
        if name not in self._reads:
            if name == "dirty_reads":
                seqs = [l.rstrip(b"\r\n") for l in gzip.open(os.path.join(GOLD, "dirty_reads.fa.gz"), "rb") if not l.startswith(b">")]
                r = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), len(seqs[0]))
            elif name == "errors_150bp":
                r = _error_reads(150, 6000, 0.05, 0.01)
            elif name == "errors_500bp":
                r = _error_reads(500, 1500, 0.03, 0.01)
            else:
                r = golden_reads(name)[0]
            self._reads[name] = np.ascontiguousarray(r)
        return self._reads[name]

    def fasta(self, name):
        p = self.d / (name + ".fa")
        if not p.exists():
            p.write_bytes(b"".join(b">%d\n%s\n" % (i, bytes(r)) for i, r in enumerate(self.reads(name))))
        return p

    def stage_prefix(self, name):
        return str(self.d / (name + ".emul"))

    def counts(self, name, w1, w2):
        """(D, R1, R2) of the emulation's "gapped chain" line; the run also dumps the emulation's stages (stage_prefix)"""
        if (name, w1, w2) not in self._counts:
            (d, r1, r2), (_, _, differ) = run_gapped_chain(self.exe, self.faa, self.fasta(name), self.d / "e.m8", w1, w2, dump=self.stage_prefix(name))
            assert differ == 0
            self._counts[name, w1, w2] = {"flanks": d, "second_window": r1, "full_size": r2}
        return self._counts[name, w1, w2]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _Sets(tmp_path_factory.mktemp("gapped_chain"))


@pytest.fixture(scope="module")
def engine():
    from microbecensus_amd._native import Engine
    e = Engine(device=0)
    yield e
    e.close()


@pytest.mark.parametrize("name", ["config1_example_fq", "dirty_reads", "errors_150bp", "errors_500bp"])
def test_chain_counts_of_the_product_library_equal_the_emulation(name, engine, sets):
    """Product library, windows (36, 64): after one unsplit mc_run_range the distinct flanks, the flanks sent to the second window
    and those sent to full-size rows are EXACTLY the emulation's.  The emulation's counts per set, D / R1 / R2:
    config1_example_fq 4,034 / 0 / 0; dirty_reads 23,046 / 1 / 0; errors_150bp (150 bp, 5 % substitutions, 1 % indels, n = 6000)
    58,620 / 90 / 0; errors_500bp (500 bp, 3 %, 1 %, n = 1500) 114,831 / 525 / 0.  The two sets of reads with errors are the ones
    that put the second launch to work (asserted); no set sends a flank to full-size rows with the product's windows (R2 = 0: a
    finding, not a requirement) - k_gapped is witnessed by the small-window library below."""
    reads = sets.reads(name)
    want = sets.counts(name, 36, 64)
    engine.set_run(reads.shape[1])
    engine.upload(reads)
    engine.run_range(0, len(reads))
    st, got = engine.stats(), engine.gap_counts()
    print(name, "device", got, "emulation", want)
    assert st["range_splits"] == 0
    assert got == want
    assert got["flanks"] > 100
    if name in ("errors_150bp", "errors_500bp"):
        assert got["second_window"] > 0


_CODON = dict(A="GCT", R="CGT", N="AAC", D="GAC", C="TGC", Q="CAG", E="GAA", G="GGT", H="CAC", I="ATC", L="CTG", K="AAA", M="ATG", F="TTC", P="CCG", S="TCT", T="ACC",
              W="TGG", Y="TAC", V="GTT")


def _read_with_a_gap_every_fifth_residue(marker, head=20, naa=170):
    """510 bp: the marker's first `head` residues back-translated unchanged (a seed and an ungapped segment), then its residues
    with every 5th one left out - the best path of the right flank opens a one-column gap after every four matches."""
    aa, k, i = list(marker[:head]), head, 0
    while len(aa) < naa:
        i += 1
        if i % 5:
            aa.append(marker[k])
        k += 1
    return np.frombuffer("".join(_CODON[a] for a in aa).encode(), dtype=np.uint8).reshape(1, 3 * naa)


def test_a_flank_with_32_gap_runs_reaches_full_size_rows_in_the_product_library(engine, sets):
    """The product's own windows, the route `ws.ovf`: a live path with 32 gap runs no longer fits the 5-bit run fields of an LDS
    cell (mc_gap_pack), k_gapped_lds hands the flank to its 64-column launch, which overflows in the same way, and k_gapped
    decides it with full-size cells.  The read is made from the packaged marker ARCH69_P641276511 (one residue in five left out
    behind an unchanged head of 20): the emulation counts 16 distinct flanks, 3 to the second window, 1 to full-size rows, and the
    oracle prints the read's alignment to that marker with 35 gap openings over 204 columns.  Rows == the oracle's, counts == the
    emulation's, at least one flank through k_gapped."""
    from microbecensus_amd import _native
    names, seqs = _native.load_markers()
    reads = _read_with_a_gap_every_fifth_residue(seqs[names.index("ARCH69_P641276511")])
    sets._reads["gap_every_fifth"] = reads
    want = sets.counts("gap_every_fifth", 36, 64)
    oracle = _oracle_rows(reads)
    assert want["full_size"] >= 1 and max(r[4] for r in oracle) >= 32          # (what the construction is for, said by the checkers themselves)
    engine.set_run(reads.shape[1])
    engine.upload(reads)
    engine.run_range(0, 1)
    st, got = engine.stats(), engine.gap_counts()
    print("device", got, "emulation", want)
    rows = _rows(engine.rows())
    assert st["range_splits"] == 0
    assert_rows_equal(rows, oracle)
    assert got == want and got["full_size"] >= 1
    assert max(r[4] for r in rows) >= 32


def test_flanks_wider_than_64_columns_reach_full_size_rows_in_the_product_library(sets, tmp_path):
    """The product's own windows, the route by width: six reads against a database of six synthetic subjects
    (gapped_cases.wide_witness - 30 shared residues, then flanks whose band is 70 columns wide or wider by the oracle's AlignGapped;
    high-complexity residues, SEG masks none of them).  The emulation counts 6 distinct flanks, all 6 through the second window
    to full-size rows; the device counts the same, and the rows are the oracle's on a database prerapsearch-formatted from the same
    subjects.  With the read above this is all the work k_gapped gets in the product build: that one by run count, these by width.
    (Measured on the MI355X: 1.2 s.)"""
    import gapped_cases as gc
    from microbecensus_amd import _native
    names, seqs, reads = gc.wide_witness()
    faa, fa = tmp_path / "wide.faa", tmp_path / "wide.fa"
    faa.write_text("".join(">%s\n%s\n" % ns for ns in zip(names, seqs)))
    fa.write_bytes(b"".join(b">%d\n%s\n" % (i, bytes(r)) for i, r in enumerate(reads)))
    (d, r1, r2), (_, _, differ) = run_gapped_chain(sets.exe, faa, fa, tmp_path / "e.m8", 36, 64)
    want = {"flanks": d, "second_window": r1, "full_size": r2}
    assert differ == 0 and r2 >= len(reads)
    _native.rapdb_write(names, seqs, str(tmp_path / "rapdb_2.15"))
    oracle = _oracle_rows(reads, ref_dir=str(tmp_path))
    assert len(oracle) >= len(reads)
    eng = _native.Engine(device=0, names=names, seqs=seqs, marker_family=[0] * len(names), nfam=1)
    try:
        eng.set_run(reads.shape[1])
        eng.upload(reads)
        eng.run_range(0, len(reads))
        st, got = eng.stats(), eng.gap_counts()
        rows = _rows(eng.rows())
    finally:
        eng.close()
    print("device", got, "emulation", want)
    assert st["range_splits"] == 0
    assert_rows_equal(rows, oracle)
    assert got == want and got["full_size"] > 0


_SMALL_WORKER = r"""
import hashlib, json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from microbecensus_amd import _native
work = sys.argv[2]
out = {"lib": _native.load_library()._name, "sets": {}}
eng = _native.Engine(device=0)
for name in json.load(open(os.path.join(work, "sets.json"))):
    reads = np.load(os.path.join(work, name + ".npy"))
    eng.set_run(reads.shape[1])
    eng.upload(reads)
    eng.run_range(0, len(reads))
    rows = eng.rows()
    m8 = os.path.join(work, name + ".m8")
    eng.write_m8(m8)
    out["sets"][name] = {"rows": len(rows), "md5": hashlib.md5(open(m8, "rb").read()).hexdigest(), "range_splits": eng.stats()["range_splits"], "counts": eng.gap_counts()}
    if name == "errors_150bp":
        np.save(os.path.join(work, "errors_150bp.rows.npy"), rows)
    if name == "dirty_reads":
        np.save(os.path.join(work, "dirty_reads.hsps.npy"), eng.debug_stage(3))
eng.close()
json.dump(out, open(os.path.join(work, "out.json"), "w"))
"""


def test_small_window_library_every_fallback_busy_results_unchanged(sets, tmp_path):
    """The library built with -DMC_GAP_WIN=16 -DMC_GAP_WIN2=24: a band of ordinary width (about 31 columns) leaves both windows, so
    the second launch of k_gapped_lds (LANES = 64, REFILL = 1, thousands of items) and k_gapped (full-size rows, its own workspace
    indexing, d_retry2 and its device-side count, both sides of a segment) decide thousands of real flanks - emulation at (16, 24),
    D / R1 / R2: config1_example_fq 4,034 / 2,976 / 1,140; dirty_reads 23,046 / 12,968 / 3,332; errors_150bp 58,620 / 50,677 /
    15,084.  One child process with that library: the m8 of three goldens is the reference binary's byte for byte, the rows of the
    reads with errors are the oracle's, the chain's counts are the emulation's exactly, and the HSP pool of dirty_reads is the
    emulation's (which extends every flank with the full-size form) as a multiset."""
    csrc = os.path.join(REPO, "microbecensus_amd", "csrc")
    lib = str(tmp_path / "libsmallwin.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           "-DMC_GAP_WIN=16", "-DMC_GAP_WIN2=24", "-o", lib,
                           os.path.join(csrc, "mc_hip.hip"), os.path.join(csrc, "mc_reader.cpp"), "-lz", "-ldl", "-pthread"], timeout=900)
    names = ["config1_example_fq", "unittest_metagenome", "dirty_reads", "errors_150bp"]
    for name in names:
        np.save(tmp_path / (name + ".npy"), sets.reads(name))
    (tmp_path / "sets.json").write_text(json.dumps(names))
    w = tmp_path / "w.py"
    w.write_text(_SMALL_WORKER)
    subprocess.check_call([sys.executable, str(w), REPO, str(tmp_path)], env=dict(os.environ, MCENSUS_LIB=lib), timeout=900)
    res = json.load(open(tmp_path / "out.json"))
    print(res)
    assert os.path.realpath(res["lib"]) == os.path.realpath(lib)
    got = res["sets"]
    for name in names:
        assert got[name]["range_splits"] == 0, name
    for name in ("config1_example_fq", "unittest_metagenome", "dirty_reads"):
        meta = json.load(open(os.path.join(GOLD, name + ".json")))
        assert (got[name]["rows"], got[name]["md5"]) == (meta["m8_rows"], meta["m8_md5"]), name
    rows = np.load(tmp_path / "errors_150bp.rows.npy")
    assert_rows_equal(_rows(rows), _oracle_rows(sets.reads("errors_150bp")))
    assert len(rows) > 100 and (rows["gapopen"] > 0).sum() > 5
    for name in ("config1_example_fq", "dirty_reads", "errors_150bp"):
        want = sets.counts(name, 16, 24)
        print(name, "device", got[name]["counts"], "emulation", want)
        assert got[name]["counts"] == want, name
    for name in ("config1_example_fq", "dirty_reads"):
        c = got[name]["counts"]
        assert c["full_size"] > 100 and c["second_window"] > c["full_size"], name
    # the HSP pool of dirty_reads against the emulation's (the comparison of test_every_stage_equals_the_emulation)
    hsp_dt = np.dtype({"names": ["read", "chrono", "sidx", "score", "frame", "alnlen", "mism", "gaps", "nmatch", "qaas", "qaae", "ds", "de", "qnts", "qnte", "loge"],
                       "formats": ["<u4", "<u4", "<i4"] + ["<i2"] * 12 + ["<f8"], "offsets": [0, 4, 8] + list(range(12, 36, 2)) + [40], "itemsize": 48})

    def table(a):                                                                       # the named fields (no padding bytes), rows in a canonical order
        t = np.stack([a[k].astype(np.float64) for k in a.dtype.names], 1)
        return t[np.lexsort(t.T[::-1])]
    he = np.fromfile(sets.stage_prefix("dirty_reads") + ".hsps", hsp_dt)
    hg = np.load(tmp_path / "dirty_reads.hsps.npy").reshape(-1).view(hsp_dt)
    hg = hg[hg["read"] != 0xFFFFFFFF]
    assert len(hg) == len(he) and len(he) > 1000 and (he["gaps"] > 0).any()
    assert np.array_equal(table(he), table(hg))
