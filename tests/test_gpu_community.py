"""GPU tests of mock communities (mc_community_*, csrc/k_community.h): device bytes and per-member counts against the numpy
restatement, one member with one copy against mc_simulate, the fused library pass against the staged one, validate() against
run_pipeline on the written metagenome, the reference's own estimate of a recorded library, and the refusals."""
import ctypes as C
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import community_restated as cr
import simlib_restated as sr
from microbecensus_amd import _native, training, validation
from microbecensus_amd import microbe_census as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
STREAM_BATCH = 2000000                                        # MC_STREAM_BATCH of csrc/mc_hip.hip

KINDS = [dict(), dict(error_model="illumina"), dict(error_model="uniform", error_rate=0.02), dict(error_model="uniform", error_rate=0.6),
         dict(paired_end=True, insert=400), dict(error_model="illumina", paired_end=True, insert=400)]


@pytest.fixture(scope="module")
def genomes():
    return cr.fixture_members()


def uneven_copies(n, seed=20261016):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = np.clip(np.floor(rng.lognormal(0.0, 1.5, n) * 30000), 1, 1 << 20).astype(np.int64)
    c[1], c[2] = 1, 1 << 20
    return c.tolist()


def write_fna(path, bases, off):
    with gzip.open(path, "wb", compresslevel=1) as f:
        for k in range(len(off) - 1):
            seq = bases[off[k]: off[k + 1]].tobytes()
            f.write(b">c%d\n" % k)
            for j in range(0, len(seq), 80):
                f.write(seq[j: j + 80] + b"\n")


# ---- 5. device bytes and counts == the restatement ------------------------------------------------------------------------
def test_device_bytes_and_counts_equal_restatement(genomes, monkeypatch):
    monkeypatch.setenv("MC_STREAM_BATCH", "1000")              # internal ranges of 1,000 reads
    members = [(b, o) for _, b, o in genomes]
    copies = uneven_copies(len(members))
    bases, off, mfirst = cr.join_members(members)
    comm = _native.Community(members, copies, 0)
    try:
        for kind in KINDS:
            comm.set_library(**kind)
            for L in (100, 150, 300):
                lid = training.library_id("thirty", L)
                first, n = 899, 2601                            # an odd start inside the first range; several ranges, many blocks
                got = comm.simulate(L, n, 7, lid, first=first)
                want, m, _, _ = cr.simulate(bases, off, mfirst, copies, L, first, n, 7, lid, **kind)
                assert np.array_equal(got, want), (kind, L)
                assert np.array_equal(comm.member_reads(), np.bincount(m, minlength=len(members))), (kind, L)
        comm.set_library()
        assert np.array_equal(comm.simulate(150, 500, 7, 1), cr.simulate(bases, off, mfirst, copies, 150, 0, 500, 7, 1)[0])
    finally:
        comm.close()


def test_a_table_searched_in_global_memory(genomes):
    """More members than the LDS table holds (the 30 genomes' contigs as members of their own, several times over): the same draw."""
    members = []
    for _, b, o in genomes * 5:
        members += [(b[o[k]: o[k + 1]], np.array([0, o[k + 1] - o[k]], np.int64)) for k in range(len(o) - 1)]
    assert len(members) > 1024
    copies = uneven_copies(len(members), 3)
    bases, off, mfirst = cr.join_members(members)
    comm = _native.Community(members, copies, 0)
    try:
        for kind in (dict(), dict(error_model="illumina", paired_end=True, insert=400)):
            comm.set_library(**kind)
            got = comm.simulate(150, 3001, 2, 5, first=77)
            want, m, _, _ = cr.simulate(bases, off, mfirst, copies, 150, 77, 3001, 2, 5, **kind)
            assert np.array_equal(got, want), kind
            assert np.array_equal(comm.member_reads(), np.bincount(m, minlength=len(members))), kind
    finally:
        comm.close()


# ---- 6. one member, one copy == mc_simulate -------------------------------------------------------------------------------
def test_one_member_one_copy_is_mc_simulate(genomes):
    for name, bases, off in (genomes[4], genomes[11]):
        g = _native.Genome(bases, off, 0)
        comm = _native.Community([(bases, off)], [1], 0)
        try:
            for kind in KINDS:
                g.set_library(**kind)
                comm.set_library(**kind)
                for L in (100, 150, 300):
                    lid = training.library_id(name, L)
                    assert comm.simulate(L, 5000, 3, lid, first=1235).tobytes() == g.simulate(L, 5000, 3, lid, first=1235).tobytes(), (name, kind, L)
                    assert comm.member_reads().tolist() == [5000]
        finally:
            comm.close()
            g.close()


# ---- 6b. the edges of the simulator both sources share ---------------------------------------------------------------------
EDGE_LS, EDGE_NS, EDGE_FIRST = (18, 101, 510), (1, 63, 65, 257), 1235       # the read-length limits and an odd one; one row, a row less / more than a wave, a row more than a block; mate 1 first


def edge_kind(kind, L):
    return dict(kind, insert=max(400, L + 7)) if kind.get("paired_end") else kind


def edge_references(genomes, kind, L):
    """The restatements' rows [EDGE_FIRST, EDGE_FIRST + 257) of a three-member community and of one genome: every shorter range is a prefix."""
    members, copies = [(b, o) for _, b, o in genomes[:3]], [3, 1, 70000]
    bases, off, mfirst = cr.join_members(members)
    n, lid, k = max(EDGE_NS), training.library_id("edges", L), edge_kind(kind, L)
    want_c, m, _, _ = cr.simulate(bases, off, mfirst, copies, L, EDGE_FIRST, n, 9, lid, **k)
    want_g = sr.simulate(genomes[4][1], genomes[4][2], L, EDGE_FIRST, n, 9, lid, **k)
    return members, copies, lid, k, want_c, m, want_g


def test_edges_of_the_shared_simulator(genomes):
    """Shapes the other tests never reach: L at both limits and L = 101 (a last block whose rows x L bytes are no multiple of 4), libraries
    of 1, 63, 65 and 257 reads, a range that begins on mate 1, an insert of max(400, L + 7) - for every kind, a community and a genome
    against their restatements, and the community of that genome alone against the genome."""
    members, copies = edge_references(genomes, {}, 18)[:2]
    _, gb, goff = genomes[4]
    comm, one, g = _native.Community(members, copies, 0), _native.Community([(gb, goff)], [1], 0), _native.Genome(gb, goff, 0)
    try:
        for kind in KINDS:
            for L in EDGE_LS:
                _, _, lid, k, want_c, m, want_g = edge_references(genomes, kind, L)
                for src in (comm, one, g):
                    src.set_library(**k)
                for n in EDGE_NS:
                    assert np.array_equal(comm.simulate(L, n, 9, lid, first=EDGE_FIRST), want_c[:n]), (kind, L, n)
                    assert np.array_equal(comm.member_reads(), np.bincount(m[:n], minlength=3)), (kind, L, n)
                    got = g.simulate(L, n, 9, lid, first=EDGE_FIRST)
                    assert np.array_equal(got, want_g[:n]), (kind, L, n)
                    assert one.simulate(L, n, 9, lid, first=EDGE_FIRST).tobytes() == got.tobytes(), (kind, L, n)
                    assert one.member_reads().tolist() == [n]
    finally:
        for src in (comm, one, g):
            src.close()


# ---- 7. fused == staged ---------------------------------------------------------------------------------------------------
COUNTS = ("reads", "seed_tasks", "gap_tasks", "hsps", "rows", "reads_with_rows", "classified")


def test_fused_library_equals_staged(genomes):
    members = [(b, o) for _, b, o in genomes]
    copies = uneven_copies(len(members))
    model = _native.load_model()
    n, L = 2 * STREAM_BATCH + 12345, 100
    assert "MC_STREAM_BATCH" not in os.environ
    comm = _native.Community(members, copies, 0)
    eng = _native.Engine(device=0)
    try:
        eng.set_run(L, model["pars"][str(L)], model["families"])
        lid = training.library_id("thirty", L)
        fused = eng.community_library(comm, n, 5, lid)
        fstats, fdrawn = eng.stats(), comm.member_reads()
        assert len(eng.rows()) == 0
        print("fused pass of %d reads: %s ms; %d best hits" % (n, eng.community_times(), len(fused)))
        reads = comm.simulate(L, n, 5, lid)
        assert np.array_equal(comm.member_reads(), fdrawn) and fdrawn.sum() == n
        eng.set_best_hits_only(True)
        _, staged = eng.search(reads)
        sstats = eng.stats()
        eng.set_best_hits_only(False)
        assert len(fused) > 1000
        assert fused.tobytes() == staged.tobytes()              # every field, same order
        print("stats fused %s\nstats staged %s" % ({k: fstats[k] for k in COUNTS}, {k: sstats[k] for k in COUNTS}))
        for k in COUNTS:
            assert fstats[k] == sstats[k], k
    finally:
        eng.close()
        comm.close()


# ---- 8. validate() == run_pipeline on the written metagenome ---------------------------------------------------------------
@pytest.mark.parametrize("kind", [dict(), dict(error_model="illumina", paired_end=True, insert=300)], ids=["default", "illumina-paired"])
def test_validate_equals_run_pipeline_on_the_written_reads(genomes, tmp_path, kind):
    gdir = tmp_path / "genomes"
    gdir.mkdir()
    for name, bases, off in genomes[:8]:
        write_fna(str(gdir / (name + ".fna.gz")), bases, off)
    cfile = tmp_path / "mock8.tsv"
    cfile.write_text("genome\tsize\trelative_abundance\n" + "".join("%s\t0\t%s\n" % (g[0], a) for g, a in zip(genomes[:8], ("0.3", "0.02", "0.1", "0.08", "0.25", "0.05", "0.15", "0.05"))))
    n, L = 60000, 150
    recs = validation.validate(str(gdir), str(tmp_path / "out"), [L], n, communities=[str(cfile)], seed=3, write_reads_dir=str(tmp_path / "reads"), **kind)
    assert len(recs) == 1 and recs[0]["community"] == "mock8" and recs[0]["members"] == 8 and recs[0]["reads"] == n
    copies = validation.copies_of([g[0] for g in genomes[:8]], ["0.3", "0.02", "0.1", "0.08", "0.25", "0.05", "0.15", "0.05"])
    assert recs[0]["true_ags"] == validation.true_ags(copies, [int(g[2][-1]) for g in genomes[:8]])
    assert sum(recs[0]["member_reads"]) == n
    path = str(tmp_path / "reads" / ("mock8_%d.fa.gz" % L))
    est, args = mc.run_pipeline({"seqfiles": [path], "nreads": n, "read_length": L, "device": 0})
    assert args["sampled_reads"] == n
    print("validate %r, run_pipeline %r, truth %r" % (recs[0]["est_ags"], est, recs[0]["true_ags"]))
    assert recs[0]["est_ags"] == est                            # same best hits, same summation order: equality
    assert recs[0]["error"] == (est - recs[0]["true_ags"]) / recs[0]["true_ags"]
    rows = training.read_map(str(tmp_path / "out" / "validation.map"), header=True)
    assert rows[0][:4] == ["mock8", str(L), "8", str(n)] and float(rows[0][5]) == est
    tsv = training.read_map(str(tmp_path / "out" / "communities" / "mock8.tsv"), header=True)
    assert [r[0] for r in tsv] == [g[0] for g in genomes[:8]] and [int(r[1]) for r in tsv] == copies and [int(r[3]) for r in tsv] == recs[0]["member_reads"]
    # the written file is the restatement's library
    members = [(b, o) for _, b, o in genomes[:8]]
    bases, off, mfirst = cr.join_members(members)
    want = cr.simulate(bases, off, mfirst, copies, L, 0, 3000, 3, training.library_id("mock8", L), **kind)[0]
    lines = gzip.open(path).read().split(b"\n")
    assert b"".join(lines[1:6000:2]) == want.tobytes()
    assert lines[0] == (b">0/1" if kind.get("paired_end") else b">0") and lines[2] == (b">0/2" if kind.get("paired_end") else b">1")


# ---- 9. against the reference itself --------------------------------------------------------------------------------------
def test_recorded_library_and_the_references_estimate(genomes):
    """tests/golden/community_golden.json (make_community_golden.py): the md5 of a library's reads as the g++ emulation made them, and
    the est_ags the reference's run_pipeline (its own rapsearch binary) returned for the file of those reads."""
    g = json.load(open(os.path.join(GOLD, "community_golden.json")))
    lib = g["library"]
    members = [(genomes[k][1], genomes[k][2]) for k in lib["genome_indices"]]
    comm = _native.Community(members, lib["copies"], 0)
    eng = _native.Engine(device=0)
    model = _native.load_model()
    try:
        comm.set_library(**lib["kind"])
        reads = comm.simulate(lib["read_len"], lib["nreads"], lib["seed"], lib["library_id"])
        assert hashlib.md5(reads.tobytes()).hexdigest() == g["reads_md5"]
        eng.set_run(lib["read_len"], model["pars"][str(lib["read_len"])], model["families"])
        best = eng.community_library(comm, lib["nreads"], lib["seed"], lib["library_id"])
        est = validation.estimate_of_best_hits(None, lib["read_len"], best, model["families"], lib["nreads"])
        truth = validation.true_ags(lib["copies"], [int(o[-1]) for _, o in members])
        print("reference est_ags %r, here %r, truth %r (%+.4f)" % (g["est_ags"], est, truth, (est - truth) / truth))
        assert truth == g["true_ags"]
        assert est == g["est_ags"]
    finally:
        eng.close()
        comm.close()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(genomes, tmp_path):
    """Every refusal comes with a message and leaves the handle's last run untouched (no launch).  A community on another device than
    the handle needs a second device to exist: that refusal is asserted where two are visible, and said to be unasserted otherwise."""
    lib = _native.load_library()
    name, bases, off = genomes[0]
    comm = _native.Community([(bases, off), (genomes[1][1], genomes[1][2])], [2, 5], 0)
    eng = _native.Engine(device=0)
    longest = max(int(np.max(np.diff(off))), int(np.max(np.diff(genomes[1][2]))))
    try:
        eng.set_run(150)
        eng.search(comm.simulate(150, 100, 1, 1))
        before = eng.stats()
        for rec, msg in [((0, 0, 7, 0.0), "unknown error model 7"), ((0, 0, 1, 1.5), "outside [0, 1]"), ((1, 0, 0, 0.0), "positive insert"),
                         ((1, longest + 1, 0, 0.0), "no contig of at least the insert")]:
            assert lib.mc_community_set_library(comm.c, C.byref(_native.McLibrary(*rec))) != 0
            assert msg in lib.mc_last_error().decode()
        comm.set_library(paired_end=True, insert=120)
        with pytest.raises(RuntimeError, match=r"insert \(120\) is shorter than the read length \(150\)"):
            comm.simulate(150, 10, 1, 1)
        with pytest.raises(RuntimeError, match=r"insert \(120\) is shorter than the read length \(150\)"):
            eng.community_library(comm, 1000, 1, 1)
        comm.set_library(paired_end=True, insert=300)
        with pytest.raises(RuntimeError, match="even number of reads"):
            eng.community_library(comm, 1001, 1, 1)
        if lib.mc_device_count() > 1:                          # a community on another device than the handle
            other = _native.Community([(bases, off)], [1], 1)
            try:
                with pytest.raises(RuntimeError, match="lies on another device than the handle"):
                    eng.community_library(other, 1000, 1, 1)
            finally:
                other.close()
        else:
            print("one device visible: the refusal of a community on another device cannot be provoked here")
        assert eng.stats() == before                           # no launch: the handle's last run is untouched
        # limits of mc_community_open, each with a message
        one = np.array([0, 1], np.int32)
        for copies, msg in [([0], "has 0 copies"), ([(1 << 20) + 1], "has 1048577 copies")]:
            assert not lib.mc_community_open(bases.ctypes.data_as(C.c_void_p), off[:2].ctypes.data_as(C.c_void_p), 1, one.ctypes.data_as(C.c_void_p),
                                             np.array(copies, np.int64).ctypes.data_as(C.c_void_p), 1, 0)
            assert msg in lib.mc_last_error().decode()
        tiny = _native.Community([(bases[:100], np.array([0, 100], np.int64))], [3], 0)
        try:
            with pytest.raises(RuntimeError, match=r"no contig of at least the read length \(150 bp\)"):
                tiny.simulate(150, 10, 1, 1)
        finally:
            tiny.close()
        # the reference read-length mode: refused before anything is opened
        gdir = tmp_path / "genomes"
        gdir.mkdir()
        write_fna(str(gdir / "g00.fna.gz"), bases, off)
        with pytest.raises(validation.ValidationError, match="reference read lengths"):
            validation.validate(str(gdir), str(tmp_path / "out"), [150], 1000, random=1, members=1, reference_lengths=True)
        comm.set_library()
        assert comm.simulate(150, 10, 1, 1).shape == (10, 150)
    finally:
        eng.close()
        comm.close()
