"""What a handle leaves behind (csrc/mc_owned.h, mc_debug_live): the device buffers, pinned host buffers, streams and events the
library holds in this process, counted where each is made and destroyed.  A handle's whole life - every entry point that allocates,
pools, staging and row slots grown on the way - ends at the counts it began with, and a call repeated with the same arguments holds
no more than the first one did.  All counts are differences from a reading at the start of the test: other modules' engines live in
the same process."""
import gc
import gzip
import os

import numpy as np
import pytest

import community_restated as cr
from microbecensus_amd import _native

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GRID = ([0.0, 0.5], [100, 90], [0.0, 30.0, 45.0])
CLASSES = [60, 80, 100]


@pytest.fixture(scope="module")
def reads():
    """the 100 bp reads of a golden case of the reference binary"""
    seqs = [l.rstrip(b"\r\n") for l in gzip.open(os.path.join(GOLD, "config1_example_fq.reads.fa.gz"), "rb") if not l.startswith(b">")]
    r = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), len(seqs[0]))
    assert r.shape[0] >= 6000 and r.shape[1] == 100
    return r


@pytest.fixture(scope="module")
def members():
    return [(b, o) for _, b, o in cr.fixture_members([0, 1])]


def live():
    gc.collect()                                                   # (an engine another module dropped without closing goes now, not between two readings)
    return np.array(_native.debug_live(), np.int64)


def mixed(reads):
    """about 1,500 reads of three lengths: as (bases, offsets) for search_varlen and as padded class rows"""
    rows = reads[:1500].copy()
    rows[500:1000, 80:] = 0
    rows[1000:, 60:] = 0
    lens = np.array([100] * 500 + [80] * 500 + [60] * 500, np.int64)
    offsets = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    return (np.concatenate([rows[i, :lens[i]] for i in range(len(lens))]), offsets), rows


def wfit_table():
    rng = np.random.Generator(np.random.PCG64(20261018))
    truth = rng.uniform(2e6, 6e6, 8)
    pred = truth[:, None] * rng.uniform(0.7, 1.3, (8, 4))
    return pred, truth, rng.uniform(0.0, 1.0, (16, 4))


class Steps:
    """the entry points of a handle that make something on the device, each as one call with fixed arguments"""

    def __init__(self, eng, reads, members, monkeypatch):
        self.eng, self.reads, self.mp = eng, reads, monkeypatch
        self.varlen, self.rows = mixed(reads)
        self.pred, self.truth, self.w = wfit_table()
        self.genome = _native.Genome(members[0][0], members[0][1], 0)
        self.genome.set_library(error_model="illumina")
        self.comm = _native.Community(members, [3, 1], 0)
        self.model = _native.load_model()

    def close(self):
        self.genome.close()
        self.comm.close()

    def set_run(self):
        self.eng.set_run(100, self.model["pars"]["100"], self.model["families"])

    def search(self, n, batch=6000):
        self.mp.setenv("MC_STREAM_BATCH", str(batch))
        rows, best = self.eng.search(self.reads[:n])
        assert len(best) > 0 and len(rows) >= len(best)
        return best

    def search_varlen(self):
        rows, best = self.eng.search_varlen(self.varlen)
        assert len(best) > 0

    def classes(self):
        self.eng.set_run_classes(CLASSES, {L: self.model["pars"][str(L)] for L in CLASSES}, self.model["families"])
        best, cls, class_reads = self.eng.search_classes(self.rows)
        assert list(class_reads) == [500, 500, 500, 0] and len(best) > 0
        self.set_run()

    def grid_classify(self):
        self.search(2000)                                            # (the grid runs on the rows of the last search)
        hits, _, _ = self.eng.grid_classify(*GRID)
        assert hits.sum() > 0

    def bootstrap(self):
        best = self.search(2000)
        si, _ = self.eng.bootstrap(best, [f % 3 for f in range(self.eng.nfam)], 64, 7)
        assert si[:, -1].sum() > 0

    def fit_weights(self):
        w, trace = self.eng.fit_weights(self.pred, self.truth, 11, 100, candidates=256, generations=4)
        assert ((w >= 0.0) & (w <= 1.0)).all() and w.sum() > 0.0 and trace.shape == (5, 3)

    def weights_mue(self):
        assert np.isfinite(self.eng.weights_mue(self.pred, self.truth, self.w)).all()

    def abundance(self):
        self.eng.set_abundance(True)
        self.search(2000)
        assert self.eng.abundance()["assigned"] > 0
        self.eng.set_abundance(False)

    def train(self, reference):
        self.genome.set_read_lengths(reference)
        self.eng.train_library(self.genome, 2000, 5, 1234, *GRID)
        assert self.eng.stats()["reads"] == 2000
        self.genome.set_read_lengths(False)

    def train_fixed(self):
        self.train(False)

    def train_reference(self):
        self.train(True)

    def community(self):
        self.eng.community_library(self.comm, 2000, 5, 99)
        assert self.eng.stats()["reads"] == 2000 and int(self.comm.member_reads().sum()) == 2000

    PER_CALL = ["search_varlen", "classes", "grid_classify", "bootstrap", "fit_weights", "weights_mue", "abundance", "train_fixed", "train_reference", "community"]


def test_a_handles_whole_life_leaves_nothing_behind(reads, members, monkeypatch):
    first = live()
    eng = _native.Engine(device=0)
    opened = live() - first
    assert (opened > 0).all(), opened                               # (the counters count: a handle holds some of every kind)
    s = Steps(eng, reads, members, monkeypatch)
    try:
        assert (live() - first)[0] > opened[0]                     # (the genome and the community hold device buffers of their own)
        s.set_run()
        s.search(2000, batch=2000)
        small = live() - first
        s.search(6000)                                               # pools, staging and row slots grow: replaced, not added
        assert ((live() - first) == small).all(), (small, live() - first)
        for name in Steps.PER_CALL:
            getattr(s, name)()
    finally:
        s.close()
        eng.close()
    assert (live() == first).all(), (first, live())


def test_repeated_calls_hold_steady(reads, members, monkeypatch):
    first = live()
    eng = _native.Engine(device=0)
    s = Steps(eng, reads, members, monkeypatch)
    try:
        s.set_run()
        s.search(6000)
        after_6000 = live()
        s.search(1000)
        s.search(6000)
        assert (live() == after_6000).all(), (after_6000 - first, live() - first)
        for name in Steps.PER_CALL:
            getattr(s, name)()
            once = live()
            getattr(s, name)()
            assert (live() == once).all(), (name, once - first, live() - first)
    finally:
        s.close()
        eng.close()
    assert (live() == first).all(), (first, live())
