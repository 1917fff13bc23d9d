"""The piece cutter on the CPU: csrc/mc_pieces.h (g++ build, tests/emul/pieces.cpp) against a plain Python statement of its rule - the
bins of a sorted batch, each of one read length, cut into the ranges the fixed-length pipeline runs (mc_search_varlen, the class
runs, mc_train_library's reference read lengths).  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BATCH = 1000
COUNTS = [0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1]


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "pieces")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(HERE, "emul", "pieces.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "pieces", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "pieces_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _cut(bins, batch):
    """The rule, restated: (pieces, Lmax, nmax, nshort); a piece is (L, tag, bin_first, bin_n, first, n), tag the bin's place in the list."""
    pieces, lmax, nmax, nshort = [], 0, 0, 0
    for tag, (L, n, first) in enumerate(bins):
        if n == 0:
            continue
        if L < 18:
            nshort += n
            continue
        a = 0
        while a < n:
            pieces.append((L, tag, first, n, a, min(batch, n - a)))
            a += batch
        lmax, nmax = max(lmax, L), max(nmax, min(batch, n))
    return pieces, lmax, nmax, nshort


def _run(exe, bins, batch):
    arg = ",".join("%d:%d:%d" % b for b in bins) if bins else ","
    p = subprocess.run([exe, str(batch), arg], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    err = p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    lines = [[int(x) for x in line.split()] for line in p.stdout.decode().splitlines()]
    lmax, nmax, nshort, npieces = lines[0]
    assert npieces == len(lines) - 1
    return [tuple(x) for x in lines[1:]], lmax, nmax, nshort


def _bins(lengths_counts):
    """bins back to back: every bin's first position is where the one before ended (ascending)"""
    bins, at = [], 0
    for L, n in lengths_counts:
        bins.append((L, n, at))
        at += n
    return bins


CASES = {
    # every count at every length: 17 (short), 18 (the shortest searched), 510 (the longest)
    "counts-x-lengths": _bins([(L, n) for L in (17, 18, 510) for n in COUNTS]),
    "all-short": _bins([(1, 3), (5, BATCH + 1), (17, 2 * BATCH + 1)]),
    "empty-list": [],
    "only-empty-bins": _bins([(18, 0), (150, 0)]),
    "every-length": _bins([(L, (7 * L) % 13) for L in range(1, 512)]),           # the 511 buckets of a varlen batch, some empty
    "classes": _bins([(50, BATCH), (100, BATCH + 1), (150, 1)]),
    "longest-not-last": [(300, 5, 0), (18, 2 * BATCH + 1, 5), (150, 0, 2 * BATCH + 6), (17, 9, 2 * BATCH + 6)],
}
for _n in COUNTS:                                                                # one bin of every count, not from position 0
    CASES["one-bin-%d" % _n] = [(150, _n, 40)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cutter_is_the_restated_rule(driver, name):
    bins = CASES[name]
    for batch in (BATCH, 1, 2_000_000):
        if batch == 1 and sum(n for _, n, _ in bins) > 20_000:
            continue
        got = _run(driver, bins, batch)
        assert got == _cut(bins, batch)
        pieces, lmax, nmax, nshort = got
        # what the callers rely on: the pieces tile every searched bin in order, none is empty or larger than the batch, the pools fit
        assert nshort == sum(n for L, n, _ in bins if L < 18)
        assert sum(q[5] for q in pieces) == sum(n for L, n, _ in bins if L >= 18)
        assert all(0 < q[5] <= batch and q[4] + q[5] <= q[3] and q[0] <= lmax and q[5] <= nmax for q in pieces)
        assert [(q[1], q[4]) for q in pieces] == sorted((q[1], q[4]) for q in pieces)
        for q in pieces:
            assert (q[0], q[3], q[2]) == tuple(bins[q[1]])


def test_the_named_cases():
    """the restatement itself, by hand, at the edges of a bin and of the batch"""
    assert _cut(CASES["all-short"], BATCH) == ([], 0, 0, 3 + BATCH + 1 + 2 * BATCH + 1)
    assert _cut([(18, BATCH + 1, 7)], BATCH) == ([(18, 0, 7, BATCH + 1, 0, BATCH), (18, 0, 7, BATCH + 1, BATCH, 1)], 18, BATCH, 0)
    assert _cut([(17, 4, 0), (510, BATCH - 1, 4)], BATCH) == ([(510, 1, 4, BATCH - 1, 0, BATCH - 1)], 510, BATCH - 1, 4)
    pieces, lmax, nmax, nshort = _cut(CASES["longest-not-last"], BATCH)
    assert (lmax, nmax, nshort) == (300, BATCH, 9) and [q[5] for q in pieces] == [5, BATCH, BATCH, 1]


def test_cutter_under_sanitizers(driver_san):
    for name in ("counts-x-lengths", "all-short", "empty-list", "every-length", "longest-not-last"):
        assert _run(driver_san, CASES[name], BATCH) == _cut(CASES[name], BATCH)
