"""Mock communities on the CPU: the draw the device runs (csrc/mc_simlib.h, compiled with g++ into tests/emul/community.cpp)
against its numpy restatement (community_restated.py) - places and reads of every library kind, the corners of the member table,
one member with one copy against the single-genome emulation, the members' proportions - and the host logic of
microbecensus_amd/validation.py (community files, copies, true AGS, random communities, refusals)."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import community_restated as cr
import simlib_restated as sr
from microbecensus_amd import _native, training, validation

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

KINDS = [
    dict(),
    dict(error_model="illumina"),
    dict(error_model="uniform", error_rate=0.05),
    dict(error_model="uniform", error_rate=0.6),              # many deletions: refused ones near the contigs' ends
    dict(error_model="uniform", error_rate=1.0),
    dict(paired_end=True, insert=300),
    dict(error_model="illumina", paired_end=True, insert=300),
    dict(error_model="uniform", error_rate=0.3, paired_end=True, insert=150),
]
KIND_IDS = ["-".join("%s" % v for v in k.values()) or "default" for k in KINDS]


def _build(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(HERE, "emul", name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "community")


@pytest.fixture(scope="module")
def genome_driver(tmp_path_factory):
    return _build(tmp_path_factory, "sim_library")


def run_driver(exe, tmp_path, bases, off, mfirst, copies, L, first, n, seed, lib, error_model=None, error_rate=None, paired_end=False, insert=None, check=True):
    files = {k: tmp_path / (k + ".bin") for k in ("bases", "off", "mfirst", "copies", "out", "places")}
    files["bases"].write_bytes(b"" if bases is None else np.asarray(bases, np.uint8).tobytes())
    files["off"].write_bytes(np.asarray(off, np.int64).tobytes())
    files["mfirst"].write_bytes(np.asarray(mfirst, np.int32).tobytes())
    files["copies"].write_bytes(np.asarray(copies, np.int64).tobytes())
    r = subprocess.run([exe] + [str(files[k]) for k in ("bases", "off", "mfirst", "copies")] +
                       [str(L), str(int(paired_end)), str(insert or 0), str(sr.MODELS[error_model]), repr(float(error_rate or 0.0)), str(seed), str(lib), str(first), str(n),
                        str(files["out"]), str(files["places"])], capture_output=True, text=True)
    if not check:
        return r
    assert r.returncode == 0, r.stderr
    places = np.frombuffer(files["places"].read_bytes(), dtype=np.int64).reshape(n, 3)
    reads = None if bases is None else np.frombuffer(files["out"].read_bytes(), dtype=np.uint8).reshape(n, L)
    return reads, places[:, 0], places[:, 1], places[:, 2]


def same(got, want, reads=True):
    if reads:
        assert np.array_equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(a, b)


# ---- 1. the g++ build of the draw == the numpy restatement ----------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_community():
    mem = cr.fixture_members([3, 0, 17, 8, 29])
    bases, off, mfirst = cr.join_members([(b, o) for _, b, o in mem])
    return bases, off, mfirst, [7, 1, 1 << 20, 300, 65000]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_draw_matches_restatement_on_fixture_genomes(driver, tmp_path, fixture_community, kind):
    bases, off, mfirst, copies = fixture_community
    for L in (100, 150):
        lid = training.library_id("five", L)
        want = cr.simulate(bases, off, mfirst, copies, L, 0, 3000, 9, lid, **kind)
        same(run_driver(driver, tmp_path, bases, off, mfirst, copies, L, 0, 3000, 9, lid, **kind), want)
        part = run_driver(driver, tmp_path, bases, off, mfirst, copies, L, 1001, 999, 9, lid, **kind)      # an odd start: a range may split a pair
        same(part, tuple(x[1001:2000] for x in want))
        assert len(set(want[1].tolist())) > 1
        if kind.get("paired_end"):
            assert np.array_equal(want[1][0::2], want[1][1::2]) and np.array_equal(want[3][0::2], want[3][1::2])     # both mates from one fragment of one member


def toy_members():
    """three toy genomes: the middle one has no contig of 150 bases"""
    a, oa = sr.toy_genome(5)
    b, ob = sr.toy_genome(6, lens=(120, 149, 30))
    c, oc = sr.toy_genome(7, lens=(151, 2000, 10, 150))
    return [(a, oa), (b, ob), (c, oc)]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_corners(driver, tmp_path, kind):
    bases, off, mfirst = cr.join_members(toy_members())
    copies = [1, 1 << 20, 1 << 20]                                    # copies 1 and 2^20 side by side
    span = kind.get("insert", 150)
    want = cr.simulate(bases, off, mfirst, copies, 150, 0, 4000, 3, 11, **kind)
    same(run_driver(driver, tmp_path, bases, off, mfirst, copies, 150, 0, 4000, 3, 11, **kind), want)
    if span >= 150:
        assert not np.any(want[1] == 1)                               # a member too short for the span is never drawn
    else:
        assert np.any(want[1] == 1)
    assert np.all(want[3] + span <= off[want[2] + 1]) and np.all(want[3] >= off[want[2]])
    L = 50 if span >= 50 else span                                    # at 50 bp (single end) every member has starts
    want = cr.simulate(bases, off, mfirst, copies, L, 0, 4000, 3, 11, **kind)
    same(run_driver(driver, tmp_path, bases, off, mfirst, copies, L, 0, 4000, 3, 11, **kind), want)
    # one member (with several copies: the same reads as with one)
    b1, o1 = toy_members()[2]
    m1 = np.array([0, len(o1) - 1], np.int32)
    one = run_driver(driver, tmp_path, b1, o1, m1, [1], 150, 0, 2000, 3, 11, **kind)
    same(one, cr.simulate(b1, o1, m1, [1], 150, 0, 2000, 3, 11, **kind))
    assert np.all(one[1] == 0)


def test_universe_just_under_2_62(driver, tmp_path):
    """A table without bases (places only): 2^20 copies x (2^42 - 1) valid starts, then one member more: 2^62 - 2^20 + 3."""
    L = 100
    big = (1 << 42) - 1 + L - 1
    off = np.array([0, big, big + 5 + L - 1, big + 5 + L - 1 + 50], np.int64)        # valid starts: 2^42 - 1, 5, 0
    mfirst = np.array([0, 1, 3], np.int32)
    copies = [1 << 20, 3]
    vstart, total, cum = cr.member_table(off, mfirst, copies, L)
    assert total == [(1 << 42) - 1, 5] and cum[-1] == (1 << 62) - (1 << 20) + 15 < 1 << 62
    want = cr.simulate(None, off, mfirst, copies, L, 12345, 20000, 1, 2, places_only=True)
    got = run_driver(driver, tmp_path, None, off, mfirst, copies, L, 12345, 20000, 1, 2)
    same(got, want, reads=False)
    assert np.all(want[3] + L <= off[want[2] + 1])
    # the same x by hand for the first rows: Python integers
    key = sr.mix64(1 ^ sr.mix64(2))
    for k in range(50):
        u = sr.mix64((key + 12345 + k) & sr.MASK) % cum[-1]
        m = 0 if u < cum[1] else 1
        v = (u - cum[m]) % total[m]
        assert (int(want[1][k]), int(want[3][k])) == (m, int(off[mfirst[m]]) + v)
    # 2^62 and beyond, and a universe of 0: refused
    r = run_driver(driver, tmp_path, None, off, mfirst, [1 << 20, 1 << 20], L, 0, 1, 1, 2, check=False)
    assert r.returncode == 5 and "2^62" in r.stderr
    r = run_driver(driver, tmp_path, None, np.array([0, 99, 150], np.int64), np.array([0, 1, 2], np.int32), [4, 4], L, 0, 1, 1, 2, check=False)
    assert r.returncode == 4 and "no contig of 100 bases" in r.stderr


# ---- 2. one member, one copy == the single-genome emulation ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_one_member_one_copy_is_the_genome_library(driver, genome_driver, tmp_path, kind):
    from test_sim_library_host import run_driver as run_genome
    cases = [sr.toy_genome()] + [(b, o) for _, b, o in cr.fixture_members([2])]
    for bases, off in cases:
        for L in (50, 150):
            if kind.get("insert", L) < L:
                continue
            lid = training.library_id("g02", L)
            want = run_genome(genome_driver, tmp_path, bases, off, L, 777, 2500, 5, lid, **kind)
            got = run_driver(driver, tmp_path, bases, off, np.array([0, len(off) - 1], np.int32), [1], L, 777, 2500, 5, lid, **kind)
            assert got[0].tobytes() == want.tobytes()
            assert np.array_equal(got[0], sr.simulate(bases, off, L, 777, 2500, 5, lid, **kind))


# ---- 3. the members' proportions ------------------------------------------------------------------------------------------
def test_member_proportions():
    """n = 10^6 rows of the restatement: every member's count within 6 x sqrt(n p (1 - p)) of n p, p = copies x total / universe
    (6 sigma of the binomial; two-sided tail 2e-9 per member)."""
    mem = cr.fixture_members()
    _, off, mfirst = cr.join_members([(b, o) for _, b, o in mem])
    rng = np.random.Generator(np.random.PCG64(20261016))
    copies = np.maximum(1, np.floor(rng.lognormal(0.0, 1.5, len(mem)) * 30000)).astype(np.int64).tolist()
    n, L = 1000000, 150
    _, m, c, s = cr.simulate(None, off, mfirst, copies, L, 0, n, 4, training.library_id("thirty", L), places_only=True)
    _, total, cum = cr.member_table(off, mfirst, copies, L)
    counts = np.bincount(m, minlength=len(mem))
    assert counts.sum() == n
    for k in range(len(mem)):
        p = copies[k] * total[k] / cum[-1]
        print("member %2d: copies %7d, p %.5f, expected %9.1f, drawn %7d, bound %.1f" % (k, copies[k], p, n * p, counts[k], 6 * np.sqrt(n * p * (1 - p))))
        assert abs(counts[k] - n * p) <= 6 * np.sqrt(n * p * (1 - p)), k
    # inside a member the starts are uniform over its valid starts: the mean of v / total is 1/2 (6 sigma of a uniform's mean)
    vs = np.array(cr.member_table(off, mfirst, copies, L)[0])
    k = int(np.argmax(counts))
    x = (s[m == k] - off[c[m == k]] + vs[c[m == k]]) / total[k]
    assert abs(x.mean() - 0.5) <= 6 * np.sqrt(1 / 12 / len(x))


# ---- 4. host logic --------------------------------------------------------------------------------------------------------
NAMES = ["g%02d" % i for i in range(30)]


def _write(tmp_path, text, name="mock.tsv"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_community_file(tmp_path):
    # laid out like the reference's community.txt: more columns than needed, in any order
    p = _write(tmp_path, "genome_name\tgenome_size\trelative_abundance\tnote\ng03\t123\t0.25\tx\ng00\t456\t0.5\ty\n\ng17\t789\t0.25\tz\n")
    mem, ab = validation.read_community(p, NAMES)
    assert mem == ["g03", "g00", "g17"] and ab == ["0.25", "0.5", "0.25"]
    assert validation.copies_of(mem, ab) == [250000, 500000, 250000]
    assert validation.community_name(p) == "mock"
    p = _write(tmp_path, "genome\tabundance\ng01\t3\ng02\t1e-1\n")
    assert validation.read_community(p, NAMES) == (["g01", "g02"], ["3", "1e-1"])


@pytest.mark.parametrize("text,msg", [
    ("genome\trelative_abundance\ng03\t0.5\ng99\t0.5\n", "no genome file for g99"),
    ("genome\trelative_abundance\ng03\t0.5\ng03\t0.5\n", "names g03 twice"),
    ("genome\tshare\ng03\t0.5\n", "no column headed relative_abundance or abundance"),
    ("genome\trelative_abundance\ng03\n", "the line of g03 has no abundance"),
    ("genome\trelative_abundance\n", "names no genome"),
    ("", "is empty"),
])
def test_community_file_refusals(tmp_path, text, msg):
    with pytest.raises(validation.ValidationError, match=msg):
        validation.read_community(_write(tmp_path, text), NAMES)


@pytest.mark.parametrize("ab,msg", [
    (["0.5", "-0.1"], "g01: abundance -0.1 is negative"),
    (["0.5", "nan"], "g01: abundance 'nan' is not a finite number"),
    (["inf", "1"], "g00: abundance 'inf' is not a finite number"),
    (["0.5", "abc"], "g01: abundance 'abc' is not a finite number"),
    (["1", "0.0000004"], "g01 comes to 0 copies"),
    (["1", "0"], "g01 comes to 0 copies"),
    (["0", "0"], "sum to 0"),
    ([1.0, float("nan")], "g01: abundance nan is not a finite number"),
])
def test_abundance_refusals(ab, msg):
    with pytest.raises(validation.ValidationError, match=msg):
        validation.copies_of(NAMES[:2], ab)


def test_copies_and_true_ags_are_exact():
    rng = np.random.default_rng(5)
    cases = [["0.1", "0.2", "0.7"], ["1", "1", "1"], ["0.0000005", "0.9999995"], ["3.3e-3", "12.5", "7"], ["0.5000005", "0.4999995"],
             [repr(float(x)) for x in rng.lognormal(0, 2, 20)], [float(x) for x in rng.lognormal(0, 1, 30)]]
    for ab in cases:
        names = NAMES[: len(ab)]
        fr = [Fraction(a) for a in ab]                                # (Fraction of a float is the float's exact value)
        tot = sum(fr)
        want = [int((a / tot * 1000000 + Fraction(1, 2)).__floor__()) for a in fr]
        copies = validation.copies_of(names, ab)
        assert copies == want
        sizes = [int(x) for x in rng.integers(500000, 12000000, len(ab))]
        exact = sum(Fraction(k * s) for k, s in zip(copies, sizes)) / sum(copies)
        num, den = validation.true_ags_fraction(copies, sizes)
        assert Fraction(num, den) == exact
        assert validation.true_ags(copies, sizes) == float(exact)
    assert validation.copies_of(["a", "b"], ["0.0000005", "0.9999995"]) == [1, 1000000]      # a half rounds up
    assert validation.true_ags([1, 3], [4000000, 2000000]) == 2500000.0


def test_random_communities():
    a = validation.random_community(NAMES, 3, 20, 1.0, 7)
    assert a == validation.random_community(NAMES, 3, 20, 1.0, 7)
    assert len(a[0]) == 20 and len(set(a[0])) == 20 and a[0] == sorted(a[0]) and all(x > 0 for x in a[1])
    others = [validation.random_community(NAMES, k, 20, 1.0, 7) for k in (0, 1, 2, 4)] + [validation.random_community(NAMES, 3, 20, 1.0, 8)]
    assert all(o != a for o in others) and all(o[1] != a[1] for o in others)
    # from (seed, k) alone: the stated generator
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([validation.RANDOM_TAG, 7, 3])))
    pick = np.sort(rng.choice(30, size=20, replace=False))
    assert a[0] == [NAMES[i] for i in pick] and a[1] == rng.lognormal(0.0, 1.0, size=20).tolist()
    assert validation.random_community(NAMES, 0, 30, 0.0, 1)[1] == [1.0] * 30
    with pytest.raises(validation.ValidationError, match="--members 31: there are 30 genomes"):
        validation.random_community(NAMES, 0, 31, 1.0, 0)


def test_summary():
    recs = [dict(read_length=100, error=e) for e in (0.01, -0.03, 0.02)] + [dict(read_length=150, error=None)]
    assert validation.unsigned_error_summary(recs) == {100: (0.02, 0.03), 150: (None, None)}


@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was opened")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Community", boom)


REFUSED = [
    (dict(reference_lengths=True), "reference read lengths .* are not supported"),
    (dict(read_lengths=[100, 123]), r"read length 123 is not one the model \(packaged\) was trained for: \[50, 60"),
    (dict(nreads=0), "must be positive"),
    (dict(error_model="uniform"), "needs an error rate"),
    (dict(error_rate=0.01), "only with the uniform error model"),
    (dict(error_model="sanger"), "unknown error model"),
    (dict(paired_end=True), "needs an insert"),
    (dict(insert=300), "only with a paired-end library"),
    (dict(paired_end=True, insert=120), "insert 120 is shorter than the read length 150"),
    (dict(paired_end=True, insert=300, nreads=1001), "even number of reads"),
    (dict(paired_end=True, insert=600), "community mock has no contig of at least 600 bp"),
    (dict(communities=None), "no community given"),
    (dict(communities=None, random=2), "--random needs --members"),
]


@pytest.mark.parametrize("kw,msg", REFUSED, ids=[m for _, m in REFUSED])
def test_validate_refusals(tmp_path, no_engine, kw, msg):
    from test_sim_library_host import _genome_dir
    gd = _genome_dir(tmp_path, 3)
    comm = _write(tmp_path, "genome\trelative_abundance\ng0\t1\ng2\t3\n")
    args = dict(read_lengths=[100, 150], nreads=1000, communities=[comm])
    args.update(kw)
    out = str(tmp_path / "out")
    with pytest.raises(validation.ValidationError, match=msg):
        validation.validate(gd, out, **args)
    assert not os.path.exists(out)


def test_cli_refusals(tmp_path):
    from test_sim_library_host import _genome_dir
    gd = _genome_dir(tmp_path, 2)
    comm = _write(tmp_path, "genome\trelative_abundance\ng0\t1\ng7\t3\n")
    script = os.path.join(REPO, "scripts", "validate_microbe_census.py")
    for extra, msg in [(["--communities", comm], "no genome file for g7"), (["--random", "2", "--members", "5"], "--members 5: there are 2 genomes"),
                       (["--random", "1", "--members", "2", "--reference-lengths"], "reference read lengths"),
                       (["--random", "1", "--members", "2", "--paired-end"], "needs an insert (--insert)")]:
        r = subprocess.run([sys.executable, script, gd, str(tmp_path / "o"), "-l", "150", "-n", "1000"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and msg in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "o")


def test_gzipped_reads_file(tmp_path):
    import gzip
    reads = np.frombuffer(b"AAAACCCCGGGGTTTT", np.uint8).reshape(4, 4)
    training.write_reads(str(tmp_path / "r" / "pe.fa.gz"), reads, paired_end=True)
    assert gzip.open(tmp_path / "r" / "pe.fa.gz").read() == b">0/1\nAAAA\n>0/2\nCCCC\n>1/1\nGGGG\n>1/2\nTTTT\n"
