"""Host side of the training workflow (no GPU): the parameter fit against the reference's own functions, the simulator's
stated formula, the marker set of a --gene-fams directory, the model writer, and the refusals of a training run."""
import gzip
import json
import os

import numpy as np
import pytest

from microbecensus_amd import _native, training
from microbecensus_amd import microbe_census as mc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MASK = (1 << 64) - 1


# ---- 1. the fit ---------------------------------------------------------------------------------------------------------------
def _cases():
    with gzip.open(os.path.join(GOLD, "training_fit.json.gz"), "rt") as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("ci", [0, 1])
def test_fit_matches_reference(ci):
    case = _cases()[ci]
    genomes, x = case["genomes"], case["xfolds"]
    sizes = [case["sizes"][g] for g in genomes]
    lib_bp = np.array([case["library_bp"][g] for g in genomes], dtype=np.float64)
    cands = training.candidates()
    for L, fams in case["expected"].items():
        for fam, want in fams.items():
            counts = np.array(case["counts"][L][fam], dtype=np.float64)
            rates = counts / lib_bp[:, None]
            k, err, coeff, preds, errors = training.fit(rates, sizes, x)
            s, p, c, t = cands[k]
            assert [s, p, c, "rate_" + t] == want["pars"] and k == want["index"]
            assert coeff == want["coefficient"]
            assert ["NA" if v is None else v for v in preds] == want["preds"]
            np.testing.assert_allclose(errors, want["errors"], rtol=1e-12, atol=0)
            assert err == min(want["errors"])


def test_rates_by_candidate_order():
    shape = (4, 6, 27, 2)
    rng = np.random.default_rng(1)
    hits, aln = rng.integers(0, 9, shape), rng.integers(0, 900, shape)
    cov = rng.random(shape)
    r = training.rates_by_candidate([hits], [aln], [cov], [1000])
    for k, (s, p, c, t) in enumerate(training.candidates()[:300]):
        ic, ip, isc = training.ALN_COVS.index(c), training.MAX_PIDS.index(p), training.MIN_SCORES.index(s)
        src = {"hits": hits, "aln": aln, "cov": cov}[t]
        assert r[0, 1, k] == src[ic, ip, isc, 1] / 1000.0


def test_xfold_indexes_leftovers():
    train, test = training.xfold_indexes(12, 5, 5)
    assert test == [8, 9] and train == [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]


# ---- 2. the simulator's formula (csrc/k_simulate.h), restated in numpy -----------------------------------------------------------
def mix64(z):
    z = (int(z) + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def simulate_np(bases, off, L, first, n, seed, lib):
    lens = np.diff(off)
    vstart = np.zeros(len(lens) + 1, dtype=np.int64)
    vstart[1:] = np.cumsum(np.maximum(0, lens - L + 1))
    key = mix64(seed ^ mix64(lib))
    u = np.array([mix64((key + i) & MASK) % int(vstart[-1]) for i in range(first, first + n)], dtype=np.int64)
    c = np.searchsorted(vstart, u, side="right") - 1
    s = off[c] + (u - vstart[c])
    return bases[s[:, None] + np.arange(L)[None, :]], s, c


def _toy_genome():
    rng = np.random.default_rng(5)
    lens = [30, 400, 5, 1200, 151, 149]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, int(off[-1]))]
    return bases, off


def test_simulator_reads_lie_in_their_contig():
    bases, off = _toy_genome()
    for L in (50, 150):
        reads, s, c = simulate_np(bases, off, L, 0, 3000, 3, 9)
        assert np.all(s + L <= off[c + 1]) and np.all(s >= off[c])
        for i in range(0, 3000, 97):
            assert reads[i].tobytes() == bases[s[i]: s[i] + L].tobytes()
        assert set(np.unique(c)) <= {i for i in range(len(off) - 1) if off[i + 1] - off[i] >= L}


def test_simulator_windows_and_libraries():
    bases, off = _toy_genome()
    whole = simulate_np(bases, off, 100, 0, 500, 1, 2)[0]
    for cut in (1, 137, 499):
        a = simulate_np(bases, off, 100, 0, cut, 1, 2)[0]
        b = simulate_np(bases, off, 100, cut, 500 - cut, 1, 2)[0]
        assert np.array_equal(np.concatenate([a, b]), whole)
    assert not np.array_equal(simulate_np(bases, off, 100, 0, 500, 1, 3)[0], whole)
    assert not np.array_equal(simulate_np(bases, off, 100, 0, 500, 2, 2)[0], whole)


def test_library_size_rounds_half_away():
    assert training.py2_round(2.5) == 3.0 and training.py2_round(3.5) == 4.0 and training.py2_round(-2.5) == -3.0
    assert training.py2_round(2.4999999) == 2.0 and training.py2_round(0.49999999999999994) == 0.0
    assert training.library_reads(10, 150, 100) == 15          # 15.0
    assert training.library_reads(1, 250, 100) == 3            # 2.5 -> 3 (Python 3's round would give 2)
    assert training.library_reads(1, 350, 100) == 4            # 3.5 -> 4
    assert training.library_reads(10, 84_700_000, 150) == 5_646_667


# ---- 3. the marker set of a --gene-fams directory ------------------------------------------------------------------------------
def test_marker_set_from_family_files(tmp_path):
    """The packaged markers written back one file per family: files in packaged order, so a marker goes to the file it was read
    from - the smallest marker_family at or behind it.  One marker (ARCH67_P638154538) lies in family 6's file although gene_fam.map
    (the packaged marker_family) puts it in family 28: --gene-fams names a marker's family by its file, so it is the one difference."""
    names, seqs = _native.load_markers()
    model = _native.load_model()
    fams = model["families"]
    origin = np.minimum.accumulate(np.array(model["marker_family"])[::-1])[::-1].tolist()
    for fi, fam in enumerate(fams):
        with gzip.open(tmp_path / (fam + ".faa.gz"), "wt") as f:
            first = True
            for nm, sq, of in zip(names, seqs, origin):
                if of == fi:
                    f.write(">%s some description\n" % nm)
                    for j in range(0, len(sq), 60):
                        f.write(sq[j: j + 60] + "\n")
                    if first and fi > 0:           # a sequence of the first family again, under another name: dropped
                        f.write(">dup_%d\n%s\n" % (fi, seqs[0]))
                    first = False
    n2, s2, f2, fam2 = training.build_marker_set(training.list_families(str(tmp_path)))
    assert n2 == names and s2 == seqs and fam2 == fams and f2 == origin
    diff = [i for i, (a, b) in enumerate(zip(f2, model["marker_family"])) if a != b]
    assert [(names[i], fams[f2[i]], fams[model["marker_family"][i]]) for i in diff] == [("ARCH67_P638154538", fams[6], fams[28])]


# ---- 4. the model writer ---------------------------------------------------------------------------------------------------------
def test_model_writer_round_trip(tmp_path):
    names, seqs, mf, fams = training.packaged_marker_set()
    pk = _native.load_model()
    pars = {"150": {f: [0.25, 70.0, 35.0, "hits"] for f in fams}, "125": {f: [0.5, 100.0, 41.0, "cov"] for f in fams}}
    coeff = {"%s_%s" % (L, f): 1.0 + i / 7.0 for i, (L, f) in enumerate((L, f) for L in ("125", "150") for f in fams)}
    weights = {k: 1.0 for k in coeff}
    sizes = {"gA": 3_000_000, "gB": 4_500_123}
    preds = [(150, fams[0], "gA", 2.5e6 / 3.0), (150, fams[0], "gB", None)]
    d = str(tmp_path / "m")
    training.write_model(d, names, seqs, mf, fams, [150, 125], pars, coeff, weights, sizes, preds)
    m = _native.load_model(os.path.join(d, "model.json"))
    assert sorted(m) == sorted(pk) and m["read_lengths"] == [125, 150]
    assert _native.load_markers(os.path.join(d, "markers.faa.gz")) == (names, seqs)
    assert m["marker_family"] == pk["marker_family"] and m["families"] == pk["families"]
    assert mc.find_opt_pars(d, 125)[fams[2]] == {"min_cov": 0.5, "max_aaid": 100.0, "min_score": 41.0, "aln_stat": "cov"}
    assert mc.find_opt_pars(None, 150) == {f: {"min_cov": p[0], "max_aaid": p[1], "min_score": p[2], "aln_stat": p[3]} for f, p in pk["pars"]["150"].items()}
    assert mc._valid_read_lengths(d) == [125, 150] and mc._valid_read_lengths() == mc.VALID_READ_LENGTHS
    rows = training.read_map(os.path.join(d, "pars.map"), header=True)
    assert {(r[1], r[0]): [float(r[2]), float(r[3]), float(r[4]), r[5]] for r in rows} == {(L, f): v for L, fp in pars.items() for f, v in fp.items()}
    assert {r[0]: float(r[1]) for r in training.read_map(os.path.join(d, "coefficients.map"))} == coeff
    assert {r[0]: float(r[1]) for r in training.read_map(os.path.join(d, "weights.map"))} == weights
    assert [int(r[0]) for r in training.read_map(os.path.join(d, "read_len.map"))] == [125, 150]
    assert [r for r in training.read_map(os.path.join(d, "gene_fam.map"))] == [[n, fams[f]] for n, f in zip(names, mf)]
    assert [r for r in training.read_map(os.path.join(d, "gene_len.map"))] == [[n, str(len(s))] for n, s in zip(names, seqs)]
    got = training.read_map(os.path.join(d, "training_preds.map"), header=True)
    assert got == [["150", fams[0], "gA", "3000000", repr(2.5e6 / 3.0)], ["150", fams[0], "gB", "4500123", "NA"]]


# ---- 5. refusals, before any engine is opened -------------------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was opened")
    monkeypatch.setattr(_native, "Engine", boom)
    monkeypatch.setattr(_native, "Genome", boom)


def _genome_dir(tmp_path, n, contig=500):
    d = tmp_path / "genomes"
    d.mkdir(exist_ok=True)
    for i in range(n):
        with gzip.open(d / ("g%d.fna.gz" % i), "wt") as f:
            f.write(">c\n%s\n" % ("ACGT" * (contig // 4)))
    return str(d)


def test_refusals(tmp_path, no_engine):
    out = str(tmp_path / "out")
    gd = _genome_dir(tmp_path, 3)
    with pytest.raises(training.TrainingError, match="at least 4 genomes"):
        training.train(gd, out, [100], 10, xfolds=4)
    for L in (17, 511):
        with pytest.raises(training.TrainingError, match="outside 18..510"):
            training.train(gd, out, [L], 10, xfolds=2)
    with pytest.raises(training.TrainingError, match="no contig of at least 510 bp"):
        training.train(gd, out, [510], 10, xfolds=2)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(training.TrainingError, match="is empty"):
        training.train(str(empty), out, [100], 10, xfolds=1)
    (tmp_path / "genomes" / "x.fa.gz").write_bytes(b"")
    with pytest.raises(training.TrainingError, match=r"\.fna\.gz extension"):
        training.train(gd, out, [100], 10, xfolds=1)
    os.remove(tmp_path / "genomes" / "x.fa.gz")
    fd = tmp_path / "fams"
    fd.mkdir()
    for i in range(33):
        with gzip.open(fd / ("f%02d.faa.gz" % i), "wt") as f:
            f.write(">m%d\nMKV%sL\n" % (i, "A" * i))
    with pytest.raises(training.TrainingError, match="at most 32"):
        training.train(gd, out, [100], 10, gene_fams_dir=str(fd), xfolds=2)
    os.remove(fd / "f32.faa.gz")
    (fd / "f99.fasta").write_text(">m\nMK\n")
    with pytest.raises(training.TrainingError, match=r"\.faa\.gz extension"):
        training.train(gd, out, [100], 10, gene_fams_dir=str(fd), xfolds=2)
    os.remove(fd / "f99.fasta")
    big = tmp_path / "big"
    big.mkdir()
    with gzip.open(big / "f.faa.gz", "wt") as f:
        for i in range(32768):
            f.write(">m%d\nM%s\n" % (i, np.base_repr(i, 20)))
    with pytest.raises(training.TrainingError, match="at most 32767"):
        training.train(gd, out, [100], 10, gene_fams_dir=str(big), xfolds=2)
    assert not os.path.exists(out)


def test_cli_refusal_message(tmp_path, capsys):
    import subprocess
    import sys
    gd = _genome_dir(tmp_path, 2)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "scripts", "train_microbe_census.py"), gd, str(tmp_path / "o"), "-l", "100", "-c", "10"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "10-fold cross-validation needs at least 10 genomes; 2 given" in r.stderr


def test_model_dir_refused_without_its_files(tmp_path):
    with pytest.raises(SystemExit, match="lacks markers.faa.gz"):
        mc.check_model_dir(str(tmp_path))
