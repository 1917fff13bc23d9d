"""Length classes on the CPU: the rule of csrc/mc_classes.h (g++ build, tests/emul/classes.cpp) against its numpy restatement
(classes_restated.py), the native class sampler against the Python statement of the rule, the pooled estimate, the default class
choice, the refusals and the report.  No GPU."""
import bz2
import gzip
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from microbecensus_amd import microbe_census as mc

import classes_restated as cr

HERE = os.path.dirname(os.path.abspath(__file__))
VALID = list(mc._valid_read_lengths())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("classes") / "classes")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "emul", "classes.cpp")])
    return exe


CLASS_LISTS = [[100], [18], [510], [50, 100, 150], VALID, list(range(18, 50)), [18 + 15 * k for k in range(32)], [70, 71, 72, 300, 509, 510]]


@pytest.mark.parametrize("cl", CLASS_LISTS, ids=lambda cl: "K%d-%d-%d" % (len(cl), cl[0], cl[-1]))
def test_rule_over_every_length(driver, cl):
    out = subprocess.check_output([driver, ",".join(str(x) for x in cl)]).decode().split("\n")
    assert out[0].split()[0] == "0"
    got = np.array([[int(x) for x in line.split()] for line in out[1:] if line])
    assert got.shape == (521, 4) and (got[:, 0] == np.arange(521)).all()
    lens = np.arange(521)
    assert (got[:, 1] == np.minimum(lens, cl[-1])).all()                       # the length the row carries
    want = cr.class_of(lens, cl)
    assert (got[:, 2] == want).all() and (got[:, 3] == want).all()             # cutting a read to the stride does not change its class
    # the numpy statement against the plain rule, and the package's own Python statement
    for n in range(521):
        fit = [k for k, L in enumerate(cl) if L <= n]
        assert want[n] == (fit[-1] if fit else len(cl))
        assert mc.class_of_length(cl, n) == (fit[-1] if fit else None)
    rows = cr.make_rows([b"A" * n for n in range(521)], cl[-1])
    assert (cr.row_len(rows) == np.minimum(lens, cl[-1])).all()


@pytest.mark.parametrize("cl,code,bad", [([], 1, 0), (list(range(18, 51)), 1, 33), ([17], 2, 17), ([100, 511], 2, 511), ([100, 100], 3, 100), ([150, 100], 3, 100)])
def test_illegal_lists_are_named(driver, cl, code, bad):
    arg = ",".join(str(x) for x in cl) if cl else ","
    assert subprocess.check_output([driver, arg]).decode().split("\n")[0].split() == [str(code), str(bad)]


# ---- the native class sampler against the Python statement -----------------------------------------------------------------------
SAMPLER_CLASSES = [50, 100, 150, 200, 300]


def _records(seed, n, fastq, qoff):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        length = rng.choice([rng.randint(30, 49), rng.randint(50, 99), rng.randint(100, 149), rng.randint(150, 199), rng.randint(200, 320)])
        seq = "".join(rng.choice("ACGT" if rng.random() < 0.9 else "ACGTN") for _ in range(length))
        if recs and rng.random() < 0.04:                                        # an exact duplicate of an earlier record
            seq = rng.choice(recs)[0]
        elif recs and rng.random() < 0.04:                                      # the reverse complement of one
            seq = rng.choice(recs)[0][::-1].translate(str.maketrans("ACGTN", "TGCAN"))
        qual = "".join(chr(qoff + (rng.randint(2, 40) if rng.random() < 0.97 else rng.randint(0, 6))) for _ in range(len(seq))) if fastq else None
        recs.append((seq, qual))
    return recs


def _write(path, recs, fastq, seed):
    rng = random.Random(seed)
    lines = []
    for i, (seq, qual) in enumerate(recs):
        if fastq:
            lines.append("@r%d\n%s\n+\n%s\n" % (i, seq, qual))
        else:                                                                   # multi-line records: the sequence folded at a width of its own
            w = rng.choice([60, 70, 1000])
            lines.append(">r%d some text\n%s\n" % (i, "\n".join(seq[a:a + w] for a in range(0, len(seq), w))))
    data = "".join(lines).encode()
    opener = gzip.open if path.endswith(".gz") else bz2.open if path.endswith(".bz2") else open
    with opener(path, "wb") as f:
        f.write(data)


SAMPLER_CASES = [
    ("fa", ".fa", False, 33, {}),
    ("fa-gz-dups", ".fa.gz", False, 33, {"filter_dups": True}),
    ("fa-bz2-u", ".fa.bz2", False, 33, {"max_unknown": 2}),
    ("fq33-q-m", ".fq", True, 33, {"min_quality": 3, "mean_quality": 19}),
    ("fq64-gz-m-dups", ".fq.gz", True, 64, {"mean_quality": 20, "filter_dups": True, "max_unknown": 3}),
    ("fq33-bz2-q", ".fq.bz2", True, 33, {"min_quality": 2}),
    ("fq33-small-n", ".fq", True, 33, {"nreads": 777, "filter_dups": True}),
    ("fa-small-n", ".fa", False, 33, {"nreads": 500}),
]


@pytest.mark.parametrize("name,ext,fastq,qoff,extra", SAMPLER_CASES, ids=[c[0] for c in SAMPLER_CASES])
def test_native_class_sampler_matches_the_python_statement(name, ext, fastq, qoff, extra, tmp_path):
    from microbecensus_amd import _native
    recs = _records(zlib.crc32(name.encode()), 3000, fastq, qoff)
    # the file puts enough records in every class, and below the lowest one
    lens = np.array([len(s) for s, _ in recs])
    per_class = np.bincount(cr.class_of(lens, SAMPLER_CLASSES), minlength=len(SAMPLER_CLASSES) + 1)
    assert (per_class[:len(SAMPLER_CLASSES)] >= 200).sum() >= 4 and per_class[-1] >= 50
    path = str(tmp_path / ("reads" + ext))
    _write(path, recs, fastq, 5)
    args = {"seqfiles": [path], "verbose": False, "read_length": 100}
    args.update(extra)
    mc.impute_missing_args(args)
    assert args["file_type"] == ("fastq" if fastq else "fasta")
    args["length_classes"] = SAMPLER_CLASSES
    py_fa, nat_fa = str(tmp_path / "py.fa"), str(tmp_path / "nat.fa")
    want_rows, want = mc._process_seqfile_py(args, {"tempfile": py_fa})
    rd = _native.Reader.with_classes(args["seqfiles"], SAMPLER_CLASSES, args["nreads"], fastq, args.get("quality_offset") or 0, args["min_quality"], args["mean_quality"],
                                     args["max_unknown"], args["filter_dups"], nat_fa)
    try:
        n = rd.run()
        st = rd.stats()
        assert rd.read_len == SAMPLER_CLASSES[-1]
        rows = rd.reads(n).copy()
    finally:
        rd.close()
    assert (st["sampled"], st["too_short"], st["low_qual"], st["dups"]) == (want["sampled"], want["too_short"], want["low_qual"], want["dups"])
    assert want["sampled"] > 300 and want["too_short"] >= 50
    if "nreads" in extra:
        assert want["sampled"] == extra["nreads"]                              # the sample got full in the middle of the file
    if args["filter_dups"]:
        assert want["dups"] > 20
    if extra.get("min_quality", -5) > -5 or extra.get("mean_quality", -5) > -5 or extra.get("max_unknown", 100) < 100:
        assert want["low_qual"] > 20
    assert rows.shape == want_rows.shape and (rows == want_rows).all()
    assert open(nat_fa).read() == open(py_fa).read()
    # every row is its class length long, and the classes are all in use
    rl = cr.row_len(rows)
    assert np.isin(rl, SAMPLER_CLASSES).all() and len(set(rl.tolist())) >= 4


def test_class_reader_refuses_illegal_lists():
    from microbecensus_amd import _native
    for cl, word in (([], "0 length classes"), (list(range(18, 51)), "33 length classes"), ([17], "17"), ([100, 511], "511"), ([150, 100], "100")):
        with pytest.raises(RuntimeError, match=word):
            _native.Reader.with_classes([__file__], cl, 10, False, 0, -5, -5, 100, False)


# ---- the pooled estimate ----------------------------------------------------------------------------------------------------------
MODEL = mc._model()
FAMS = MODEL["families"]


def _sums(seed, scale):
    rng = random.Random(seed)
    return {f: float(rng.randint(20, 60) * scale) for f in rng.sample(FAMS, len(FAMS))}


def test_one_class_is_ags_of_sums_bit_for_bit():
    for L in (100, 150):
        s = _sums(L, 3)
        want = mc._ags_of_sums(MODEL, L, s, 12345 * L)
        assert mc.pooled_ags(MODEL, [L], [12345], [s]) == want
        # ... and where the other classes hold no read at all
        assert mc.pooled_ags(MODEL, [70, L, 200], [0, 12345, 0], [{}, s, {}]) == want


def _per_class(L, n, s):
    return {f: MODEL["coefficients"]["%s_%s" % (L, f)] / (v / (n * L)) for f, v in s.items() if v}


def _pooled_parts(cl, n, sums):
    """est_f and w_f of the pooled estimate, restated"""
    B = sum(nk * L for nk, L in zip(n, cl) if nk)
    est, w = {}, {}
    for f in FAMS:
        x = 0.0
        for L, nk, s in zip(cl, n, sums):
            if nk:
                x += s.get(f, 0) / MODEL["coefficients"]["%s_%s" % (L, f)]
        if x:
            est[f] = B / x
            w[f] = sum(nk * L * MODEL["weights"]["%s_%s" % (L, f)] for L, nk in zip(cl, n) if nk) / B
    return est, w


def test_est_f_lies_between_the_per_class_estimates():
    cl, n = [80, 100, 150], [4000, 9000, 5000]
    sums = [_sums(1, 2), _sums(2, 5), _sums(3, 4)]
    est, w = mc.pooled_family_estimates(MODEL, cl, n, sums)                     # what pooled_ags itself uses
    want_est, want_w = _pooled_parts(cl, n, sums)                               # the independent restatement
    assert set(est) == set(want_est) == set(FAMS)
    for f in FAMS:
        assert abs(est[f] - want_est[f]) <= 1e-12 * want_est[f] and abs(w[f] - want_w[f]) <= 1e-12 * want_w[f]
    per = [_per_class(L, nk, s) for L, nk, s in zip(cl, n, sums)]
    for f, e in est.items():
        lo, hi = min(p[f] for p in per), max(p[f] for p in per)
        assert lo * (1 - 1e-12) <= e <= hi * (1 + 1e-12)


def test_a_class_without_hits_raises_the_estimate():
    cl, sums = [100, 150], [_sums(2, 5), _sums(3, 4)]
    a = mc.pooled_ags(MODEL, cl, [9000, 5000], sums)
    b = mc.pooled_ags(MODEL, cl + [200], [9000, 5000, 3000], sums + [{}])
    ea, _ = mc.pooled_family_estimates(MODEL, cl, [9000, 5000], sums)
    eb, _ = mc.pooled_family_estimates(MODEL, cl + [200], [9000, 5000, 3000], sums + [{}])
    assert set(ea) == set(eb) == set(FAMS)
    for f in ea:
        assert eb[f] > ea[f]
        assert abs(eb[f] / ea[f] - (9000 * 100 + 5000 * 150 + 3000 * 200) / (9000 * 100 + 5000 * 150)) < 1e-12     # B grows, x_f does not
    assert b > a
    # a family without a hit in any class is left out; the order is that of the first hit, k ascending
    some = [{FAMS[2]: 3.0}, {FAMS[0]: 2.0, FAMS[2]: 1.0}]
    e, _ = mc.pooled_family_estimates(MODEL, cl, [10, 10], some)
    assert list(e) == [FAMS[2], FAMS[0]]


def test_three_classes_by_hand():
    cl, n = [80, 100, 150], [4000, 9000, 5000]
    sums = [_sums(1, 2), _sums(2, 5), _sums(3, 4)]
    del sums[0][FAMS[3]]                                                       # a family one class has no hit of
    est, w = _pooled_parts(cl, n, sums)
    vals = sorted(est.values())
    m = len(vals)
    med = vals[m // 2] if m % 2 else (vals[m // 2 - 1] + vals[m // 2]) / 2
    dev = sorted(abs(v - med) for v in vals)
    madv = 1.48 * (dev[m // 2] if m % 2 else (dev[m // 2 - 1] + dev[m // 2]) / 2)
    keep = [f for f in est if abs(est[f] - med) < madv]
    assert 0 < len(keep) < len(est)
    want = sum(est[f] * w[f] for f in keep) / sum(w[f] for f in keep)
    got = mc.pooled_ags(MODEL, cl, n, sums)
    assert abs(got - want) <= 1e-12 * want
    # the figure itself, from the packaged model
    assert got == mc.pooled_ags(MODEL, cl, n, [dict(s) for s in sums])


# ---- the default class choice, the refusals, the report --------------------------------------------------------------------------
def _fasta(path, lengths):
    with open(path, "w") as f:
        for i, n in enumerate(lengths):
            f.write(">%d\n%s\n" % (i, "ACGT" * (n // 4) + "A" * (n % 4)))
    return str(path)


def test_default_classes_keep_the_lengths_one_percent_fall_in(tmp_path):
    lengths = [80 + i % 71 for i in range(2000)] + [400] * 5 + [30] * 100     # spread over 80 .. 150, a few stray long reads, some too short
    got = mc.auto_detect_length_classes(_fasta(tmp_path / "a.fa", lengths), VALID)
    want = [L for k, L in enumerate(VALID) if 100 * int((cr.class_of(lengths, VALID) == k).sum()) >= len(lengths)]
    assert got == want and got[0] <= 80 and got[-1] == 150 and len(got) >= 4
    with pytest.raises(SystemExit, match="Median read length is 40"):
        mc.auto_detect_length_classes(_fasta(tmp_path / "b.fa", [40] * 50), VALID)


def test_switch_refusals(tmp_path):
    path = _fasta(tmp_path / "a.fa", [100, 150] * 50)
    base = {"seqfiles": [path], "mixed_lengths": True}
    for extra, word in (({"bootstrap": 10}, "--bootstrap"), ({"curve": 3}, "--curve"), ({"rapsearch": "/bin/true"}, "-r"), ({"keep_tmp": True}, "keep_tmp"),
                        ({"read_length": 100}, "-l 100")):
        with pytest.raises(SystemExit, match=word):
            mc.check_mixed_lengths(dict(base, **extra))
    with pytest.raises(SystemExit, match=r"\[101\]"):
        mc.check_mixed_lengths(dict(base, mixed_lengths=[100, 101]))
    args = dict(base, mixed_lengths=[150, 100])
    mc.check_mixed_lengths(args)
    assert args["length_classes"] == [100, 150] and args["read_length"] == "mixed"
    args = dict(base)
    mc.check_mixed_lengths(args)
    assert args["length_classes"] == [100, 150]
    # run_pipeline refuses before any GPU work: the exit comes from the check, whatever device there is
    with pytest.raises(SystemExit, match="--bootstrap"):
        mc.run_pipeline({"seqfiles": [path], "outfile": str(tmp_path / "o.txt"), "mixed_lengths": True, "bootstrap": 5})
    from microbecensus_amd import distributed
    for switch in (True, [100, 150], []):
        with pytest.raises(SystemExit, match="run_pipeline_distributed has no class form"):
            distributed.run_pipeline_distributed({"seqfiles": [path], "outfile": str(tmp_path / "d.txt"), "mixed_lengths": switch})
    # an empty list is a refused list, not "off"
    with pytest.raises(SystemExit, match="Length classes"):
        mc.check_mixed_lengths(dict(base, mixed_lengths=[]))
    with pytest.raises(SystemExit, match="Length classes"):
        mc.run_pipeline({"seqfiles": [path], "outfile": str(tmp_path / "e.txt"), "mixed_lengths": []})
    assert mc.mixed_lengths_on({"mixed_lengths": []}) and not mc.mixed_lengths_on({"mixed_lengths": None}) and not mc.mixed_lengths_on({})


PLAIN = ("Parameters\nmetagenome:\ta,b\nreads_sampled:\t5\ntrimmed_length:\t100\nmin_quality:\t-5\nmean_quality:\t-5\n"
         "filter_dups:\tFalse\nmax_unknown:\t100\n\nResults\naverage_genome_size:\t3051745.7641809303\ntotal_bases:\t980306\n"
         "genome_equivalents:\t0.32122793828571367\n")


def _report(tmp_path, name, **extra):
    args = {"outfile": str(tmp_path / name), "seqfiles": ["a", "b"], "sampled_reads": 5, "read_length": 100, "min_quality": -5, "mean_quality": -5,
            "filter_dups": False, "max_unknown": 100}
    args.update(extra)
    mc.report_results(args, 3051745.7641809303, 980306)
    return open(args["outfile"]).read()


def test_report(tmp_path):
    assert _report(tmp_path, "a.txt") == PLAIN
    assert _report(tmp_path, "b.txt", mixed_lengths=None, length_classes=[100], class_reads=[5]) == PLAIN     # figures left in args do not leak
    text = _report(tmp_path, "c.txt", mixed_lengths=True, read_length="mixed", length_classes=[100, 150], class_reads=[2, 3])
    assert text == PLAIN.replace("trimmed_length:\t100\n", "trimmed_length:\tmixed\n").replace("max_unknown:\t100\n", "max_unknown:\t100\nlength_classes:\t100\t150\n") \
                        .replace("average_genome_size:\t3051745.7641809303\n", "average_genome_size:\t3051745.7641809303\nclass_reads:\t2\t3\n")


def test_command_line_switch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_microbe_census", os.path.join(os.path.dirname(HERE), "scripts", "run_microbe_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_arguments(["in.fq", "out.txt"])["mixed_lengths"] is None
    assert mod.parse_arguments(["in.fq", "out.txt", "--mixed-lengths"])["mixed_lengths"] is True
    assert mod.parse_arguments(["--mixed-lengths", "100,150", "in.fq", "out.txt"])["mixed_lengths"] == [100, 150]


# ---- scoring on mixed-length communities (validate --length-mix) ------------------------------------------------------------------
def test_length_mix_is_parsed_and_refused():
    from microbecensus_amd import validation
    assert validation.parse_length_mix("150:0.5,100:0.5") == [(100, 0.5), (150, 0.5)]
    assert validation.mix_label(validation.parse_length_mix("100:0.25,150:0.5,300:0.25")) == "100+150+300"
    for text, word in (("100", "expected"), ("100:a", "expected"), ("100:0.5,100:0.5", "twice"), ("100:0.5,150:0.6", "add up"), ("100:1.5,150:-0.5", "positive")):
        with pytest.raises(validation.ValidationError, match=word):
            validation.parse_length_mix(text)
    # a length the model lacks is refused, before any GPU work; so is a class with an odd number of mates
    with pytest.raises(validation.ValidationError, match="read length 101 is not one the model"):
        validation.check_request([], 1000, VALID, "(packaged)", length_mix=[(101, 0.5), (150, 0.5)])
    with pytest.raises(validation.ValidationError, match="no read length given"):
        validation.check_request([], 1000, VALID, "(packaged)")
    with pytest.raises(validation.ValidationError, match="even number"):
        validation.check_request([], 1002, VALID, "(packaged)", paired_end=True, insert=400, length_mix=[(100, 0.5), (150, 0.5)])
    validation.check_request([], 1000, VALID, "(packaged)", length_mix=[(100, 0.5), (150, 0.5)])
    # the summary keeps the single lengths in front of the mixed rows
    recs = [{"read_length": "100+150", "error": -0.02}, {"read_length": 150, "error": 0.01}, {"read_length": 100, "error": 0.03}]
    assert list(validation.unsigned_error_summary(recs)) == [100, 150, "100+150"]
