"""The lookahead's bookkeeping on the CPU: csrc/mc_ahead.h (g++ build, tests/emul/ahead.cpp) against a plain Python statement of its
rule - which range is expected next, and when a range that is begun may use the frames a lookahead has translated.  No GPU."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
VALUES = [0, 1, 9, 10, 11, 1000]
FIELDS = ("reads_gen", "first", "count", "read_len", "FP", "tables_gen")
KEY = dict(reads_gen=7, first=2000, count=2000, read_len=150, FP=52, tables_gen=3)


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "ahead")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(HERE, "emul", "ahead.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "ahead", ["-O2"])


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory, "ahead_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


class Model:
    """The rule, restated: one lookahead at most; every operation answers with the line the driver prints."""

    def __init__(self):
        self.key = None

    @staticmethod
    def predict(first, count, nreads):
        if first < 0 or count <= 0 or first + count > nreads:
            return 0, 0                                                 # not a range of the set
        n = min(count, nreads - (first + count))
        return (n, first + count) if n > 0 else (0, 0)

    def covered(self, want):
        """the reads of the begun range whose frames the lookahead holds: a prefix of it, all of it, or nothing"""
        k = self.key
        if k is None or want["count"] <= 0 or k["count"] <= 0 or any(k[f] != want[f] for f in FIELDS if f != "count"):
            return 0
        return min(k["count"], want["count"])

    def run(self, op):
        if op[0] == "p":
            return "p %d %d" % self.predict(*op[1:])
        if op[0] == "o":
            self.key = dict(op[1])
            return "o 1"
        if op[0] == "t":
            n = self.covered(op[1])
            self.key = None                                             # gone either way
            return "t %d 0" % n
        self.key = None
        return "d 0"


def _arg(op):
    if op[0] == "p":
        return "p:%d:%d:%d" % op[1:]
    if op[0] == "d":
        return "d"
    return op[0] + ":" + ":".join(str(op[1][f]) for f in FIELDS)


def _run(exe, ops):
    p = subprocess.run([exe] + [_arg(o) for o in ops], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    err = p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return p.stdout.decode().splitlines()


def _model(ops):
    m = Model()
    return [m.run(o) for o in ops]


def _changed(field):
    k = dict(KEY)
    k[field] += 1
    return k


def _with(**kw):
    return dict(KEY, **kw)


PREDICT = [("p", f, c, n) for f, c, n in itertools.product(VALUES, VALUES, VALUES)]
SCRIPTS = {
    "predict": PREDICT,
    "take-after-offer": [("o", KEY), ("t", KEY)],
    "every-field-changed": [op for f in FIELDS if f != "count" for op in (("o", KEY), ("t", _changed(f)))],
    "prefix": [("o", KEY), ("t", _with(count=1500)), ("o", KEY), ("t", _with(count=1))],
    "larger": [("o", KEY), ("t", _with(count=2001))],
    "empty": [("o", KEY), ("t", _with(count=0))],
    "take-twice": [("o", KEY), ("t", KEY), ("t", KEY)],
    "take-without-offer": [("t", KEY)],
    "drop": [("o", KEY), ("d",), ("t", KEY), ("d",), ("d",)],
    "offer-replaces": [("o", KEY), ("o", _with(first=4000)), ("t", KEY), ("o", KEY), ("o", _with(first=4000)), ("t", _with(first=4000))],
    "a-miss-invalidates": [("o", KEY), ("t", _changed("reads_gen")), ("t", KEY)],
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_bookkeeping_is_the_restated_rule(driver, name):
    assert _run(driver, SCRIPTS[name]) == _model(SCRIPTS[name])


def test_the_named_cases():
    """the restatement itself, by hand"""
    assert Model.predict(0, 10, 1000) == (10, 10)
    assert Model.predict(0, 10, 11) == (1, 10)                          # clipped to the set
    assert Model.predict(0, 10, 10) == (0, 0) and Model.predict(1, 10, 11) == (0, 0)   # the end of the set
    assert Model.predict(9, 1, 11) == (1, 10) and Model.predict(10, 1, 11) == (0, 0)
    assert Model.predict(0, 0, 1000) == (0, 0) and Model.predict(1000, 10, 11) == (0, 0)
    assert _model(SCRIPTS["take-after-offer"]) == ["o 1", "t 2000 0"]
    assert _model(SCRIPTS["every-field-changed"]) == ["o 1", "t 0 0"] * 5
    assert _model(SCRIPTS["prefix"]) == ["o 1", "t 1500 0", "o 1", "t 1 0"]
    assert _model(SCRIPTS["larger"]) == ["o 1", "t 2000 0"] and _model(SCRIPTS["empty"]) == ["o 1", "t 0 0"]   # (the 2,001st read is the caller's to translate)
    assert _model(SCRIPTS["take-twice"]) == ["o 1", "t 2000 0", "t 0 0"]
    assert _model(SCRIPTS["drop"]) == ["o 1", "d 0", "t 0 0", "d 0", "d 0"]
    assert _model(SCRIPTS["a-miss-invalidates"]) == ["o 1", "t 0 0", "t 0 0"]


def test_bookkeeping_under_sanitizers(driver_san):
    for name in sorted(SCRIPTS):
        assert _run(driver_san, SCRIPTS[name]) == _model(SCRIPTS[name])
