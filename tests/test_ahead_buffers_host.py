"""The buffer bookkeeping of the lookahead on the CPU: csrc/mc_ahead.h (g++ build with -fsanitize=address,undefined,
tests/emul/ahead_buffers.cpp) against a plain Python statement of its rule.  A context has two frame buffers; the running range's is
the current one, a lookahead writes the other, a take that covers any read makes the lookahead's buffer the current one - a partial
cover too: the rest is translated on top, into the same buffer - and a take that covers nothing, or a drop, changes nothing.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("reads_gen", "first", "count", "read_len", "FP", "tables_gen")
KEY = dict(reads_gen=7, first=2000, count=2000, read_len=150, FP=52, tables_gen=3)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ahead_buffers") / "ahead_buffers")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(HERE, "emul", "ahead_buffers.cpp")])
    return exe


class Model:
    """the rule, restated; every operation answers with the line the driver prints"""

    def __init__(self):
        self.key, self.cur, self.buf = None, 0, 1

    def run(self, op):
        if op[0] == "g":
            return "g %d" % (1 - self.cur)
        if op[0] == "o":
            self.key, self.buf = dict(op[1]), 1 - self.cur
            return "o 1 %d %d" % (self.buf, self.cur)
        if op[0] == "t":
            k, want = self.key, op[1]
            n = 0
            if k is not None and want["count"] > 0 and k["count"] > 0 and all(k[f] == want[f] for f in FIELDS if f != "count"):
                n = min(k["count"], want["count"])
            self.key = None
            if n:
                self.cur = self.buf
            return "t %d 0 %d" % (n, self.cur)
        self.key = None
        return "d 0 %d" % self.cur


def _arg(op):
    return op[0] if op[0] in "dg" else op[0] + ":" + ":".join(str(op[1][f]) for f in FIELDS)


def _run(exe, ops):
    p = subprocess.run([exe] + [_arg(o) for o in ops], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    err = p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return p.stdout.decode().splitlines()


def _model(ops):
    m = Model()
    return [m.run(o) for o in ops]


def _with(**kw):
    return dict(KEY, **kw)


NEXT = _with(first=4000)
SCRIPTS = {
    "offer-take": [("g",), ("o", KEY), ("g",), ("t", KEY), ("g",)],
    "partial-take": [("o", KEY), ("t", _with(count=1500)), ("g",)],
    "longer-take": [("o", KEY), ("t", _with(count=2001)), ("g",)],
    "drop": [("o", KEY), ("d",), ("g",), ("t", KEY), ("g",)],
    "miss": [("o", KEY), ("t", _with(first=0)), ("g",), ("t", KEY)],
    "empty-take": [("o", KEY), ("t", _with(count=0)), ("g",)],
    "two-takes-in-a-row": [("o", KEY), ("t", KEY), ("t", KEY), ("g",)],
    "a-stream": [("o", KEY), ("t", KEY), ("o", NEXT), ("t", NEXT), ("o", KEY), ("t", KEY), ("g",)],
    "never-taken-then-taken": [("o", KEY), ("t", _with(first=0)), ("o", KEY), ("t", KEY), ("o", NEXT), ("d",), ("o", NEXT), ("t", NEXT)],
    "offer-replaces": [("o", KEY), ("o", NEXT), ("t", KEY), ("o", KEY), ("o", NEXT), ("t", NEXT)],
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_buffers_follow_the_restated_rule(driver, name):
    assert _run(driver, SCRIPTS[name]) == _model(SCRIPTS[name])


def test_the_named_cases():
    """the restatement itself, by hand: which buffer is current after each operation"""
    assert _model(SCRIPTS["offer-take"]) == ["g 1", "o 1 1 0", "g 1", "t 2000 0 1", "g 0"]
    assert _model(SCRIPTS["partial-take"]) == ["o 1 1 0", "t 1500 0 1", "g 0"]
    assert _model(SCRIPTS["longer-take"]) == ["o 1 1 0", "t 2000 0 1", "g 0"]
    assert _model(SCRIPTS["drop"]) == ["o 1 1 0", "d 0 0", "g 1", "t 0 0 0", "g 1"]
    assert _model(SCRIPTS["miss"]) == ["o 1 1 0", "t 0 0 0", "g 1", "t 0 0 0"]
    assert _model(SCRIPTS["empty-take"]) == ["o 1 1 0", "t 0 0 0", "g 1"]
    assert _model(SCRIPTS["two-takes-in-a-row"]) == ["o 1 1 0", "t 2000 0 1", "t 0 0 1", "g 0"]
    assert _model(SCRIPTS["a-stream"]) == ["o 1 1 0", "t 2000 0 1", "o 1 0 1", "t 2000 0 0", "o 1 1 0", "t 2000 0 1", "g 0"]
