"""tools/ahead_trace.py on kernel traces written by hand: the tail of the lookahead's translation - what is left of it when the seed
kernel has ended - and where k_eval_seeds starts against its end.  The ranges of tests/test_ahead_trace_host.py (queue 1 the range's
stream, queue 2 the lookaheads, queue 4 the rows' copy), with the lookahead's end and the start of k_eval_seeds set per case.  No GPU."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MS = 1000000
SEED = 5.0                                                              # the seed kernel's duration


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("ahead_trace", os.path.join(HERE, "..", "tools", "ahead_trace.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _range(t, tr_end, ev_start):
    """the dispatches of one range whose seed kernel starts at t (ms): the lookahead ends tr_end and k_eval_seeds starts ev_start behind
    the seed kernel's START; k_eval_seeds lasts 2 ms and everything behind it follows it"""
    e = t + ev_start + 2
    return [("__amd_rocclr_fillBufferAligned", 1, t - 0.05, t - 0.01),
            ("k_enumerate_q<8>", 1, t, t + SEED), ("k_eval_seeds<true>", 1, t + ev_start, e), ("k_gap_emit", 1, e + 2, e + 3),
            ("k_order_light", 1, e + 3, e + 5), ("k_finish_heavy<6144, 13, -1>", 3, e + 5, e + 6), ("k_emit_rows", 1, e + 6, e + 7),
            ("__amd_rocclr_copyBuffer", 4, e + 7, e + 12), ("__amd_rocclr_copyBuffer", 1, e + 7, e + 8.5),
            ("k_translate_seg<true, true>", 2, t + 0.05, t + tr_end)], e + 8.7


def _steps(tool, path, tr_end, ev_start):
    t, rows = 10.0, []
    for _ in range(3):
        r, t = _range(t, tr_end, ev_start)
        rows += r
    rows.append(("k_enumerate_q<8>", 1, t, t + SEED))
    with open(path, "w") as f:
        f.write('"Kind","Agent_Id","Queue_Id","Stream_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n')
        for name, q, a, b in rows:
            f.write('"KERNEL_DISPATCH",1,%d,%d,"void %s(int)",%d,%d\n' % (q, q, name, round(a * MS), round(b * MS)))
    st = tool.steps(tool.load(path))
    assert len(st) == 2                                                 # (the first range of a trace is not reported)
    return st


def test_eval_starts_behind_a_tail_of_0_9_ms(tool, tmp_path):
    """the translation ends 0.9 ms after the seed kernel and k_eval_seeds starts 0.02 ms behind it: the tail is 0.9 ms, no part of the
    translation lies inside k_eval_seeds, and eval_ms - seed kernel's end to the end of k_eval_seeds - holds the tail"""
    for r in _steps(tool, str(tmp_path / "t.csv"), SEED + 0.9, SEED + 0.92):
        assert r["translate_tail_alone_ms"] == pytest.approx(0.9, abs=1e-6)
        assert r["eval_start_after_translate_end_ms"] == pytest.approx(0.02, abs=1e-6)
        assert r["eval_ms"] == pytest.approx(2.92, abs=1e-6)
        assert r["translate_ms"] == pytest.approx(SEED + 0.85, abs=1e-6)
        assert r["translate_share_in_seed"] == pytest.approx((SEED - 0.05) / (SEED + 0.85))
        assert r["translate_share_in_eval"] == pytest.approx(0.9 / (SEED + 0.85))   # (the stage, from the seed kernel's end: the tail lies in it)
        assert r["translate_share_in_gapped"] == 0.0


def test_a_translation_that_ends_inside_the_seed_kernel(tool, tmp_path):
    """no tail, and k_eval_seeds starts 0 behind the seed kernel's end"""
    for r in _steps(tool, str(tmp_path / "t.csv"), SEED - 0.4, SEED):
        assert r["translate_tail_alone_ms"] == 0.0
        assert r["eval_start_after_translate_end_ms"] == 0.0
        assert r["eval_ms"] == pytest.approx(2.0, abs=1e-6)
        assert r["translate_share_in_seed"] == pytest.approx(1.0) and r["translate_share_in_eval"] == 0.0


def test_the_parent_s_order_eval_beside_the_tail(tool, tmp_path):
    """k_eval_seeds starts at the seed kernel's end, 1.3 ms before the translation ends"""
    for r in _steps(tool, str(tmp_path / "t.csv"), SEED + 1.3, SEED):
        assert r["translate_tail_alone_ms"] == pytest.approx(1.3, abs=1e-6)
        assert r["eval_start_after_translate_end_ms"] == pytest.approx(-1.3, abs=1e-6)
        assert r["eval_ms"] == pytest.approx(2.0, abs=1e-6)
        assert r["translate_share_in_eval"] == pytest.approx(1.3 / (SEED + 1.25))
