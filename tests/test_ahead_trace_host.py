"""tools/ahead_trace.py on kernel traces written by hand: the figures it reports per step are the ones the timestamps hold - above all
how long the next seed kernel waited for the lookahead's translation, which must not be 0 by construction.  Three ranges on queue 1
(seed kernel, k_eval_seeds, k_gap_emit, k_emit_rows, the copy of the best hits; the next range's memsets in front of its seed
kernel), the lookaheads on queue 2, the rows' copy on queue 4.  No GPU."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MS = 1000000


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("ahead_trace", os.path.join(HERE, "..", "tools", "ahead_trace.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _range(t, wait_ms):
    """the dispatches of one range whose seed kernel starts at t (ms), and the lookahead issued at its begin: (name, queue, start, end)
    in ms; the lookahead lasts until wait_ms behind the range's last copy (negative: it ends earlier).  Returns the rows and the time
    the next range's seed kernel starts."""
    end = t + 15.5                                                      # the end of the range's last copy
    tr_end = end + wait_ms
    nxt = max(end, tr_end) + 0.1                                        # the next range's memsets follow whichever ends last
    rows = [("__amd_rocclr_fillBufferAligned", 1, t - 0.05, t - 0.01),
            ("k_enumerate_q<8>", 1, t, t + 5), ("k_eval_seeds<true>", 1, t + 5, t + 7), ("k_gap_emit", 1, t + 9, t + 10),
            ("k_order_light", 1, t + 10, t + 12), ("k_finish_heavy<6144, 13, -1>", 3, t + 12, t + 13), ("k_emit_rows", 1, t + 13, t + 14),
            ("__amd_rocclr_copyBuffer", 4, t + 14, t + 19),           # the rows leave beside the next range: nobody waits for them
            ("__amd_rocclr_copyBuffer", 1, t + 14, end),
            ("k_translate_seg<true>", 2, t + 0.05, tr_end)]
    return rows, nxt + 0.05


def _trace(path, waits):
    t, rows = 10.0, []
    for w in waits + [-5.0]:
        r, t = _range(t, w)
        rows += r
    rows.append(("k_enumerate_q<8>", 1, t, t + 5))
    with open(path, "w") as f:
        f.write('"Kind","Agent_Id","Queue_Id","Stream_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n')
        for name, q, a, b in rows:
            f.write('"KERNEL_DISPATCH",1,%d,%d,"void %s(int)",%d,%d\n' % (q, q, name, round(a * MS), round(b * MS)))
    return path


@pytest.mark.parametrize("wait", [0.0, 0.9, 25.0])
def test_the_wait_for_the_translation_is_the_one_in_the_trace(tool, tmp_path, wait):
    """four ranges and the seed kernel of a fifth.  The first range of a trace is not reported (where its begin lies is unknown); the
    three behind it are: one whose lookahead ends 3 ms before the range's last copy - no wait - one whose lookahead ends `wait` ms
    behind it, and one whose lookahead ends 5 ms before it"""
    ks = tool.load(_trace(str(tmp_path / "t.csv"), [-1.0, -3.0, wait]))
    st = tool.steps(ks)
    assert len(st) == 3
    assert st[0]["next_seed_kernel_waited_for_translation_ms"] == 0.0 and st[2]["next_seed_kernel_waited_for_translation_ms"] == 0.0
    assert st[1]["next_seed_kernel_waited_for_translation_ms"] == pytest.approx(wait, abs=1e-6)
    for r in st:
        assert r["seed_ms"] == pytest.approx(5.0) and r["eval_ms"] == pytest.approx(2.0) and r["gapped_ms"] == pytest.approx(3.0) and r["c_d_ms"] == pytest.approx(4.0)
        assert r["translate_start_after_seed_start_ms"] == pytest.approx(0.05)
    assert st[1]["translate_ms"] == pytest.approx(15.45 + wait) and st[1]["translate_end_after_emit_rows_ms"] == pytest.approx(1.5 + wait)
    assert st[1]["step_ms"] == pytest.approx(15.5 + wait + 0.15)
    assert st[0]["translate_share_in_seed"] == pytest.approx(4.95 / 12.45)


def test_queues_are_reported(tool, tmp_path):
    q = tool.queues(tool.load(_trace(str(tmp_path / "t.csv"), [-1.0, -1.0])))
    assert set(q) == {"1", "2", "3", "4"} and set(q["2"]) == {"k_translate_seg<true>"} and set(q["4"]) == {"__amd_rocclr_copyBuffer"}
