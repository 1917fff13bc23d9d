"""The ordering and finishing kernels' algorithms, held to their statements on the CPU (no GPU): the formulation of mc_wave_std_sort
(csrc/k_finish.h; tests/emul/wave_sort_form.h restates it with the lanes flattened) against mc_std_sort, and mc_build_stacks - the
reference of the device test of the ordering kernels - against a plain restatement of CalRes' rule.  The inputs the device test
(test_gpu_order_units.py) sends to the GPU are the ones checked here, so they are known to reach the heap-sort fallback before they travel."""
import os
import re
import subprocess

import numpy as np
import pytest

import order_cases as oc


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-ffp-contract=off", "-I", oc.CSRC, "-o", exe, os.path.join(oc.EMUL, "wave_sort_form.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("wave_sort_form"), "wave_sort_form", ["-O2"])


def _adversary(exe, tmp):
    lens = oc.adversary_lengths()
    oc.write_sections(tmp / "adv.in", [np.array(lens, np.int32)])
    subprocess.check_call([exe, "adversary", str(tmp / "adv.in"), str(tmp / "adv.out")])
    return {n: np.frombuffer(b, "<f8") for n, b in zip(lens, oc.read_sections(tmp / "adv.out"))}


def test_wave_sort_formulation_equals_std_sort_on_200000_arrays(driver):
    out = subprocess.check_output([driver, "check", "200000"], text=True)
    print(out)
    got = dict(zip(out.split()[::2], map(int, out.split()[1::2])))
    assert got["arrays"] == 200000 and got["adversary_arrays"] == len(oc.WAVE_LENGTHS + oc.WAVE_LENGTHS_MORE[2])
    assert got["differ"] == 0 and got["adversary_differ"] == 0
    assert got["overflow"] == 0 and got["adversary_overflow"] == 0
    assert got["fallbacks"] > 0 and got["adversary_ge64_without_fallback"] == 0 and got["adversary_largest"] > 64


def test_wave_sort_inputs_of_the_device_test_reach_the_fallback(driver, tmp_path):
    sets = oc.wave_sort_sets(_adversary(driver, tmp_path))
    oc.write_sections(tmp_path / "w.in", oc.wave_input(sets))
    subprocess.check_call([driver, "waves", str(tmp_path / "w.in"), str(tmp_path / "w.out")])
    out = oc.read_sections(tmp_path / "w.out")
    differ = 0
    for q in range(len(sets)):
        want, got = np.frombuffer(out[3 * q], "<u4"), np.frombuffer(out[3 * q + 1], "<u4")
        assert len(want) == sum(n for n, _, _ in sets[q][1])
        differ += int((want != got).sum())
    print("formulation against mc_std_sort on the device test's arrays: %d differences" % differ)
    print("\n".join(oc.fallback_conditions(sets, [np.frombuffer(out[3 * q + 2], "<i4") for q in range(len(sets))])))
    assert differ == 0


def test_driver_under_sanitizers(tmp_path):
    """The formulation, the adversary and mc_build_stacks once under AddressSanitizer and UBSan, as a stand-alone program."""
    exe = _build(tmp_path, "wave_sort_form_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"])
    out = subprocess.check_output([exe, "check", "20000"], text=True)
    assert re.search(r"arrays 20000 differ 0 overflow 0 ", out) and " adversary_differ 0 " in out, out
    pool, slots, heads, low, _ = oc.order_case()
    oc.write_sections(tmp_path / "o.in", [pool, slots, heads, low])
    subprocess.check_call([exe, "stacks", str(tmp_path / "o.in"), str(tmp_path / "o.out")])


def test_build_stacks_against_calres_rule_restated(driver, tmp_path):
    pool, slots, heads, low, reads = oc.order_case()
    oc.write_sections(tmp_path / "o.in", [pool, slots, heads, low])
    subprocess.check_call([driver, "stacks", str(tmp_path / "o.in"), str(tmp_path / "o.out")])
    out = oc.read_sections(tmp_path / "o.out")
    vexp, vn = np.frombuffer(out[0], oc.HSP), np.frombuffer(out[1], "<u4")
    assert len(vexp) == len(slots) and len(vn) == len(reads)
    for r, (n, kind, _) in enumerate(reads):
        a = int(heads[r])
        seg = pool[slots[a:a + n]]
        keep, sizes = oc.restated_stacks(seg)
        assert vn[r] == len(keep), (r, n, kind)
        got = vexp[a:a + len(keep)]
        for f in oc.COMPARED_FIELDS:
            assert np.array_equal(got[f], seg[f][keep]), (r, n, kind, f)
        assert np.array_equal(got["read"], sizes), (r, n, kind)
    print("mc_build_stacks == CalRes' rule restated on %d reads, %d HSPs, %d stacked" % (len(reads), len(slots), int(vn.sum())))
