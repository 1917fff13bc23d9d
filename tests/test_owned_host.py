"""Who owns what the library takes from the HIP runtime, on the CPU.  csrc/mc_owned.h over a fake runtime (g++ build,
tests/emul/owned.cpp), plain and under ASan / UBSan with leak detection: every owner type made, replaced, moved, reset and failed,
the live counts back at zero after every case.  And the rule itself, read off the source text: the eight calls that make and destroy
device buffers, pinned buffers, streams and events occur in csrc/ only inside mc_owned.h.  No GPU."""
import glob
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "microbecensus_amd", "csrc")
OWNERS = ["device buffer", "pinned buffer", "stream", "event", "event without timing"]
OWNER_CASES = ["create, destroy", "a second creation frees the first one first", "move-construct", "move-assign onto a full owner", "reset twice",
               "a failed creation leaves the owner empty and the error named"]
CASES = ["%s: %s" % (o, c) for o in OWNERS for c in OWNER_CASES] + [
    "device buffer: usable as the pointer it holds", "McDevBuf: five buffers, the third fails", "McDevBuf: five buffers", "McEvents: four events, the third fails",
    "every kind at once"]


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "owned")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(HERE, "emul", "owned.cpp")])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    err = p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return [line[3:] for line in p.stdout.decode().splitlines() if line.startswith("ok ")]


def test_owners(tmp_path_factory):
    assert _run(_build(tmp_path_factory, "owned", ["-O2"])) == CASES


def test_owners_under_sanitizers(tmp_path_factory):
    """no leak, no double free, no use after free in any case (the fake keeps every resource in malloc'd memory)"""
    assert _run(_build(tmp_path_factory, "owned_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])) == CASES


CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipStreamCreate\w*|hipStreamDestroy|hipEventCreate\w*|hipEventDestroy)\b")


def test_no_resource_call_outside_the_owners():
    files = sorted(f for pat in ("*.hip", "*.h") for f in glob.glob(os.path.join(CSRC, pat)) if os.path.basename(f) != "mc_owned.h")
    assert len(files) > 20 and any(f.endswith("mc_hip.hip") for f in files)
    found, warm = [], 0
    for f in files:
        with open(f) as fh:
            for no, line in enumerate(fh, 1):
                for m in CALLS.finditer(line):
                    if line[m.start():].startswith("hipFree(nullptr)"):      # open_impl: initialises the runtime, frees nothing
                        warm += 1
                    else:
                        found.append("%s:%d: %s" % (os.path.basename(f), no, m.group(0)))
    assert found == [] and warm == 1
    with open(os.path.join(CSRC, "mc_owned.h")) as fh:                       # (and the pattern does find them where they are)
        assert {m.group(1) for m in CALLS.finditer(fh.read())} == {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipStreamCreate", "hipStreamDestroy",
                                                                   "hipEventCreate", "hipEventCreateWithFlags", "hipEventDestroy"}
