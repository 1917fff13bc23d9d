#!/usr/bin/env python3
"""Are two builds the same instructions, kernel by kernel?  (development aid, CPU only: DESIGN.md 13.3, 13.13)
    tools/kernel_diff.py OLD NEW [name-filter]
OLD, NEW: a device assembly file each (hipcc -S --cuda-device-only), or the root of a tree each - then csrc/mc_hip.hip is compiled with
the flags of tools/kernel_report.sh.  Per kernel symbol: the instructions on either side and `same` or `differs`; labels are renumbered
in their order of appearance, comments and directives dropped.  Exit status 1 when a symbol differs or is on one side only."""
import os, re, subprocess, sys, tempfile


def assembly(path):
    if os.path.isfile(path):
        return open(path).read()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(path, "microbecensus_amd", "csrc")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", src,
                               "-o", os.path.join(tmp, "k.s"), os.path.join(src, "mc_hip.hip")])
        return open(os.path.join(tmp, "k.s")).read()


def kernels(text):
    """{symbol: instructions} of the kernels (the symbols with a .amdhsa_kernel block)"""
    names, out = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)), {}
    for f in re.split(r"\n(?=\w+:)", text):
        name = f.split(":")[0]
        if name not in names:
            continue
        body = f[len(name) + 1:].split(".Lfunc_end")[0]
        lines = [re.sub(r"\s+", " ", l.split(";")[0]).strip() for l in body.split("\n")]
        lines = [l for l in lines if l and (l.endswith(":") or not l.startswith("."))]
        labels = {}                                                 # in their order of appearance, defined or referred to
        for l in lines:
            for lab in re.findall(r"\.LBB\w+", l):
                labels.setdefault(lab, "L%d" % len(labels))
        out[name] = [re.sub(r"\.LBB\w+", lambda m: labels[m.group(0)], l) for l in lines]
    return out


def main():
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    want = sys.argv[3] if len(sys.argv) == 4 else ""
    old, new, bad = kernels(assembly(sys.argv[1])), kernels(assembly(sys.argv[2])), 0
    for name in sorted(set(old) | set(new)):
        if want not in name:
            continue
        a, b = old.get(name), new.get(name)
        count = lambda k: "-" if k is None else str(sum(1 for l in k if not l.endswith(":")))
        verdict = "same" if a == b else "differs" if a is not None and b is not None else "missing"
        bad += verdict != "same"
        print("%-72s %6s %6s  %s" % (name[:72], count(a), count(b), verdict))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
