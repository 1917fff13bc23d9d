#!/usr/bin/env python3
"""Where the lookahead's translation runs (development aid; the traces come from the GPU box): tools/ahead_trace.py PARENT.csv THIS.csv OUT_PREFIX
Both inputs are rocprofv3 --kernel-trace CSVs of `bench.py --steps 4 --warmup 2 --batch 1000000` (a run of its own: no counters, no other
tracing), one of the parent's build and one of this one.  Writes OUT_PREFIX_trace.json - per step, from the trace's timestamps: where
k_translate_seg of range i + 1 starts against the end of the last gapped kernel and of k_emit_rows of range i, the span of stage C + D of
range i beside the parent's, and how long the seed kernel's stream had to wait for the translation - and OUT_PREFIX_kernel_stats.csv, the
mean duration of every kernel of the library in both builds.  (Under the profiler the copies to the host run as kernels and take
milliseconds: the time between k_emit_rows and the next range's first kernel is the profiler's, not the bench's.)"""
import csv
import json
import statistics
import sys


def load(path):
    ks = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        ks.append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    ks.sort(key=lambda k: k[1])
    return ks


def first_after(ks, name, t):
    for k in ks:
        if k[0].startswith(name) and k[1] >= t:
            return k
    return None


def steps(ks):
    """one record per range i that has a range i + 1 behind it (ms)"""
    out = []
    emits = [k for k in ks if k[0] == "k_gap_emit"]
    for e, e_next in zip(emits, emits[1:]):
        rows = first_after(ks, "k_emit_rows", e[2])
        seed = first_after(ks, "k_enumerate_q", e[2])
        tr = [k for k in ks if k[0].startswith("k_translate_seg") and e[2] <= k[1] < e_next[1]]
        if rows is None or seed is None or not tr or rows[1] > e_next[1]:
            continue
        t = tr[0]
        out.append({"translate_start_after_last_gapped_kernel_ms": (t[1] - e[2]) / 1e6, "translate_start_after_emit_rows_ms": (t[1] - rows[2]) / 1e6,
                    "translate_ms": sum(k[2] - k[1] for k in tr) / 1e6, "translate_end_after_emit_rows_ms": (tr[-1][2] - rows[2]) / 1e6,
                    "stage_c_d_span_ms": (rows[2] - e[2]) / 1e6, "seed_kernel_start_after_translate_end_ms": (seed[1] - tr[-1][2]) / 1e6,
                    "gapped_end_to_next_seed_kernel_ms": (seed[1] - e[2]) / 1e6})
    return out


def median_of(recs):
    return {k: round(statistics.median(r[k] for r in recs), 3) for k in recs[0]} if recs else {}


def kernel_means(ks):
    acc = {}
    for name, a, b in ks:
        if name.startswith("k_"):
            acc.setdefault(name, []).append((b - a) / 1e6)
    return {k: (len(v), sum(v) / len(v)) for k, v in acc.items()}


def main():
    parent, this, prefix = load(sys.argv[1]), load(sys.argv[2]), sys.argv[3]
    sp, st = steps(parent), steps(this)
    ahead = [r for r in st if r["translate_start_after_emit_rows_ms"] < 0]          # (the steps whose next range was translated ahead)
    doc = {"what": "rocprofv3 --kernel-trace of bench.py --steps 4 --warmup 2 --batch 1000000 (1 M reads of 150 bp per step), parent build and this build; medians over the steps, ms",
           "parent": dict(median_of(sp), steps=len(sp)), "this": dict(median_of(ahead), steps=len(ahead), steps_without_lookahead=len(st) - len(ahead))}
    if sp and ahead:
        p, t = doc["parent"], doc["this"]
        doc["stage_c_d_stretch_ms"] = round(t["stage_c_d_span_ms"] - p["stage_c_d_span_ms"], 3)
        doc["translate_stretch_ms"] = round(t["translate_ms"] - p["translate_ms"], 3)
        doc["seed_kernel_waited_for_translation_ms"] = round(max(0.0, t["translate_end_after_emit_rows_ms"]), 3)
        doc["gapped_end_to_next_seed_kernel_saved_ms"] = round(p["gapped_end_to_next_seed_kernel_ms"] - t["gapped_end_to_next_seed_kernel_ms"], 3)
    with open(prefix + "_trace.json", "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    mp, mt = kernel_means(parent), kernel_means(this)
    with open(prefix + "_kernel_stats.csv", "w") as f:
        f.write("kernel,parent_calls,parent_mean_ms,this_calls,this_mean_ms\n")
        for k in sorted(set(mp) | set(mt), key=lambda k: -mt.get(k, (0, 0))[1]):
            f.write("\"%s\",%d,%.4f,%d,%.4f\n" % (k, mp.get(k, (0, 0))[0], mp.get(k, (0, 0))[1], mt.get(k, (0, 0))[0], mt.get(k, (0, 0))[1]))
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
