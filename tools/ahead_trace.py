#!/usr/bin/env python3
"""Where the lookahead's translation runs (development aid; the traces come from the GPU box): tools/ahead_trace.py PARENT.csv THIS.csv OUT_PREFIX
Both inputs are rocprofv3 --kernel-trace CSVs of `bench.py --steps 4 --warmup 2 --batch 1000000` (a run of its own: no counters, no other
tracing), one of the parent's build and one of this one.  Writes OUT_PREFIX_trace.json and OUT_PREFIX_kernel_stats.csv, the mean
duration of every kernel of the library in both builds.  The json holds, from the trace's timestamps:

per step of either build (a step: from the start of one range's seed kernel, k_enumerate_q, to the start of the next range's) the
duration of every foreground stage - the seed kernel, k_eval_seeds, the gapped stage (end of k_eval_seeds to the end of k_gap_emit),
stage C + D (end of k_gap_emit to the end of k_emit_rows) - and the whole step; medians over the steps, and this build's stretch of
each stage against the parent's;

per step of this build, where k_translate_seg of the NEXT range runs (the lookahead of a step: the translation that starts between the
end of the range before, its k_emit_rows, and the end of this one, and not in front of the seed kernel on its queue - that is a
range's own A0): its start behind the step's seed kernel's start, its duration,
the share of its interval that lies inside each foreground stage, its tail (translate_tail_alone_ms: from the end of the seed kernel
to the end of the translation, 0 where it ended inside the seed kernel) and the start of k_eval_seeds behind the later of the two ends
(eval_start_after_translate_end_ms: negative where k_eval_seeds started beside the translation; eval_ms, end of the seed kernel to the
end of k_eval_seeds, holds the tail in a build whose k_eval_seeds waits for it - DESIGN.md 5.12), its end against the end of k_emit_rows, and how long the next seed
kernel waited for it (translation's end behind the end of this range's last dispatch on the seed kernel's own queue, its last copy
to the host; 0 where it ended earlier; an upper bound, the host's pause between two ranges lies in it);

the hardware queue of every kernel's dispatches (Queue_Id), so that one sees which streams share a queue.

(Under the profiler the copies to the host run as kernels and take milliseconds: the time between k_emit_rows and the next range's
first kernel is the profiler's, not the bench's.  mc_ahead_kernel_ms() gives the background kernel's interval without a profiler.)"""
import csv
import json
import statistics
import sys

STAGES = ("seed_ms", "eval_ms", "gapped_ms", "c_d_ms")


def load(path):
    ks = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        ks.append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "")))
    ks.sort(key=lambda k: k[1])
    return ks


def first_after(ks, name, t):
    for k in ks:
        if k[0].startswith(name) and k[1] >= t:
            return k
    return None


def overlap(a0, a1, b0, b1):
    return max(0, min(a1, b1) - max(a0, b0))


def steps(ks):
    """one record per range i that has a range i + 1 behind it (ms)"""
    out = []
    seeds = [k for k in ks if k[0].startswith("k_enumerate_q")]
    prev_rows_end = None
    for s, s_next in zip(seeds, seeds[1:]):
        ev = first_after(ks, "k_eval_seeds", s[2])
        emit = first_after(ks, "k_gap_emit", s[2])
        rows = first_after(ks, "k_emit_rows", s[2])
        if ev is None or emit is None or rows is None or rows[2] > s_next[1]:
            prev_rows_end = None
            continue
        since, prev_rows_end = prev_rows_end, rows[2]
        if since is None:                                              # (the first range of the trace: where its range_begin lies is not known)
            continue
        # the stages of the range, end to end
        marks = {"seed_ms": (s[1], s[2]), "eval_ms": (s[2], ev[2]), "gapped_ms": (ev[2], emit[2]), "c_d_ms": (emit[2], rows[2])}
        rec = {k: (b - a) / 1e6 for k, (a, b) in marks.items()}
        rec["step_ms"] = (s_next[1] - s[1]) / 1e6
        rec["gapped_end_to_next_seed_kernel_ms"] = (s_next[1] - emit[2]) / 1e6
        # the lookahead of the step: the translation issued between the end of the range before (its k_emit_rows) and the end of this
        # one, on another queue than the seed kernel's - a range's own A0 runs in front of its seed kernel on the same queue
        tr = [k for k in ks if k[0].startswith("k_translate_seg") and since <= k[1] < rows[2] and (k[3] != s[3] or k[1] > s[1])]
        if tr:
            t0, t1 = tr[0][1], max(k[2] for k in tr)
            span = max(1, sum(k[2] - k[1] for k in tr))
            rec["translate_start_after_seed_start_ms"] = (t0 - s[1]) / 1e6
            rec["translate_start_after_last_gapped_kernel_ms"] = (t0 - emit[2]) / 1e6
            rec["translate_ms"] = span / 1e6
            rec["translate_end_after_emit_rows_ms"] = (t1 - rows[2]) / 1e6
            for name, (a, b) in marks.items():
                rec["translate_share_in_" + name[:-3]] = sum(overlap(k[1], k[2], a, b) for k in tr) / span
            # the translation's tail: what is left of it when the seed kernel has ended (0: it ended inside the seed kernel), and where
            # k_eval_seeds starts against its end - negative while the two run beside each other, as they do in the tree; at least 0 (the
            # dispatch's delay) in a build whose k_eval_seeds waits for the lookahead's end (measured and not kept)
            rec["translate_tail_alone_ms"] = max(0.0, (t1 - s[2]) / 1e6)
            rec["eval_start_after_translate_end_ms"] = (ev[1] - max(t1, s[2])) / 1e6 if t1 <= ev[1] else (ev[1] - t1) / 1e6
            # What the next range has to follow apart from the lookahead: the dispatches of THIS range on the seed kernel's own queue,
            # the range's stream - its kernels (the side streams join it) and its copies to the host, the last of which ends the
            # range.  Not the lookaheads' queue, not the rows' copy, which goes on beside the next range, and not what the next
            # range puts on the queue in front of its seed kernel - its memsets, a translation of its own - because its stream waits
            # for the lookahead in front of them.  Where the translation ends behind the last of this range, the difference is the
            # wait - with the host's pause between the two ranges in it, which a trace cannot tell from waiting: an upper bound.
            last_fg = max(k[2] for k in ks if s[1] <= k[1] < s_next[1] and k[3] == s[3] and "fillBuffer" not in k[0] and not k[0].startswith("k_translate_seg"))
            rec["next_seed_kernel_waited_for_translation_ms"] = max(0.0, (t1 - last_fg) / 1e6)
        out.append(rec)
    return out


def median_of(recs):
    keys = [k for k in recs[0] if all(k in r for r in recs)] if recs else []
    return {k: round(statistics.median(r[k] for r in recs), 3) for k in keys}


def kernel_means(ks):
    acc = {}
    for name, a, b, q in ks:
        if name.startswith("k_"):
            acc.setdefault(name, []).append((b - a) / 1e6)
    return {k: (len(v), sum(v) / len(v)) for k, v in acc.items()}


def queues(ks):
    """queue id -> the kernels dispatched on it (with their counts)"""
    acc = {}
    for name, a, b, q in ks:
        acc.setdefault(str(q), {}).setdefault(name, 0)
        acc[str(q)][name] += 1
    return acc


def main():
    parent, this, prefix = load(sys.argv[1]), load(sys.argv[2]), sys.argv[3]
    sp, st = steps(parent), steps(this)
    ahead = [r for r in st if "translate_ms" in r]                                   # (the steps in which a lookahead ran)
    doc = {"what": "rocprofv3 --kernel-trace of bench.py --steps 4 --warmup 2 --batch 1000000 (1 M reads of 150 bp per step), parent build and this build; medians over the steps, ms",
           "parent": dict(median_of(sp), steps=len(sp)), "this": dict(median_of(ahead), steps=len(ahead), steps_without_lookahead=len(st) - len(ahead)),
           "this_per_step": [{k: round(v, 3) for k, v in r.items()} for r in ahead],
           "queues_parent": queues(parent), "queues_this": queues(this)}
    if sp and ahead:
        p, t = doc["parent"], doc["this"]
        doc["stretch_ms"] = {k: round(t[k] - p[k], 3) for k in STAGES + ("step_ms",)}
        doc["gapped_end_to_next_seed_kernel_saved_ms"] = round(p["gapped_end_to_next_seed_kernel_ms"] - t["gapped_end_to_next_seed_kernel_ms"], 3)
    with open(prefix + "_trace.json", "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    mp, mt = kernel_means(parent), kernel_means(this)
    with open(prefix + "_kernel_stats.csv", "w") as f:
        f.write("kernel,parent_calls,parent_mean_ms,this_calls,this_mean_ms\n")
        for k in sorted(set(mp) | set(mt), key=lambda k: -mt.get(k, (0, 0))[1]):
            f.write("\"%s\",%d,%.4f,%d,%.4f\n" % (k, mp.get(k, (0, 0))[0], mp.get(k, (0, 0))[1], mt.get(k, (0, 0))[0], mt.get(k, (0, 0))[1]))
    print(json.dumps({k: v for k, v in doc.items() if not k.startswith("queues") and k != "this_per_step"}, indent=1))


if __name__ == "__main__":
    main()
