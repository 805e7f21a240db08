#!/usr/bin/env python3
"""lane_overlap.py - what a rocprofv3 --kernel-trace of a multi-lane bench.py run says about the lanes:

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps 10 --warmup 2
  python tools/lane_overlap.py DIR [--warmup 2]

Prints, for the process with the most dispatches, (1) which HIP streams dispatched on which hardware queue during the timed steps - two lane streams
on one queue serialise behind each other's barrier packets ("Hardware queues") - and (2) the share of the timed window with
0 / 1 / 2 / 3 / 4+ pipeline kernels in flight, with the window's length per step.  The timed window starts where the warm-up steps' last k_stereo
ends (bench.py fences there) and ends with the last pipeline kernel."""
import argparse
import csv
import glob
import os
import sys
from collections import Counter, defaultdict

PIPELINE = ("k_pyramid", "k_detect", "k_compact", "k_blur", "k_describe", "k_stereo", "k_median")


def short(name):
    for p in PIPELINE:
        if p in name:
            return "k_blur_compact" if "k_blur_compact" in name else p
    return None


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = short(r.get("Kernel_Name", ""))
            if k is None:
                continue
            rows.append({"k": k, "queue": r.get("Queue_Id", "?"), "stream": r.get("Stream_Id"), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--warmup", type=int, default=2, help="warm-up steps of the traced run")
    ap.add_argument("--lanes", type=int, default=4)
    a = ap.parse_args()
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % a.dir)
    rows = max((load(f) for f in files), key=len)
    stereo_ends = sorted(r["t1"] for r in rows if r["k"] == "k_stereo")
    n_warm = a.warmup * a.lanes
    if len(stereo_ends) <= n_warm:
        sys.exit("fewer k_stereo dispatches (%d) than the warm-up has" % len(stereo_ends))
    w0 = stereo_ends[n_warm - 1] if n_warm else min(r["t0"] for r in rows)
    win = [r for r in rows if r["t0"] >= w0]
    w1 = max(r["t1"] for r in win)
    w0 = min(r["t0"] for r in win)
    steps = (len(stereo_ends) - n_warm) / float(a.lanes)
    print("dispatches in the timed window: %d, steps: %.1f, window %.3f ms = %.4f ms per step" % (len(win), steps, (w1 - w0) * 1e-6, (w1 - w0) * 1e-6 / steps))
    print("sum of kernel durations per step: %.4f ms" % (sum(r["t1"] - r["t0"] for r in win) * 1e-6 / steps))
    # (1) stream -> queue
    table = defaultdict(Counter)
    for r in win:
        table[r["stream"] if r["stream"] not in (None, "") else "(no Stream_Id column)"][r["queue"]] += 1
    print("stream -> hardware queue (dispatches):")
    per_queue = defaultdict(set)
    for s in sorted(table, key=str):
        print("  stream %-6s %s" % (s, ", ".join("queue %s: %d" % (q, n) for q, n in sorted(table[s].items()))))
        for q in table[s]:
            per_queue[q].add(s)
    shared = {q: sorted(v, key=str) for q, v in per_queue.items() if len(v) > 1}
    print("queues used: %d; queues with more than one stream: %s" % (len(per_queue), shared if shared else "none"))
    # (2) kernels in flight
    ev = []
    for r in win:
        ev.append((r["t0"], 1))
        ev.append((r["t1"], -1))
    ev.sort(key=lambda e: (e[0], e[1]))
    share, depth, last = Counter(), 0, w0
    for t, d in ev:
        share[min(depth, 4)] += t - last
        last = t
        depth += d
    total = float(w1 - w0)
    print("kernels in flight, share of the window: " + ", ".join("%s: %.1f %%" % ("4+" if c == 4 else c, 100.0 * share[c] / total) for c in range(5)))


if __name__ == "__main__":
    main()
