#!/usr/bin/env python
"""Main-stream idle time of the pipelined encoder step, from a rocprofv3 kernel_trace.csv of `bench.py`.

    python tools/step_gap_table.py <kernel_trace.csv> [steps-to-average]

A step is cut at the starts of two consecutive launches of its first kernel: k_input_fwd where the step has one, else the
self-loop GEMM that forms H0 on load (the prologue instantiation, k_gemm_w8<.., true>); the main stream is that kernel's
queue.  For the
last complete steps (default 8) prints: the timeline of the last one, and a table -- mean over the steps -- of the gap
in front of every main-stream kernel (end of the previous main-stream kernel to its start), the sum of those gaps, and
the time no kernel runs on any queue."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 8


def short(n):
    return (n.replace("(anonymous namespace)::", "").replace("void ", "").replace("rgcn::", "").split("(")[0][:60])


ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", r.get("Stream_Id", "?")),
             short(r["Kernel_Name"])) for r in rows)
starts = [i for i, k in enumerate(ks) if k[3].startswith("k_input_fwd")]
if not starts:
    starts = [i for i, k in enumerate(ks) if k[3].startswith("k_gemm") and k[3].rstrip().endswith("true>")]
if len(starts) < nsteps + 2:
    sys.exit("too few steps in the trace")
mainq = ks[starts[-1]][2]
main = [k for k in ks if k[2] == mainq]
prev_end = {id(k): main[i - 1][1] if i else k[0] for i, k in enumerate(main)}

table = {}       # position among the step's main-stream kernels -> [name, gaps]
walls, idles = [], []
for n in range(nsteps):
    lo, hi = starts[-2 - n], starts[-1 - n]
    step = ks[lo:hi]
    t0, t1 = ks[lo][0], ks[hi][0]
    walls.append((t1 - t0) / 1e3)
    pos = 0
    for k in step:
        if k[2] != mainq:
            continue
        table.setdefault(pos, [k[3], []])[1].append((k[0] - prev_end[id(k)]) / 1e3)
        pos += 1
    # time without a kernel on any queue, the gap in front of the step's first kernel included
    busy_end = max(k[1] for k in ks[:lo]) if lo else t0
    idle = 0.0
    for k in step:
        idle += max(0.0, (k[0] - busy_end) / 1e3)
        busy_end = max(busy_end, k[1])
    idles.append(idle)
    if n == 0:
        print("last complete step: %.1f us start to start, %d kernels, main stream = q%s" % (walls[0], len(step), mainq))
        for k in step:
            gap = (k[0] - prev_end[id(k)]) / 1e3 if k[2] == mainq else 0.0
            print("%8.1f  %7.1f us  q%-3s %s%s" % ((k[0] - t0) / 1e3, (k[1] - k[0]) / 1e3, k[2], k[3],
                                                   "   <-- main stream idle %.1f us before" % gap if gap > 1.0 else ""))

mean = lambda v: sum(v) / len(v)      # noqa: E731
print("\nmain-stream gaps, mean of the last %d steps (us)" % nsteps)
total = 0.0
for pos in sorted(table):
    name, gaps = table[pos]
    g = mean(gaps)
    total += g
    print("  %2d %-62s %6.2f%s" % (pos, name, g, "" if g <= 1.0 else "  *"))
print("  sum of main-stream gaps: %.1f us   (gaps over 1 us: %.1f us)"
      % (total, sum(mean(g) for _, g in table.values() if mean(g) > 1.0)))
print("  no kernel on any queue:  %.1f us" % mean(idles))
print("  step, start to start:    %.1f us" % mean(walls))
