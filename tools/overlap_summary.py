"""Which kernels ran beside a given kernel: for every launch in a rocprofv3 --kernel-trace kernel_trace.csv whose name matches
PATTERN, the time it shared with other launches (their [start, end) intersected with its own), summed per other kernel.
    usage: python tools/overlap_summary.py <kernel_trace.csv> <pattern>      e.g.  ... gemm3_grouped_kernel
A launch sequence on one stream shares nothing (the table is empty); the weight gradients on the side stream (vbx_wgrad_overlap)
share their time with the norm backward and the next layer's chain."""
import collections
import csv
import re
import sys

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    name = re.sub(r"\(anonymous namespace\)::|void ", "", r["Kernel_Name"]).split("(")[0][:70]
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
rows.sort()
pat = re.compile(sys.argv[2])
targets = [i for i, r in enumerate(rows) if pat.search(r[2])]
shared = collections.defaultdict(float)
own = alone = 0.0
started_beside = 0
for i in targets:
    s, e, _ = rows[i]
    own += (e - s) / 1e3
    beside = False
    cover = []  # intervals of other launches inside [s, e)
    for j in range(max(0, i - 64), min(len(rows), i + 512)):
        if j == i:
            continue
        s2, e2, n2 = rows[j]
        if s2 >= e:
            break
        lo, hi = max(s, s2), min(e, e2)
        if hi > lo:
            shared[n2] += (hi - lo) / 1e3
            cover.append((lo, hi))
            beside |= s2 <= s < e2
    started_beside += beside
    cover.sort()
    t, cur = 0, s
    for lo, hi in cover:
        if hi > cur:
            t += hi - max(lo, cur)
            cur = hi
    alone += ((e - s) - t) / 1e3
n = max(len(targets), 1)
print(f"{len(targets)} launches matching '{sys.argv[2]}': {own / n:.1f} us each on average, of which {alone / n:.1f} us with nothing else "
      f"running; {started_beside} of them started while another kernel was running")
print(f"{'kernel running beside them':72s} {'shared us / launch':>18s}")
for k, v in sorted(shared.items(), key=lambda kv: -kv[1])[:12]:
    print(f"{k:72s} {v / n:18.1f}")
