"""Launch table of a rocprofv3 --kernel-trace run (kernel_trace.csv): kernel name x grid x workgroup size -> call count, total and
average time.  Two builds issue the same launches when their tables agree in every column but the times
(`launch_table.py a.csv --no-times` prints only those columns, for diff)."""
import collections
import csv
import re
import sys


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return n.split("(")[0][:100]


def table(path):
    agg = collections.defaultdict(lambda: [0, 0.0])
    for r in csv.DictReader(open(path)):
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        a = agg[(short(r["Kernel_Name"]), grid, wg)]
        a[0] += 1
        a[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    return agg


if __name__ == "__main__":
    times = "--no-times" not in sys.argv
    agg = table(sys.argv[1])
    print(f"{'kernel':100s} {'grid':>16s} {'workgroup':>10s} {'calls':>6s}" + (f" {'total_us':>10s} {'avg_us':>9s}" if times else ""))
    for (name, grid, wg), (c, t) in sorted(agg.items()):
        print(f"{name:100s} {grid:>16s} {wg:>10s} {c:6d}" + (f" {t:10.1f} {t / c:9.2f}" if times else ""))
    print(f"{len(agg)} rows, {sum(v[0] for v in agg.values())} launches" + (f", {sum(v[1] for v in agg.values()) / 1e3:.2f} ms" if times else ""))
