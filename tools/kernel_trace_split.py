#!/usr/bin/env python3
"""Per-launch-site statistics from a rocprofv3 kernel trace: the --stats table merges the launches of one kernel, this splits
them by grid size and by the kernel launched in front of them (e.g. the attention block's in- and out-projection: both
k_conv1h, with the folded block of one grid, the second behind k_attn3h).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o b -- python3 bench.py --gpus 1 --steps 1 --warmup 1
    python tools/kernel_trace_split.py DIR/.../b_kernel_trace.csv [substring of a kernel name ...]      (default: k_conv1h k_attn)"""
import csv
import sys
from collections import defaultdict


def main():
    path, pats = sys.argv[1], sys.argv[2:] or ["k_conv1h", "k_attn"]
    rows = defaultdict(list)
    with open(path, newline="") as f:
        recs = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    prev = "-"                                       # the launch in front tells two launches of one kernel and grid apart
    for r in recs:
        name = r["Kernel_Name"]
        short = name.replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "").split("(")[0]
        if any(p in name for p in pats):
            rows[(short + "  after " + prev.split("<")[0], r["Grid_Size_X"], r["Grid_Size_Y"], r["Workgroup_Size_X"])].append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        prev = short
    print(f"{'kernel':84s} {'grid':>16s} {'wg':>5s} {'n':>6s} {'avg us':>9s} {'med us':>9s} {'min us':>9s} {'max us':>9s}")
    for (k, gx, gy, wg), v in sorted(rows.items()):
        v.sort()
        print(f"{k[:84]:84s} {gx + 'x' + gy:>16s} {wg:>5s} {len(v):6d} {sum(v) / len(v):9.1f} {v[len(v) // 2]:9.1f} {v[0]:9.1f} {v[-1]:9.1f}")


if __name__ == "__main__":
    main()
