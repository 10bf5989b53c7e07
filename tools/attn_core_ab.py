#!/usr/bin/env python3
"""Same-box A/B of the attention core's tile loop (k_attn3h) against a parent tree built in place (ab_parent/: a
`git archive` of the parent commit with `python build.py` run inside it), by the protocol of tools/attn_fold_ab.py.

    python tools/attn_core_ab.py trace            rocprofv3 --kernel-trace --stats over bench.py --gpus 1 --steps 1 --warmup 1,
                                                  parent then this tree: k_attn3h and three kernels that did not change
    python tools/attn_core_ab.py bench [rounds]   alternating bench.py --gpus 1 --steps 6 --warmup 2: parent (A), this tree,
                                                  parent (B); the bar is 3 x median |A - B|
    python tools/attn_core_ab.py dumps            bench.py --dump-outputs on the parent, this tree and the parent at
                                                  --precision fp32: rel-L2 and max-abs against the parent
    python tools/attn_core_ab.py cfg5             tools/bench_cfg5.py, parent then this tree
Every run is a child process under its own time limit; the first failure ends the script.  Output: stdout."""
import csv
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.environ.get("AB_PARENT", "ab_parent")
UNCHANGED = ("k_convup", "k_inorm_images", "k_attn_images")          # kernels no source of which differs: the clock drift


def run(cmd, tree, limit=300):
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=os.path.join(ROOT, tree), capture_output=True, text=True)
    if p.returncode != 0:
        print(f"{cmd} in {tree}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
        sys.exit(1)
    return p.stdout.strip().splitlines()[-1], time.time() - t0


def trace():
    out = {}
    for name, tree in (("parent", PARENT), ("child", ".")):
        d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"attn_core_trace_{name}")
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "b", "--", sys.executable, "bench.py",
             "--gpus", "1", "--steps", "1", "--warmup", "1"], tree, limit=400)
        f = sorted(glob.glob(d + "/**/b_kernel_trace.csv", recursive=True), key=os.path.getmtime)[-1]
        per = {}
        for r in csv.DictReader(open(f, newline="")):
            k = r["Kernel_Name"]
            key = "k_attn3h<8, true, false>" if "k_attn3h<8, true, false>" in k else next((u for u in UNCHANGED if u in k), None)
            if key:
                per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out[name] = per
        for k, v in sorted(per.items()):
            se = statistics.stdev(v) / len(v) ** 0.5
            print(f"{name:6s} {k:28s} n {len(v):5d}  avg {statistics.mean(v):8.2f} us  med {statistics.median(v):8.2f}  min {min(v):8.2f}  "
                  f"max {max(v):8.2f}  standard error {se:.3f}", flush=True)
    for k in sorted(out["parent"]):
        a, b = statistics.mean(out["parent"][k]), statistics.mean(out["child"][k])
        print(f"{k:28s} parent {a:8.2f} -> child {b:8.2f} us  ({100 * (b / a - 1):+.2f} %)")


def bench(rounds):
    arms = [("parentA", PARENT), ("child", "."), ("parentB", PARENT)]
    vals = {a[0]: [] for a in arms}
    for r in range(rounds):
        for name, tree in arms:
            line, dt = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "6", "--warmup", "2"], tree, limit=120)
            d = json.loads(line)
            vals[name].append(d["value"])
            gs = d.get("gpu_state", {})
            print(f"round {r} {name:8s} samples/s {d['value']}  ({dt:.0f} s)  sclk before/after "
                  f"{gs.get('before', {}).get('sclk_mhz')}/{gs.get('after', {}).get('sclk_mhz')}", flush=True)
    both = vals["parentA"] + vals["parentB"]
    parent, spread = statistics.median(both), statistics.median(abs(a - b) for a, b in zip(vals["parentA"], vals["parentB"]))
    child = statistics.median(vals["child"])
    print(f"|A - B| per round: {' '.join(f'{abs(a - b):.3f}' for a, b in zip(vals['parentA'], vals['parentB']))}; median {spread:.3f} "
          f"samples/s = {100 * spread / parent:.2f} % of the parent's median {parent:.3f}; bar 3 x = {300 * spread / parent:.2f} %")
    print(f"parent, all runs: {min(both):.3f} .. {max(both):.3f}")
    print(f"child   median {child:.3f} = {100 * (child / parent - 1):+.2f} % against the parent's median; range {min(vals['child']):.3f} .. "
          f"{max(vals['child']):.3f}; every child run above every parent run: {min(vals['child']) > max(both)}")


def dumps():
    import numpy as np
    arrs = {}
    for name, tree, extra in [("parent", PARENT, []), ("child", ".", []), ("parent_fp32", PARENT, ["--precision", "fp32"])]:
        d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"attn_core_dump_{name}")
        _, dt = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", d] + extra, tree)
        f = os.path.join(d, "samples.npy")
        arrs[name] = np.load(f).astype(np.float64)
        print(f"dump {name}: samples.npy sha256/16 = {hashlib.sha256(open(f, 'rb').read()).hexdigest()[:16]}  ({dt:.0f} s)", flush=True)
    ref = arrs["parent"]
    for name in ("child", "parent_fp32"):
        a = arrs[name]
        print(f"{name} against parent: rel-L2 {np.linalg.norm(a - ref) / np.linalg.norm(ref):.3e}  max-abs {np.abs(a - ref).max():.3e}  "
              f"(max |parent| {np.abs(ref).max():.3f})")


def cfg5():
    for name, tree in (("parent", PARENT), ("child", ".")):
        line, dt = run([sys.executable, "tools/bench_cfg5.py"], tree, limit=420)
        print(f"cfg5 {name}: {line}  ({dt:.0f} s)", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "bench"
    if what == "trace":
        trace()
    elif what == "bench":
        bench(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    elif what == "dumps":
        dumps()
    elif what == "cfg5":
        cfg5()
    else:
        sys.exit(__doc__)
