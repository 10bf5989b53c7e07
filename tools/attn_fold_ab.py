#!/usr/bin/env python3
"""Same-box A/B of the folded attention block (PUNetG.attn_fold) against a parent tree built in place
(ab_parent/: a `git archive` of the parent commit, `python build.py` run inside it; git-ignored like every ab_*/).

    python tools/attn_fold_ab.py bench [rounds]    alternating bench.py --gpus 1 --steps 6 --warmup 2: parent (A), this tree,
                                                   this tree with DIFFSCI_ATTN_FOLD=0, parent (B); the bar is 3 x median |A - B|
    python tools/attn_fold_ab.py dumps             bench.py --dump-outputs on the parent, this tree, this tree with the fold off
                                                   and the parent at --precision fp32: sha256, rel-L2 and max-abs against the parent
    python tools/attn_fold_ab.py cfg5              tools/bench_cfg5.py, parent then this tree
Every run is a child process under its own time limit; the first failure ends the script.  Output: stdout."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.environ.get("AB_PARENT", "ab_parent")


def run(cmd, tree, env=None, limit=300):
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, cwd=os.path.join(ROOT, tree),
                       env=dict(os.environ, **(env or {})), capture_output=True, text=True)
    if p.returncode != 0:
        print(f"{cmd} in {tree}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
        sys.exit(1)
    return p.stdout.strip().splitlines()[-1], time.time() - t0


def bench(rounds):
    arms = [("parentA", PARENT, {}), ("fold", ".", {}), ("fold_off", ".", {"DIFFSCI_ATTN_FOLD": "0"}), ("parentB", PARENT, {})]
    vals = {a[0]: [] for a in arms}
    for r in range(rounds):
        for name, tree, env in arms:
            line, dt = run(["bench.py", "--gpus", "1", "--steps", "6", "--warmup", "2"], tree, env, limit=120)
            d = json.loads(line)
            vals[name].append(d["value"])
            gs = d.get("gpu_state", {})
            print(f"round {r} {name:9s} samples/s {d['value']}  ({dt:.0f} s)  sclk before/after "
                  f"{gs.get('before', {}).get('sclk_mhz')}/{gs.get('after', {}).get('sclk_mhz')}", flush=True)
    med = {k: statistics.median(v) for k, v in vals.items()}
    both = vals["parentA"] + vals["parentB"]
    parent, spread = statistics.median(both), statistics.median(abs(a - b) for a, b in zip(vals["parentA"], vals["parentB"]))
    print(f"medians: {med}")
    print(f"|A - B| per round: {' '.join(f'{abs(a - b):.3f}' for a, b in zip(vals['parentA'], vals['parentB']))}; median {spread:.3f} "
          f"samples/s = {100 * spread / parent:.2f} % of the parent's median {parent:.3f}; bar 3 x = {300 * spread / parent:.2f} %")
    print(f"parent, all runs: {min(both):.3f} .. {max(both):.3f}")
    for k in ("fold", "fold_off"):
        print(f"{k:9s} median {med[k]:.3f} = {100 * (med[k] / parent - 1):+.2f} % against the parent's median; "
              f"range {min(vals[k]):.3f} .. {max(vals[k]):.3f}")


def dumps():
    import numpy as np
    arrs = {}
    for name, tree, env, extra in [("parent", PARENT, {}, []), ("child", ".", {}, []), ("child_fold_off", ".", {"DIFFSCI_ATTN_FOLD": "0"}, []),
                                   ("parent_fp32", PARENT, {}, ["--precision", "fp32"])]:
        d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"attn_fold_dump_{name}")
        _, dt = run(["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "1", "--dump-outputs", d] + extra, tree, env)
        f = os.path.join(d, "samples.npy")
        arrs[name] = np.load(f).astype(np.float64)
        print(f"dump {name}: samples.npy sha256/16 = {hashlib.sha256(open(f, 'rb').read()).hexdigest()[:16]}  ({dt:.0f} s, "
              f"{os.path.getsize(f)} bytes)", flush=True)
    ref = arrs["parent"]
    for name in ("child", "child_fold_off", "parent_fp32"):
        a = arrs[name]
        print(f"{name} against parent: rel-L2 {np.linalg.norm(a - ref) / np.linalg.norm(ref):.3e}  max-abs {np.abs(a - ref).max():.3e}  "
              f"(max |parent| {np.abs(ref).max():.3f})")


def cfg5():
    for name, tree in (("parent", PARENT), ("child", ".")):
        line, dt = run(["tools/bench_cfg5.py"], tree, limit=420)
        print(f"cfg5 {name}: {line}  ({dt:.0f} s)", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "bench"
    if what == "bench":
        bench(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif what == "dumps":
        dumps()
    elif what == "cfg5":
        cfg5()
    else:
        sys.exit(__doc__)
