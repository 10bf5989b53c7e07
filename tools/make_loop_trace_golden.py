"""Generate tests/golden/loop_trace.json: for every case of tests/loop_trace.py, what the sampler loops of a given commit -- the
PARENT of the change under test, never the working tree -- hand to the library during one run: every launch (entry point, scalars
with every field of the coefficient structs, pointers as [label, byte offset]), the Philox state set_noise wrote, where the
result lives.  tests/test_loop_trace.py traces the working tree's loops and requires the same record.

diffsci_amd/ of --rev is exported with `git archive` into a temporary directory; a child process traces with that directory
first on sys.path and DIFFSCI_HIP_LIB pointing at the working tree's built library (size and support queries only).  Runs on
the host; the golden names the host's CPU kernel set, since the step tables' scalars are exact only on the same one.  Prints
the entry points the cases reach; the golden keeps that list for the test to hold the case table to.  One case per line, so a
changed case shows as one changed line.

    python tools/make_loop_trace_golden.py --rev <parent commit>"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_trace.json")
CHILD = """
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from tests import loop_trace
import diffsci_amd
assert diffsci_amd.__file__.startswith(sys.argv[1]), diffsci_amd.__file__
import torch
from tests.golden_util import cpu_vendor
json.dump({"cpu_capability": torch.backends.cpu.get_cpu_capability(), "cpu_vendor": cpu_vendor(),
           "cases": {name: loop_trace.trace_of(name) for name in loop_trace.CASES}}, sys.stdout)
"""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", required=True, help="the commit whose diffsci_amd/ is the reference (the parent of the change)")
    args = ap.parse_args()
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.rev], check=True, capture_output=True, text=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, "diffsci_amd"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        env = dict(os.environ, DIFFSCI_HIP_LIB=os.path.join(ROOT, "diffsci_amd", "_lib", "libdiffsci_hip.so"))
        child = subprocess.run([sys.executable, "-c", CHILD, tmp, ROOT], check=True, stdout=subprocess.PIPE, env=env)
    made = json.loads(child.stdout)
    cases = made.pop("cases")
    for name, t in cases.items():
        print(f"{name}: {len(t['calls'])} launches")
    reached = sorted({c[0] for t in cases.values() for c in t["calls"]} - {"give"})
    print(f"{len(reached)} entry points:", " ".join(reached))
    dump = lambda v: json.dumps(v, separators=(",", ":"))      # noqa: E731
    with open(GOLDEN, "w") as f:
        f.write('{"diffsci_amd_of":%s,"cpu":%s,"entry_points":%s,"cases":{\n' % (dump(rev), dump(made), dump(reached)))
        f.write(",\n".join(f"{dump(name)}:{dump(t)}" for name, t in cases.items()))
        f.write("\n}}\n")
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
