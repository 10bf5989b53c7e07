"""Generate tests/golden/net_trace.json.gz (PUNetG) and tests/golden/adm_trace.json.gz (ADM and its stand-alone blocks): for every
case of a table of tests/net_trace.py, what the network of a given commit -- the PARENT of the change under test, never the
working tree -- hands to the library during a whole forward pass: every launch (entry
point, arguments, pointers as [label, byte offset]), the pool's take count, and a digest of every pool buffer ATen wrote.
tests/test_net_trace.py traces the working tree's network and requires the same record.

diffsci_amd/ of --rev is exported with `git archive` into a temporary directory; a child process traces with that directory
first on sys.path and DIFFSCI_HIP_LIB pointing at the working tree's built library (size and support queries only).  Runs on
the host.  Prints the entry points the cases reach; the golden keeps that list for the test to hold the case table to.
The file is minified JSON, gzipped with no timestamp: 590 KB of text would drown the diff of the change it pins, and the same
record gives the same bytes.  `zcat` shows it.

    python tools/make_net_trace_golden.py --rev <parent commit> [--table net_trace | adm_trace]"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHILD = """
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from tests import net_trace
import diffsci_amd
assert diffsci_amd.__file__.startswith(sys.argv[1]), diffsci_amd.__file__
json.dump({t: {name: net_trace.trace_of(name, net_trace.TABLES[t]) for name in net_trace.TABLES[t]} for t in sys.argv[3:]}, sys.stdout)
"""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", required=True, help="the commit whose diffsci_amd/ is the reference (the parent of the change)")
    ap.add_argument("--table", action="append", help="a table of tests/net_trace.py (TABLES) to write; default: every one")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from tests.net_trace import TABLES
    tables = args.table or list(TABLES)
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.rev], check=True, capture_output=True, text=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, "diffsci_amd"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        env = dict(os.environ, DIFFSCI_HIP_LIB=os.path.join(ROOT, "diffsci_amd", "_lib", "libdiffsci_hip.so"))
        child = subprocess.run([sys.executable, "-c", CHILD, tmp, ROOT] + tables, check=True, stdout=subprocess.PIPE, env=env)
    for table, cases in json.loads(child.stdout).items():
        write(os.path.join(GOLDEN, table + ".json.gz"), rev, cases)


def write(gold, rev, cases):
    for name, t in cases.items():
        print(f"{name}: {sum(c[0] != 'give' for c in t['calls'])} launches, {t['pool'][0]} pool buffers, {len(t['writes'])} written by ATen")
    reached = sorted({c[0] for t in cases.values() for c in t["calls"]} - {"give"})
    print(f"{sum(c[0] != 'give' for t in cases.values() for c in t['calls'])} launches through {len(reached)} entry points:", " ".join(reached))
    text = json.dumps({"diffsci_amd_of": rev, "entry_points": reached, "cases": cases}, separators=(",", ":")) + "\n"
    with open(gold, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write(text.encode())
    print(f"wrote {gold} ({os.path.getsize(gold)} bytes, {len(text)} of JSON)")


if __name__ == "__main__":
    main()
