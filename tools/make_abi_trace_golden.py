"""Generate tests/golden/abi_trace.json: for every case of tests/abi_trace.py, the launches (entry point, arguments, pointers
as [label, byte offset]) that the ops.py of a given commit -- the PARENT of the change under test, never the working tree --
makes through a recording stand-in for the library.  tests/test_abi_trace.py replays the cases against the working tree and
requires the same record.  Runs on the host; needs the built library for the size and support queries only.

    python tools/make_abi_trace_golden.py --rev <parent commit>"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import abi_trace  # noqa: E402


def load_ops(rev):
    """diffsci_amd/ops.py as of `rev`, as a module of the diffsci_amd package next to the working tree's own."""
    src = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:diffsci_amd/ops.py"], check=True, capture_output=True, text=True).stdout
    spec = importlib.util.spec_from_loader("diffsci_amd._ops_at_rev", loader=None)
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "diffsci_amd"
    exec(compile(src, f"{rev}:diffsci_amd/ops.py", "exec"), mod.__dict__)
    return mod


def drop_device_tests(ops):
    """The traced tensors live on the host.  That ops.py tests "on the current device" in three places of its own
    (require_device, _pi, _philox): each is replaced by itself without that test."""
    def require_device(t, what="tensor"):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{what} has dtype {t.dtype}; the HIP path is fp32 only")

    def _pi(t, n, what="amax"):
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
            raise TypeError(f"{what} must be a contiguous int32 tensor of {n} entries")
        return t.data_ptr()

    def _philox(philox):
        if philox is None:
            return None, 0
        state, offset = philox
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.int64 and state.numel() == 2 and state.is_contiguous()):
            raise TypeError("philox state must be a contiguous int64[2] tensor (seed, base offset)")
        return state.data_ptr(), int(offset)
    for fn in (require_device, _pi, _philox):
        assert hasattr(ops, fn.__name__), fn.__name__
        setattr(ops, fn.__name__, fn)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", required=True, help="the commit whose ops.py is the reference (the parent of the change)")
    args = ap.parse_args()
    ops = load_ops(args.rev)
    drop_device_tests(ops)
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.rev], check=True, capture_output=True, text=True).stdout.strip()
    gold = {"ops_py_of": rev, "cases": {}}
    for name, fn in abi_trace.CASES.items():
        gold["cases"][name] = abi_trace.trace_of(ops, setattr, fn)
        print(f"{name}: {len(gold['cases'][name]['calls'])} launches")
    reached = {c[0] for t in gold["cases"].values() for c in t["calls"]}
    print("launch entry points never reached:", sorted(set(abi_trace.LAUNCHES) - reached))
    path = os.path.join(ROOT, "tests", "golden", "abi_trace.json")
    with open(path, "w") as f:
        json.dump(gold, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
