#!/usr/bin/env python3
"""Compare this tree's device assembly with another checkout's, file by file (needs hipcc, no GPU; 5-10 s per file).
    python tools/device_asm_diff.py <checkout of another commit> [ds_norm.hip ...]     (default: every entry of build.SOURCES)
Each file is compiled in both trees with the library's own flags, --cuda-device-only -S in place of -c.  The lines naming
__hip_cuid_ (the per-translation-unit id symbol, the only thing that differs between two compiles of equal code) are dropped;
the rest, kernel descriptors (.amdhsa_) included, is compared as text.  Exit status 1 if any file differs."""
import difflib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import build  # noqa: E402


def device_asm(root, name):
    src = os.path.join(root, "diffsci_amd", "csrc", name)
    cmd = [build.HIPCC] + build.FLAGS + build.EXTRA_FLAGS.get(name, []) + ["--cuda-device-only", "-S", src, "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}\n{r.stderr}")
    return [ln for ln in r.stdout.splitlines() if "__hip_cuid_" not in ln]


def differing_lines(theirs, mine):
    return sum(1 for ln in difflib.unified_diff(theirs, mine, lineterm="", n=0) if ln[0] in "+-" and ln[:3] not in ("+++", "---"))


if __name__ == "__main__":
    other = os.path.abspath(sys.argv[1])
    names = sys.argv[2:] or build.SOURCES
    with ThreadPoolExecutor(max_workers=16) as pool:                                 # at most 16 compiles at a time
        asm = list(pool.map(lambda job: device_asm(*job), [(root, n) for n in names for root in (other, build.ROOT)]))
    counts = [differing_lines(asm[2 * i], asm[2 * i + 1]) for i in range(len(names))]
    for name, n in zip(names, counts):
        print(f"{name:20s} {'identical' if n == 0 else f'{n} lines differ'}")
    sys.exit(1 if any(counts) else 0)
