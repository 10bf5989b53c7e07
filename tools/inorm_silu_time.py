#!/usr/bin/env python3
"""ds_inorm_silu alone at planes of 1024 < HW <= 4096 floats, where it runs one wave per plane with 8 or 16 vectors per lane, many
and few planes, and two controls (32 x 32, 128 x 128): device events around 20 launches, best and worst of five such windows, and the
stream rate in GB/s (8 B per element).  DIFFSCI_HIP_LIB selects another build of the library for a comparison.

    python tools/inorm_silu_time.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsci_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
print("library:", os.environ.get("DIFFSCI_HIP_LIB", "product"))
for shape in ((64, 128, 64, 64), (64, 64, 64, 64), (64, 128, 48, 40), (64, 256, 32, 40), (8, 64, 64, 64), (1, 64, 64, 64), (2, 32, 48, 40),
              (64, 256, 32, 32), (64, 64, 128, 128)):
    x = torch.randn(shape, device=dev)
    y = torch.empty_like(x)
    w = torch.ones(shape[1], device=dev)
    for kind in (0, 1):
        for _ in range(5):
            ops.inorm_silu(x, w, w, kind, out=y)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                ops.inorm_silu(x, w, w, kind, out=y)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / 20)
        t = min(ts)
        print(f"inorm_silu {shape} kind {kind}: {1e3 * t:.1f} us min, {1e3 * max(ts):.1f} us max of 5x20, {x.numel() * 8 / t / 1e6:.0f} GB/s")
    del x, y
