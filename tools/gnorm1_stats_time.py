#!/usr/bin/env python3
"""ds_gnorm1_stats alone on ADM-sized tensors: device events around 20 launches, best and worst of five such windows, and
the stream rate in GB/s (4 B per element).  DIFFSCI_HIP_LIB selects another build of the library for a comparison.

    python tools/gnorm1_stats_time.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsci_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
for shape in ((32, 128, 256, 256), (32, 256, 128, 128), (32, 512, 64, 64), (8, 512, 32, 32)):
    x = torch.randn(shape, device=dev)
    st = torch.empty(shape[0], 2, device=dev)
    ws = torch.empty(ops.N.lib().ds_gnorm1_workspace_bytes(shape[0]) // 4, device=dev)
    for _ in range(5):
        ops.gnorm1_stats(x, 0, stats=st, workspace=ws)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            ops.gnorm1_stats(x, 0, stats=st, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 20)
    t = min(ts)
    print(f"gnorm1_stats {shape}: {1e3 * t:.1f} us min, {1e3 * max(ts):.1f} us max of 5x20, {x.numel() * 4 / t / 1e6:.0f} GB/s")
    del x
