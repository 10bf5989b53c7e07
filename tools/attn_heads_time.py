"""Time ops.attention (fp16x3) with a head axis at E = 256: H = 1, 4, 8 at L = 1024 (B = 64) and L = 4096 (B = 16), the
K / V staging forms side by side (in every workgroup / pre-split images), on the same inputs.  Device events around 20
launches after a warm-up, three rounds alternating the variants; the median round is printed."""
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops

dev = torch.device("cuda:0")


def timed(f, n=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for B, E, L in ((64, 256, 1024), (16, 256, 4096)):
    qkv = torch.randn(B, 3 * E, L, device=dev)
    rows = ops.amax_new(2 * B, dev)
    ops.absmax_rows(qkv[:, :2 * E], out=rows[:B])
    ops.absmax_rows(qkv[:, 2 * E:], out=rows[B:])
    out = torch.empty(B, E, L, device=dev)
    ws = torch.empty(B * L * E * 2, device=dev)                # the largest image workspace (B L E 8 bytes)
    variants = {}
    for H in (1, 4, 8):
        for form in ("staged", "images"):
            use = form == "images"
            def f(H=H, use=use):
                ops.ATTN_IMAGES_MIN_L = ops.ATTN_IMAGES_MIN_L_WIDE = 0 if use else 1 << 30
                return ops.attention(qkv, E, out=out, precision="fp16x3", workspace=ws, in_amax=rows, heads=H)
            variants[(H, form)] = f
    ref = {}
    for key, f in variants.items():                           # warm-up; the two forms agree bit for bit
        f()
        torch.cuda.synchronize()
        ref.setdefault(key[0], out.clone())
        assert torch.equal(ref[key[0]], out), key
    times = {k: [] for k in variants}
    for _ in range(3):
        for key, f in variants.items():
            times[key].append(timed(f))
    for (H, form), t in times.items():
        us = sorted(t)[1]
        print(f"B{B} E{E} L{L} H{H} d{E // H:3d} {form:6s}: {us:8.1f} us (rounds {', '.join(f'{x:.1f}' for x in t)})  "
              f"{4.0 * L * L * E * B / us / 1e6:6.1f} TF-eq", flush=True)
