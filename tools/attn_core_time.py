"""Time the fp16x3 attention entry (pre-pass + core where the image form runs) with the library of the tree it is run in: the
headline shape, L = 4096, and the small shapes of tests/test_gpu_attention_core.py in the form with a head axis and the form
that stages in the workgroup.  Five batches of n launches between two events each; prints the median and the spread.

    python <this tree>/tools/attn_core_time.py [--sha]      --sha: also a hash of each output, to compare two libraries' bits"""
import hashlib
import os
import statistics
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops

dev = torch.device("cuda:0")
CASES = [(64, 256, 1024, 1, "images", 20), (16, 256, 4096, 1, "images", 5), (64, 256, 1024, 1, "staged", 20),
         (32, 512, 1024, 2, "images", 20),
         (3, 256, 160, 1, "images", 200), (3, 256, 160, 1, "staged", 200), (3, 512, 32, 2, "images", 200), (3, 512, 32, 2, "staged", 200),
         (3, 32, 96, 1, "images", 200), (3, 32, 96, 1, "staged", 200)]
for B, E, L, H, form, n in CASES:
    ops.ATTN_IMAGES_MIN_L = ops.ATTN_IMAGES_MIN_L_WIDE = 0 if form == "images" else 1 << 30
    qkv = torch.randn(B, 3 * E, L, generator=torch.Generator().manual_seed(B + E + L)).to(dev)
    out = torch.empty(B, E, L, device=dev)
    nws = ops.attention_workspace_floats(B, E, L, "fp16x3", heads=H)
    ws = torch.empty(nws, device=dev) if nws else None
    rows = torch.cat([ops.absmax_rows(qkv[:, :2 * E]), ops.absmax_rows(qkv[:, 2 * E:])])
    f = lambda: ops.attention(qkv, E, out=out, precision="fp16x3", workspace=ws, in_amax=rows, heads=H)   # noqa: E731
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / n * 1e3)
    sha = "  sha " + hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16] if "--sha" in sys.argv else ""
    print(f"B{B} E{E} L{L} H{H} {form:6s}: median {statistics.median(us):8.1f} us  (min {min(us):.1f}, max {max(us):.1f}; "
          f"{4.0 * L * L * E * B / statistics.median(us) / 1e6:6.1f} TF-eq){sha}", flush=True)
