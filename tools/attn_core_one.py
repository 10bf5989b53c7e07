"""One fp16x3 attention shape, a few launches -- for rocprofv3 --pmc passes and kernel traces of the attention core
(k_attn3h, ds_attn3h.hip).  Run from the root of the tree whose library is to be measured.

    python tools/attn_core_one.py [B E L heads form n]      form: images | staged; defaults 64 256 1024 1 images 10"""
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops

a = sys.argv[1:]
B, E, L, H = (int(v) for v in (a + ["64", "256", "1024", "1"][len(a):])[:4])
form = a[4] if len(a) > 4 else "images"
n = int(a[5]) if len(a) > 5 else 10
ops.ATTN_IMAGES_MIN_L = ops.ATTN_IMAGES_MIN_L_WIDE = 0 if form == "images" else 1 << 30
dev = torch.device("cuda:0")
qkv = torch.randn(B, 3 * E, L, device=dev, generator=torch.Generator(dev).manual_seed(1))
out = torch.empty(B, E, L, device=dev)
nws = ops.attention_workspace_floats(B, E, L, "fp16x3", heads=H)
ws = torch.empty(nws, device=dev) if nws else None
rows = torch.cat([ops.absmax_rows(qkv[:, :2 * E]), ops.absmax_rows(qkv[:, 2 * E:])])
for _ in range(n):
    ops.attention(qkv, E, out=out, precision="fp16x3", workspace=ws, in_amax=rows, heads=H)
torch.cuda.synchronize()
print(f"B{B} E{E} L{L} H{H} {form}: {n} launches, finite {bool(torch.isfinite(out).all())}")
