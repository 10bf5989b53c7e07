"""Time the ConVit kernels (ds_convit.hip) and one ConVit evaluation at embed_dim 64 and 256 on 128^2 fields, batch 32.

Device events around a window of launches after a warm-up (as many launches as fill about 30 ms, at least 20), three rounds; the
median round is printed with the achieved HBM rate -- the bytes the operation has to move (every input read once, the output
written once, computed from the shapes) over the time -- next to ds_token_layernorm on a [B, E, H*W] tensor of the same byte
count, the one streaming kernel of comparable shape the library had before.  Every kernel that can leave an out_amax is timed
with and without it (the network always asks for it), and so is ds_token_layernorm; the slots are zeroed by a ds_fill_u32 launch
in front of every timed launch that commits, as a forward pass finds them (its few microseconds are inside the figure).  The 128 MiB tensors of embed_dim 64 fit
the 256 MiB Infinity Cache, those of embed_dim 256 do not.
Then one eager evaluation of a 2-layer ConVit (default options otherwise: 8 heads, pooling by 2, so the attention runs on 64^2 = 4096 positions) with the time of its attention core alone, and the share that is.

    python tools/convit_time.py            # both widths
    python tools/convit_time.py 64         # one width"""
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops

dev = torch.device("cuda:0")
PEAK_GBS = 8000.0
B, H, W, F = 32, 128, 128, 2


def timed(f, n=None):
    f()
    torch.cuda.synchronize()
    if n is None:                                          # enough launches for a window of about 30 ms
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            f()
        e1.record()
        torch.cuda.synchronize()
        n = int(min(2000, max(20, 30.0 / max(e0.elapsed_time(e1) / 5, 1e-3))))
    rounds = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / n * 1e3)
    return sorted(rounds)[1]


def report(name, f, nbytes, n=None):
    us = timed(f, n)
    gbs = nbytes / us / 1e3
    print(f"{name:58s} {us:9.1f} us  {nbytes / 2**20:8.1f} MiB  {gbs:7.0f} GB/s  {100 * gbs / PEAK_GBS:5.1f}% of peak", flush=True)
    return us


def layernorm_at(nbytes, E):
    """ds_token_layernorm moving `nbytes` (read + write of one [B, E, L] tensor)."""
    L = max(4, nbytes // (2 * 4 * B * E) // 4 * 4)
    x, o = torch.randn(B, E, L, device=dev), torch.empty(B, E, L, device=dev)
    w, b = torch.ones(E, device=dev), torch.zeros(E, device=dev)
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    report(f"  token_layernorm [{B},{E},{L}]", lambda: ops.token_layernorm(x, w, b, out=o), 8 * x.numel())
    report(f"  token_layernorm [{B},{E},{L}] + out_amax", lambda: (ops.amax_zero(slots), ops.token_layernorm(x, w, b, out=o, out_amax=slots)), 8 * x.numel())


def kernels(E):
    from diffsci_amd.models.nets.convit import LearnedRoPE
    heads = 8
    x = torch.randn(B, E, H, W, device=dev)
    o = torch.empty_like(x)
    op = torch.empty(B, E, H // F, W // F, device=dev)
    w, mod = torch.ones(E, device=dev), torch.randn(B, E, device=dev)
    slots = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    full = 4 * x.numel()
    print(f"--- embed_dim={E}, [{B},{E},{H},{W}] ({full / 2**20:.0f} MiB)", flush=True)
    report("channel_rmsnorm", lambda: ops.channel_rmsnorm(x, w, mod, out=o), 2 * full)
    report("channel_rmsnorm + out_amax", lambda: (ops.amax_zero(slots), ops.channel_rmsnorm(x, w, mod, out=o, out_amax=slots[:B])), 2 * full)
    layernorm_at(2 * full, E)
    report("channel_rmsnorm pool=2", lambda: ops.channel_rmsnorm(x, w, mod, pool=F, out=op), full + full // 4)
    report("channel_rmsnorm pool=2 + out_amax", lambda: (ops.amax_zero(slots), ops.channel_rmsnorm(x, w, mod, pool=F, out=op, out_amax=slots[:B])), full + full // 4)
    layernorm_at(full + full // 4, E)
    L = (H // F) * (W // F)
    qkv = torch.randn(B, 3 * E, L, device=dev)
    cs = LearnedRoPE(E // heads, 2).to(dev).cos_sin((H // F, W // F))
    report(f"rope2d [{B},{3 * E},{L}] (q, k read + written, v read)", lambda: ops.rope2d(qkv, E, heads, cs), 4 * qkv.numel() * 5 // 3)
    report(f"rope2d [{B},{3 * E},{L}] + amax pair", lambda: (ops.amax_zero(slots), ops.rope2d(qkv, E, heads, cs, out_amax=slots)), 4 * qkv.numel() * 5 // 3)
    layernorm_at(4 * qkv.numel() * 5 // 3, E)
    report("upsample_bilinear x2", lambda: ops.upsample_bilinear(op, F, out=o), full + full // 4)
    layernorm_at(full + full // 4, E)
    for k in (3, 7):
        wk, bk = torch.randn(E, 1, k, k, device=dev) / k, torch.zeros(E, device=dev)
        report(f"depthwise_conv_silu k={k}", lambda: ops.depthwise_conv_silu(x, wk, bk, out=o), 2 * full)
        report(f"depthwise_conv_silu k={k} + out_amax", lambda: (ops.amax_zero(slots), ops.depthwise_conv_silu(x, wk, bk, out=o, out_amax=slots[:B])), 2 * full)
    layernorm_at(2 * full, E)
    ag = torch.randn(B, 2 * E, H, W, device=dev)
    report(f"swiglu [{B},{2 * E},{H},{W}]", lambda: ops.swiglu(ag, out=o), 3 * full)
    report(f"swiglu [{B},{2 * E},{H},{W}] + out_amax", lambda: (ops.amax_zero(slots), ops.swiglu(ag, out=o, out_amax=slots[:B])), 3 * full)
    layernorm_at(3 * full, E)
    s = torch.full((1,), 0.5, device=dev)
    xc, x0 = torch.randn_like(x), torch.randn_like(x)
    report("convit_blend (in place on x0)", lambda: ops.convit_blend(x, xc, x0, s, out=x0), 4 * full)
    layernorm_at(4 * full, E)


def forward(E):
    import diffsci_amd.models as M
    torch.manual_seed(0)
    kw = dict(embed_dim=E, num_layers=2, has_time_embedding=True, has_conditional_embedding=True)
    net = M.nets.ConVit(M.nets.ConVitConfig(**kw), conditional_embedding=torch.nn.Linear(1, E)).to(dev).eval()
    x, t = torch.randn(B, 1, H, W, device=dev), torch.rand(B, device=dev)
    with torch.no_grad():
        te = net.embed_time(t)
        shifts = net.time_shifts(te)
        us = timed(lambda: net.forward_with_shifts(x, shifts), n=3)
    L = (H // F) * (W // F)
    qkv = torch.randn(B, 3 * E, L, device=dev)
    o = torch.empty(B, E, L, device=dev)
    nws = ops.attention_workspace_floats(B, E, L, "fp16x3", heads=8)
    aws = torch.empty(nws, device=dev) if nws else None
    pair = torch.zeros(2 * B, dtype=torch.int32, device=dev)          # the exponents the network's rope2d leaves: no reduction, no allocation
    ops.absmax_rows(qkv[:, :2 * E], out=pair[:B])
    ops.absmax_rows(qkv[:, 2 * E:], out=pair[B:])
    a_o = torch.zeros(B, dtype=torch.int32, device=dev)
    ua = timed(lambda: ops.attention(qkv, E, out=o, precision="fp16x3", workspace=aws, heads=8, in_amax=pair, out_amax=a_o), n=3)
    print(f"ConVit embed_dim={E}, 2 layers, 8 heads (head width {E // 8}), [{B},1,{H},{W}]: {us / 1e3:9.2f} ms per evaluation; "
          f"attention core on {L} positions {ua / 1e3:8.2f} ms per block = {100 * 2 * ua / us:5.1f}% of the evaluation", flush=True)
    del net
    torch.cuda.empty_cache()


if __name__ == "__main__":
    widths = [int(a) for a in sys.argv[1:]] or [64, 256]
    for E in widths:
        kernels(E)
        torch.cuda.empty_cache()
    for E in widths:
        forward(E)
