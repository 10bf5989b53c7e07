"""Time one DiffusionTransformer evaluation and each of its token kernels (ds_tokens.hip) on the GPU, at
  nembed=256, nheads=4, nblocks=6, patch_size=4 on [16,1,128,128]  (L = 1024 tokens, head width 64: the fp16x3 head-axis attention)
  the defaults (nembed=64, nheads=4: head width 16, the generic attention) on [64,1,128,128].
Device events around 20 launches after a warm-up, three rounds; the median round is printed.  For the LayerNorm, gate and SiLU
kernels the achieved fraction of the 8 TB/s HBM peak, counting one read and one write of the tensor (two reads for the gate); both
tensors here (16 MiB) fit the 256 MiB Infinity Cache, as they do inside an evaluation.  The evaluation is the eager
forward_unguarded (time path included), with the time of its pieces beside it: the 1x1 convolutions and the attention of one block.

    python tools/dit_time.py"""
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops
import diffsci_amd.models as M

dev = torch.device("cuda:0")
PEAK_GBS = 8000.0


def timed(f, n=20):
    f()
    torch.cuda.synchronize()
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


def report(name, f, nbytes=None):
    us = timed(f)
    if nbytes is None:
        print(f"{name:64s} {us:9.1f} us", flush=True)
        return us
    gbs = nbytes / us / 1e3
    print(f"{name:64s} {us:9.1f} us  {nbytes / 2**20:8.1f} MiB  {gbs:7.0f} GB/s  {100 * gbs / PEAK_GBS:5.1f}% of peak", flush=True)
    return us


def case(kw, shape):
    torch.manual_seed(0)
    net = M.DiffusionTransformer(**kw).to(dev).eval()
    B, C, H, W = shape
    p, E = net.patch_size, net.nembed
    L = (H // p) * (W // p)
    blk = net.core.blocks[0]
    tag = f"[{B},{E},{L}]"
    print(f"--- DiffusionTransformer({', '.join(f'{k}={v}' for k, v in kw.items()) or 'defaults'}) on {list(shape)}: "
          f"{len(net.core.blocks)} blocks, MLP width {blk.nmlp}, head width {E // net.nheads}, tokens {tag}", flush=True)
    img, t = torch.randn(shape, device=dev), torch.rand(B, device=dev)
    x, y, a = (torch.randn(B, E, L, device=dev) for _ in range(3))
    h = torch.randn(B, blk.nmlp, L, device=dev)
    tab = torch.randn(40, 6 * E, device=dev)
    am = torch.zeros(B, dtype=torch.int32, device=dev)
    n = 4 * x.numel()
    report(f"token_layernorm + adaLN (+ amax) {tag}", lambda: ops.token_layernorm(x, blk.norm1.weight, blk.norm1.bias, tab, 0, 1, 7,
                                                                                   out=a, out_amax=am), 2 * n)
    report(f"token_gate in place {tag}", lambda: ops.token_gate(x, y, tab, 2, 7, out=x), 3 * n)
    report(f"silu_amax in place [{B},{blk.nmlp},{L}]", lambda: ops.silu_amax(h, out=h, out_amax=am), 8 * h.numel())
    report(f"patch_embed {list(shape)} -> {tag}", lambda: ops.patch_embed(img, net.embed.weight, net.embed.bias, p, out=a),
           4 * img.numel() + n)
    out = torch.empty_like(img)
    report(f"patch_unembed {tag} -> {list(shape)}", lambda: ops.patch_unembed(x, net.unembed.weight, net.unembed.bias, p, shape, out=out),
           4 * img.numel() + n)
    # the existing kernels one block spends its time in
    pk = net.packed_weights()
    mh = blk.attn.attn
    g = (B, E, H // p, W // p)
    qkv = torch.empty(B, 3 * E, H // p, W // p, device=dev)
    s1, s2, s3 = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(2 * B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    ops.absmax_rows(a, out=s1)
    split = 2 * E if E % 32 == 0 else 0
    report(f"in_proj 1x1 {E} -> {3 * E}", lambda: ops.conv(a.view(g), pk[id(mh.in_proj_weight)], bias=mh.in_proj_bias, out=qkv, in_amax=s1,
                                                          out_amax=s2 if split else None, amax_split=split))
    if not split:
        ops.absmax_rows(qkv[:, :2 * E], out=s2[:B])
        ops.absmax_rows(qkv[:, 2 * E:], out=s2[B:])
    nws = ops.attention_workspace_floats(B, E, L, "fp16x3", heads=mh.num_heads)
    aws = torch.empty(nws, device=dev) if nws else None
    report(f"attention heads={mh.num_heads} width {E // mh.num_heads}", lambda: ops.attention(qkv.view(B, 3 * E, L), E, out=y, precision="fp16x3",
                                                                                           workspace=aws, heads=mh.num_heads, in_amax=s2, out_amax=s3))
    report(f"out_proj 1x1 {E} -> {E}", lambda: ops.conv(y.view(g), pk[id(mh.out_proj.weight)], bias=mh.out_proj.bias, out=a.view(g), in_amax=s3))
    report(f"mlp.0 1x1 {E} -> {blk.nmlp}", lambda: ops.conv(a.view(g), pk[id(blk.mlp[0].weight)], bias=blk.mlp[0].bias,
                                                            out=h.view(B, blk.nmlp, H // p, W // p), in_amax=s1))
    ops.absmax_rows(h, out=s3)
    report(f"mlp.2 1x1 {blk.nmlp} -> {E}", lambda: ops.conv(h.view(B, blk.nmlp, H // p, W // p), pk[id(blk.mlp[2].weight)], bias=blk.mlp[2].bias,
                                                            out=a.view(g), in_amax=s3))
    with torch.no_grad():
        us = report(f"one evaluation, eager (forward_unguarded) {list(shape)}", lambda: net.forward_unguarded(img, t))
    print(f"    = {us / 1e3:.3f} ms, {B / us * 1e6:.0f} evaluations of one sample per second", flush=True)
    del net
    torch.cuda.empty_cache()


case(dict(nembed=256, nheads=4, nblocks=6, patch_size=4), (16, 1, 128, 128))
case(dict(), (64, 1, 128, 128))
