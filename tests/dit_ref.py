"""The reference's DiffusionTransformer restated as one plain torch function of a state_dict, in the dtype of the state_dict
(fp32 or fp64): what the GPU tests compare against at sizes that have no golden.  Own code; the lines it restates are cited from
diffsci/models/nets/difftransformer.py.  tests/test_dit.py pins it against the goldens the reference itself produced
(tests/golden/dit_*.npz): fp64 within 1e-13 rel-L2, fp32 within the reference's own fp32-vs-fp64 distance.

The number of blocks and every width are read off the state_dict; only what it does not hold is an argument (nheads, patch_size)."""
import math

import torch
import torch.nn.functional as F


def layer_norm(x, w, b, eps=1e-5):
    """torch.nn.LayerNorm over the last axis: biased variance, affine."""
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def linear(x, sd, name):
    return F.linear(x, sd[name + ".weight"], sd[name + ".bias"])


silu = F.silu


def patchify(x, p):
    """'b c (h p1) (w p2) -> b (h w) (c p1 p2)' (difftransformer.py:9-13, 77-80)."""
    B, C, H, W = x.shape
    x = x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B, (H // p) * (W // p), C * p * p)


def unpatchify(x, p, C, H, W):
    """'b (h w) (c p1 p2) -> b c (h p1) (w p2)' (difftransformer.py:16-20, 86-94)."""
    B = x.shape[0]
    x = x.reshape(B, H // p, W // p, C, p, p).permute(0, 3, 1, 4, 2, 5)
    return x.reshape(B, C, H, W)


def self_attention(x, sd, prefix, nheads):
    """nn.MultiheadAttention(E, nheads, batch_first=True)(x, x, x)[0] (difftransformer.py:131-136) in the operation order of the
    path torch takes for it in eval mode without autograd (its native multi-head attention): the in-projection as a matrix product,
    then the bias, then q times 1/sqrt(d) -- on the host that wrote the fixtures this makes the fp32 form bit-identical to the
    reference's fp32 output, not merely as close to fp64 as it is."""
    B, L, E = x.shape
    d = E // nheads
    qkv = x @ sd[prefix + ".in_proj_weight"].T + sd[prefix + ".in_proj_bias"]
    q, k, v = (t.reshape(B, L, nheads, d).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    a = torch.softmax((q * (1.0 / math.sqrt(d))) @ k.transpose(-1, -2), dim=-1) @ v
    return linear(a.transpose(1, 2).reshape(B, L, E), sd, prefix + ".out_proj")


def time_embedding(sd, t):
    """resnet_time_block(time_embed(t)) (difftransformer.py:230, 53-67; GaussianFourierProjection, commonlayers.py:185-190)."""
    proj = 2 * math.pi * t[..., None] * sd["time_embed.W"]
    g = torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)
    h = silu(linear(g, sd, "resnet_time_block.net.0"))
    h = silu(linear(h, sd, "resnet_time_block.net.2"))
    return g + linear(h, sd, "resnet_time_block.net.4")


def dit_block(x, te, sd, prefix, nheads):
    """DiTBlock.forward (difftransformer.py:162-175)."""
    mod = linear(silu(te), sd, prefix + ".adaln_modulation.1")
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = (m.unsqueeze(1) for m in mod.chunk(6, dim=1))
    a = layer_norm(x, sd[prefix + ".norm1.weight"], sd[prefix + ".norm1.bias"]) * (1 + scale_msa) + shift_msa
    x = x + gate_msa * self_attention(a, sd, prefix + ".attn.attn", nheads)
    a = layer_norm(x, sd[prefix + ".norm2.weight"], sd[prefix + ".norm2.bias"]) * (1 + scale_mlp) + shift_mlp
    return x + gate_mlp * linear(silu(linear(a, sd, prefix + ".mlp.0")), sd, prefix + ".mlp.2")


def dit_forward(sd, x, t, nheads, patch_size):
    """DiffusionTransformer.forward (difftransformer.py:226-236).  sd: the state_dict (its dtype is the arithmetic's), x [B, c, H, W],
    t [B].  The positional encoding is not applied: the reference constructs it and never calls it."""
    dtype = sd["embed.weight"].dtype
    x, t = x.to(dtype), t.to(dtype)
    B, C, H, W = x.shape
    nblocks = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("core.blocks."))
    te = time_embedding(sd, t)
    h = linear(patchify(x, patch_size), sd, "embed")
    for i in range(nblocks):
        h = dit_block(h, te, sd, f"core.blocks.{i}", nheads)
    return unpatchify(linear(h, sd, "unembed"), patch_size, C, H, W)


def load_golden(tag):
    """tests/golden/dit_<tag>.npz merged with its weight files `_w1`, `_w2`, ... -> (values, state_dict, constructor kwargs)."""
    import glob
    import json
    import os

    from tests.golden_util import GOLDEN_DIR, load
    vals, sd = load("dit_" + tag)
    parts = sorted(glob.glob(os.path.join(GOLDEN_DIR, f"dit_{tag}_w*.npz")))
    assert parts, "weight files missing"
    for path in parts:
        sd.update(load(os.path.basename(path)[:-4])[1])
    return vals, sd, json.loads(vals["kwargs"])
