"""The reference's ConVit restated as plain torch functions of a state_dict, in the dtype of the state_dict (fp32 or fp64): what
the GPU tests compare against at sizes that have no golden.  Own code; the lines it restates are cited from
diffsci/models/nets/convit.py.  tests/test_convit.py pins it against the goldens the reference itself produced
(tests/golden/convit_*.npz): fp64 within 1e-12 rel-L2, fp32 within the reference's own fp32-vs-fp64 distance.

The number of blocks, every width and every kernel size are read off the state_dict; only what it does not hold is an argument
(num_heads, attn_compression_factor, relative_positioning).  The conditional embedding of the fixtures is a Linear whose weights
are state_dict entries (`conditional_embedding.weight` / `.bias`)."""
import math

import torch
import torch.nn.functional as F


def channel_rmsnorm(x, w):
    """ChannelRMSNorm.forward (convit.py:236-243)."""
    eps = torch.finfo(x.dtype).eps
    norm = torch.sqrt(torch.mean(x ** 2, dim=1, keepdim=True) + eps)
    return x / norm * w.view(1, -1, *([1] * (x.dim() - 2)))


def rope(x, angles, relative):
    """LearnedRoPE.forward (convit.py:369-388) on x [n, *positions, d]."""
    dims = x.shape[1:-1]
    normalizers = (torch.ones(len(dims)) if not relative else torch.tensor(dims)).to(x)
    positions = torch.stack(torch.meshgrid([torch.arange(d).to(x) / n for d, n in zip(dims, normalizers)], indexing="ij"), dim=-1)
    ang = (positions.unsqueeze(-1) * angles).sum(dim=-2)                 # [*positions, d/2]
    x = x.reshape(*x.shape[:-1], x.shape[-1] // 2, 2)
    x = torch.stack([x[..., 0] * torch.cos(ang) - x[..., 1] * torch.sin(ang),
                     x[..., 0] * torch.sin(ang) + x[..., 1] * torch.cos(ang)], dim=-1)
    return x.reshape(*x.shape[:-2], -1)


def attention(x, sd, prefix, relative):
    """MultiheadAttention.forward, softmax form (convit.py:457-533), on x [B, H, W, E]."""
    B, Hh, Ww, _ = x.shape
    q, k, v = (torch.einsum("abcd,def->abcef", x, sd[f"{prefix}.{n}_proj_tensor"]) for n in "qkv")
    dv, h = q.shape[-2:]

    def roped(t):
        t = t.permute(0, 4, 1, 2, 3).reshape(B * h, Hh, Ww, dv)           # 'b m0 m1 dv h -> (b h) m0 m1 dv'
        t = rope(t, sd[f"{prefix}.rope_layer.angles"], relative)
        return t.reshape(B, h, Hh, Ww, dv).permute(0, 2, 3, 4, 1)         # '(b h) m0 m1 dv -> b m0 m1 dv h'

    def heads_first(t):
        return t.permute(0, 4, 1, 2, 3).reshape(B, h, Hh * Ww, dv)        # 'b m0 m1 dv h -> b h (m0 m1) dv'

    q, k = roped(q), roped(k)
    o = F.scaled_dot_product_attention(heads_first(q), heads_first(k), heads_first(v), attn_mask=None, is_causal=False,
                                       scale=1.0 / sd[f"{prefix}.scale"])
    o = o.reshape(B, h, Hh, Ww, dv).permute(0, 2, 3, 4, 1)                # 'b h (m0 m1) dv -> b m0 m1 dv h'
    # the letters in einops' order of appearance: torch.einsum contracts (dv, h) in letter order, and the fp32 sum follows it
    return torch.einsum("abcde,fde->abcf", o, sd[f"{prefix}.out_proj_tensor"])


def conv(x, sd, name, groups=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding="same", groups=groups)


def embedding_row(te, sd, prefix):
    """SwiGLU(final_rms=True).forward (convit.py:345-348): torch.nn.RMSNorm(E), eps=None."""
    def lin(n):
        return F.linear(te, sd[f"{prefix}.{n}.weight"], sd[f"{prefix}.{n}.bias"])
    h = F.linear(F.silu(lin("linear_in")) * lin("linear_gate"), sd[prefix + ".linear_out.weight"], sd[prefix + ".linear_out.bias"])
    return F.rms_norm(h, (h.shape[-1],), sd[prefix + ".rms.weight"], None)


def block(x, ye, sd, prefix, factor, relative):
    """ConVitBlock.forward (convit.py:605-636)."""
    y = 0.0 if ye is None else embedding_row(ye, sd, prefix + ".embedding_projection").reshape(ye.shape[0], -1, 1, 1)
    x0 = x.clone()
    x = channel_rmsnorm(x, sd[prefix + ".norm_1.weight"]) + y
    x = F.avg_pool2d(x, factor, factor, 0)
    x = attention(x.permute(0, 2, 3, 1), sd, prefix + ".attention", relative).permute(0, 3, 1, 2)
    x = F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=False)
    E = x.shape[1]
    x_conv = conv(F.silu(conv(x, sd, prefix + ".depthwise_conv", groups=E)), sd, prefix + ".pointwise_conv")
    s = torch.sigmoid(sd[prefix + ".fusion_weight"])
    x = (1 - s) * x + s * x_conv
    x = x + x0
    x0 = x.clone()
    x = channel_rmsnorm(x, sd[prefix + ".norm_2.weight"]) + y
    x = conv(F.silu(conv(x, sd, prefix + ".ffn.linear_in")) * conv(x, sd, prefix + ".ffn.linear_gate"), sd, prefix + ".ffn.linear_out")
    return x + x0


def convit_forward(sd, x, t=None, y=None, *, attn_compression_factor=2, relative_positioning=False):
    """ConVit.forward (convit.py:721-735).  sd: the state_dict (its dtype is the arithmetic's); x [B, C, H, W], t [B] or None,
    y [B, 1] or None (embedded by the Linear stored as `conditional_embedding.*`).  The number of heads is the last extent of the
    projection tensors."""
    dtype = sd["convin.weight"].dtype
    x = x.to(dtype)
    te = 0.0
    if t is not None:
        proj = 2 * math.pi * t.to(dtype)[..., None] * sd["time_embedding.W"]           # GaussianFourierProjection, commonlayers.py:185-190
        te = torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)
    ye = F.linear(y.to(dtype), sd["conditional_embedding.weight"], sd["conditional_embedding.bias"]) if y is not None else 0.0
    emb = te + ye
    if not torch.is_tensor(emb):
        emb = None
    nblocks = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    h = conv(x, sd, "convin")
    for i in range(nblocks):
        h = block(h, emb, sd, f"blocks.{i}", attn_compression_factor, relative_positioning)
    return conv(channel_rmsnorm(h, sd["normout.weight"]), sd, "convout")


def load_golden(tag):
    """tests/golden/convit_<tag>.npz merged with its weight files `_w1`, `_w2`, ... -> (values, state_dict, config kwargs)."""
    import glob
    import json
    import os

    from tests.golden_util import GOLDEN_DIR, load
    vals, sd = load("convit_" + tag)
    parts = sorted(glob.glob(os.path.join(GOLDEN_DIR, f"convit_{tag}_w*.npz")))
    assert parts, "weight files missing"
    for path in parts:
        sd.update(load(os.path.basename(path)[:-4])[1])
    for k in sorted({k.split("#")[0] for k in sd if "#" in k}):         # a tensor too large for one file: pieces along its first axis
        n = sum(1 for q in sd if q.startswith(k + "#"))
        sd[k] = torch.cat([sd.pop(f"{k}#{j}") for j in range(n)], dim=0)
    order = [k for k, _ in json.loads(vals["keys"])]
    assert sorted(order) == sorted(sd)
    return vals, {k: sd[k] for k in order}, json.loads(vals["kwargs"])
