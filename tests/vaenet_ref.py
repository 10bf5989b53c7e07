"""The reference's VAENet (diffsci/models/nets/vaenet.py) restated as plain torch functions of a state_dict, in the dtype of the
state_dict (fp32 or fp64), for fields and volumes alike: what the GPU tests compare against at sizes and options that have no
golden.  Own code, in the manner of tests/ldm_ref.py (whose swish it shares); the reference's lines are cited.
tests/test_vaenet.py pins it against the fixtures the reference itself produced (tests/golden/vaenet_*.npz).

The architecture is read off the state_dict (which blocks exist, their widths, where attention and resampling convolutions sit);
what it does not hold is an argument: num_groups, tanh_out, the attention's formulation (use_flash_attention), and whether a level resamples without a convolution (the
`levels` count is read off the keys, the resampling happens between them)."""
import json

import torch
import torch.nn.functional as F

from tests import golden_util
from tests.ldm_ref import nonlinearity, sub


def pconv(x, sd, name):
    """PatchedConv.forward without patching (vaenet.py:236-241): pad k//2 explicitly, then the child convolution."""
    w = sd[name + ".conv.weight"]
    p = w.shape[-1] // 2
    x = F.pad(x, [p] * 2 * (w.dim() - 2))
    return (F.conv3d if w.dim() == 5 else F.conv2d)(x, w, sd.get(name + ".conv.bias"))


def norm(x, sd, name, G):
    """get_norm (vaenet.py:253-258)."""
    return F.group_norm(x, G, sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)


def resnet_block(x, sd, G=32):
    """ResnetBlock.forward with temb=None, dropout 0 (vaenet.py:302-325)."""
    h = pconv(nonlinearity(norm(x, sd, "norm1", G)), sd, "conv1")
    h = pconv(nonlinearity(norm(h, sd, "norm2", G)), sd, "conv2")
    if "conv_shortcut.conv.weight" in sd:
        x = pconv(x, sd, "conv_shortcut")
    elif "nin_shortcut.conv.weight" in sd:
        x = pconv(x, sd, "nin_shortcut")
    return x + h


def attn_block(x, sd, G=32, flash=True):
    """AttnBlock.forward (vaenet.py:438-453): single-head softmax(q^T k * C**-0.5) v over the flattened positions, through
    scaled_dot_product_attention (use_flash_attention, :483-516) or the two bmm (:518-537)."""
    h = norm(x, sd, "norm", G)
    q, k, v = (pconv(h, sd, n).reshape(x.shape[0], x.shape[1], -1) for n in "qkv")
    b, c, _ = q.shape
    if flash:
        h = F.scaled_dot_product_attention(q.permute(0, 2, 1)[:, None], k.permute(0, 2, 1)[:, None], v.permute(0, 2, 1)[:, None],
                                           attn_mask=None, dropout_p=0.0, is_causal=False, scale=c ** -0.5)
        h = h[:, 0].permute(0, 2, 1)
    else:
        w_ = torch.bmm(q.permute(0, 2, 1), k) * (c ** -0.5)
        w_ = F.softmax(w_, dim=2)
        h = torch.bmm(v, w_.permute(0, 2, 1))
    return x + pconv(h.reshape(x.shape), sd, "proj_out")


def upsample(x, sd):
    """Upsample.forward (vaenet.py:633-644)."""
    x = F.interpolate(x, scale_factor=2.0, mode="area")
    return pconv(x, sd, "conv") if "conv.conv.weight" in sd else x


def downsample(x, sd):
    """Downsample.forward (vaenet.py:662-682): pad (0, 1) per axis + stride-2 convolution, or average pooling."""
    d = x.dim() - 2
    if "conv.weight" in sd:
        x = F.pad(x, (0, 1) * d, mode="constant", value=0)
        return (F.conv3d if d == 3 else F.conv2d)(x, sd["conv.weight"], sd["conv.bias"], stride=2)
    return (F.avg_pool3d if d == 3 else F.avg_pool2d)(x, kernel_size=2, stride=2)


def _levels(sd, stem):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith(stem + "."))


def _blocks(sd, stem, lvl):
    return 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(f"{stem}.{lvl}.block."))


def encoder(sd, x, G=32, flash=True):
    """VAEEncoder.forward (vaenet.py:818-876) -> moments."""
    x = x.to(sd["conv_in.conv.weight"].dtype)
    h = pconv(x, sd, "conv_in")
    levels = _levels(sd, "down")
    for lvl in range(levels):
        for i in range(_blocks(sd, "down", lvl)):
            h = resnet_block(h, sub(sd, f"down.{lvl}.block.{i}."), G)
            if f"down.{lvl}.attn.{i}.norm.weight" in sd:
                h = attn_block(h, sub(sd, f"down.{lvl}.attn.{i}."), G, flash)
        if lvl != levels - 1:
            h = downsample(h, sub(sd, f"down.{lvl}.downsample."))
    h = resnet_block(h, sub(sd, "mid.block_1."), G)
    if "mid.attn_1.norm.weight" in sd:
        h = attn_block(h, sub(sd, "mid.attn_1."), G, flash)
    h = resnet_block(h, sub(sd, "mid.block_2."), G)
    h = pconv(nonlinearity(norm(h, sd, "norm_out", G)), sd, "conv_out")
    return pconv(h, sd, "quant_conv")


def decoder(sd, z, G=32, tanh_out=False, flash=True):
    """VAEDecoder.forward (vaenet.py:1083-1140)."""
    z = z.to(sd["conv_in.conv.weight"].dtype)
    h = pconv(pconv(z, sd, "post_quant_conv"), sd, "conv_in")
    h = resnet_block(h, sub(sd, "mid.block_1."), G)
    if "mid.attn_1.norm.weight" in sd:
        h = attn_block(h, sub(sd, "mid.attn_1."), G, flash)
    h = resnet_block(h, sub(sd, "mid.block_2."), G)
    for lvl in reversed(range(_levels(sd, "up"))):
        for i in range(_blocks(sd, "up", lvl)):
            h = resnet_block(h, sub(sd, f"up.{lvl}.block.{i}."), G)
            if f"up.{lvl}.attn.{i}.norm.weight" in sd:
                h = attn_block(h, sub(sd, f"up.{lvl}.attn.{i}."), G, flash)
        if lvl != 0:
            h = upsample(h, sub(sd, f"up.{lvl}.upsample."))
    h = pconv(nonlinearity(norm(h, sd, "norm_out", G)), sd, "conv_out")
    return torch.tanh(h) if tanh_out else h


def posterior(moments, eps, clamp=None):
    """VAENet.encode's draw (vaenet.py:1244-1248) with the noise given."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    if clamp is not None:
        logvar = torch.clamp(logvar, clamp[0], clamp[1])
    return mean + torch.exp(0.5 * logvar) * eps.to(moments.dtype)


# ---- fixtures (tools/make_vaenet_golden.py) ------------------------------------------------------------------------------------
WEIGHTS_OF = {"a2": "a", "c2": "c"}       # encoder-only cases on another case's weights


def load_golden(tag):
    """-> (values, state_dict of VAENet, info): info = the recorded JSON (config keyword arguments)."""
    vals, sd = golden_util.load("vaenet_" + tag)
    src = WEIGHTS_OF.get(tag, tag)
    i = 1
    while True:
        try:
            _, part = golden_util.load(f"vaenet_{src}_w{i}")
        except FileNotFoundError:
            break
        sd.update(part)
        i += 1
    return vals, sd, json.loads(vals["info"])


def build(info):
    """This package's VAENet for a fixture."""
    from diffsci_amd.models.nets import vaenet
    return vaenet.VAENet(vaenet.VAENetConfig(**info["config"]))
