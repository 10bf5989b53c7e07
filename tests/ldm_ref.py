"""The reference's LDM AutoencoderKL decoder restated as plain torch functions of a state_dict, in the dtype of the state_dict
(fp32 or fp64), for fields (Conv2d weights) and volumes (Conv3d weights) alike: what the GPU tests compare against at sizes that
have no golden.  Own code; it follows diffsci/models/nets/autoencoderldm2d.py / autoencoderldm3d.py operation by operation (the
lines are cited).  tests/test_ldm_decoder.py pins it against the fixtures the reference itself produced (tests/golden/ldm_*.npz).

The architecture is read off the state_dict (which blocks exist, their widths, where attention and upsampling convolutions sit);
only what it does not hold is an argument (give_pre_end, tanh_out)."""
import json

import torch
import torch.nn.functional as F

from tests import golden_util


def conv(x, sd, name, padding=0):
    w = sd[name + ".weight"]
    return (F.conv3d if w.dim() == 5 else F.conv2d)(x, w, sd[name + ".bias"], stride=1, padding=padding)


def normalize(x, sd, name):
    """Normalize(): GroupNorm(32, C, eps=1e-6, affine) (autoencoderldm2d.py:17-21)."""
    return F.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], eps=1e-6)


def nonlinearity(x):
    """swish (autoencoderldm2d.py:24-26)."""
    return x * torch.sigmoid(x)


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def resnet_block(x, sd):
    """ResnetBlock.forward with temb=None, dropout 0 (autoencoderldm2d.py:68-88)."""
    h = conv(nonlinearity(normalize(x, sd, "norm1")), sd, "conv1", 1)
    h = conv(nonlinearity(normalize(h, sd, "norm2")), sd, "conv2", 1)
    if "conv_shortcut.weight" in sd:
        x = conv(x, sd, "conv_shortcut", 1)
    elif "nin_shortcut.weight" in sd:
        x = conv(x, sd, "nin_shortcut")
    return x + h


def attn_block(x, sd):
    """AttnBlock.forward (autoencoderldm2d.py:150-174; autoencoderldm3d.py:151-176 flattens three axes)."""
    h = normalize(x, sd, "norm")
    q, k, v = conv(h, sd, "q"), conv(h, sd, "k"), conv(h, sd, "v")
    b, c = q.shape[:2]
    q = q.reshape(b, c, -1).permute(0, 2, 1)
    k = k.reshape(b, c, -1)
    w_ = torch.bmm(q, k)
    w_ = w_ * (int(c) ** (-0.5))
    w_ = F.softmax(w_, dim=2)
    v = v.reshape(b, c, -1)
    h = torch.bmm(v, w_.permute(0, 2, 1)).reshape(x.shape)
    return x + conv(h, sd, "proj_out")


def upsample(x, sd):
    """Upsample.forward (autoencoderldm2d.py:199-203): nearest x2, then the convolution when the block has one."""
    x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return conv(x, sd, "conv", 1) if "conv.weight" in sd else x


def decoder(sd, z, give_pre_end=False, tanh_out=False):
    """Decoder.forward (autoencoderldm2d.py:440-474)."""
    z = z.to(sd["conv_in.weight"].dtype)
    h = conv(z, sd, "conv_in", 1)
    h = resnet_block(h, sub(sd, "mid.block_1."))
    if "mid.attn_1.norm.weight" in sd:
        h = attn_block(h, sub(sd, "mid.attn_1."))
    h = resnet_block(h, sub(sd, "mid.block_2."))
    levels = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("up."))
    for lvl in reversed(range(levels)):
        nblocks = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(f"up.{lvl}.block."))
        for i in range(nblocks):
            h = resnet_block(h, sub(sd, f"up.{lvl}.block.{i}."))
            if f"up.{lvl}.attn.{i}.norm.weight" in sd:
                h = attn_block(h, sub(sd, f"up.{lvl}.attn.{i}."))
        if lvl != 0:
            h = upsample(h, sub(sd, f"up.{lvl}.upsample."))
    if give_pre_end:
        return h
    h = conv(nonlinearity(normalize(h, sd, "norm_out")), sd, "conv_out", 1)
    return torch.tanh(h) if tanh_out else h


def autoencoder_decode(sd, z):
    """AutoencoderKL.decode (autoencoderldm2d.py:602-605) over a state_dict with decoder.* and post_quant_conv.* keys."""
    z = z.to(sd["post_quant_conv.weight"].dtype)
    return decoder(sub(sd, "decoder."), conv(z, sd, "post_quant_conv"))


# ---- fixtures (tools/make_ldm_golden.py) ---------------------------------------------------------------------------------------
WEIGHTS_OF = {"a2": "a", "ae": "a"}       # cases that reuse another case's decoder weights


def load_golden(tag):
    """-> (values, state_dict, info): info = the recorded JSON (module "2d" | "3d", ddconfig and Decoder keyword arguments)."""
    vals, sd = golden_util.load("ldm_" + tag)
    src = WEIGHTS_OF.get(tag, tag)
    i = 1
    while True:
        try:
            _, part = golden_util.load(f"ldm_{src}_w{i}")
        except FileNotFoundError:
            break
        for k, v in part.items():
            sd[("decoder." + k) if tag == "ae" else k] = v
        i += 1
    if tag == "ae":
        for k in ("post_quant_conv.weight", "post_quant_conv.bias"):
            sd[k] = vals.pop(k)
    return vals, sd, json.loads(vals["info"])


def module_of(info):
    import importlib
    return importlib.import_module("diffsci_amd.models.nets.autoencoderldm" + info["module"])


def build(info):
    """This package's Decoder for a fixture."""
    mod = module_of(info)
    return mod.Decoder(mod.ddconfig(**info["ddconfig"]), **info["decoder"])
