"""Generate tests/golden/ldm_{a,a2,b,c,ae}.npz and their weight files (`_w1`, `_w2`, ...): the reference's LDM AutoencoderKL
decoders (autoencoderldm2d.py / autoencoderldm3d.py) run on the CPU in fp32 and as fp64 copies (imported through
oracle/tools/refshim.py; needs the reference checkout that shim points at).  The fixtures are data only: the state_dict, the
inputs, the reference's outputs, and -- as JSON strings -- the constructor signatures and state_dict key -> shape lists of
ddconfig, Decoder, ResnetBlock, AttnBlock and AutoencoderKL of both modules.

    a   2-D  ch=32 ch_mult=[1,2] num_res_blocks=1 attn_resolutions=[16]            z [2,4,16,16] -> [2,1,32,32]
             groups of 1 and 2 channels; mid and level attention at L = 256; nin_shortcut (64 -> 32)
    a2  case a's weights on a 6 x 10 latent                                        L = 60: the attention kernel's generic path
    b   2-D  ch=64 ch_mult=[1,2,2] num_res_blocks=2 z_channels=8 out_ch=3 has_mid_attn=False tanh_out=True
             z [1,8,6,10] -> 24 x 40: non-square, planes that are no multiples of 4 at the bottom; groups of 2 and 4
    c   3-D  ch=32 ch_mult=[1,2] num_res_blocks=1, mid attention                   z [1,4,8,8,8] -> 16^3, L = 512
    ae  AutoencoderKL.decode over case a's decoder with embed_dim = 3 != z_channels = 4       z [2,3,16,16]

Norm affines and every bias are perturbed (+ 0.25 randn) so that no term is exercised at its initial value only.

    python tools/make_ldm_golden.py"""
import contextlib
import inspect
import io
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
from diffsci.models.nets import autoencoderldm2d as R2  # noqa: E402
from diffsci.models.nets import autoencoderldm3d as R3  # noqa: E402

torch.set_num_threads(8)
PART_BYTES = 900 << 10
MODULES = {"2d": R2, "3d": R3}
CASES = {
    "a": ("2d", dict(ch=32, ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16], resolution=32), {}, (2, 4, 16, 16), 410),
    "b": ("2d", dict(ch=64, ch_mult=[1, 2, 2], num_res_blocks=2, z_channels=8, out_ch=3, has_mid_attn=False, resolution=32),
          dict(tanh_out=True), (1, 8, 6, 10), 412),
    "c": ("3d", dict(ch=32, ch_mult=[1, 2], num_res_blocks=1, resolution=16), {}, (1, 4, 8, 8, 8), 414),
}
CLASSES = ("ddconfig", "Decoder", "ResnetBlock", "AttnBlock", "AutoencoderKL")


def quiet(fn, *a, **k):
    """The reference prints while it builds its modules."""
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def signature(cls):
    return [[n, p.kind.name, "<required>" if p.default is inspect.Parameter.empty else repr(p.default)]
            for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]


def keys(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def no_loss():
    """A lossconfig whose loss has no parameters: the reference's default one needs torchvision's pretrained LPIPS network."""
    return types.SimpleNamespace(target=lambda *a, **k: torch.nn.Identity(), disc_start=0, kl_weight=0.0, disc_weight=0.0)


def surface(R, cfg_kw):
    """Signatures and state_dict keys of one reference module's classes, at small sizes."""
    vae = quiet(R.AutoencoderKL, R.ddconfig(**cfg_kw), no_loss())
    return dict(
        signatures={c: signature(getattr(R, c)) for c in CLASSES},
        keys=dict(ResnetBlock=keys(quiet(R.ResnetBlock, in_channels=32, out_channels=64, dropout=0.0, temb_channels=0)),
                  ResnetBlockConvShortcut=keys(quiet(R.ResnetBlock, in_channels=32, out_channels=64, conv_shortcut=True, dropout=0.0,
                                                     temb_channels=0)),
                  ResnetBlockTemb=keys(quiet(R.ResnetBlock, in_channels=32, dropout=0.0)),
                  AttnBlock=keys(quiet(R.AttnBlock, 64)), Upsample=keys(quiet(R.Upsample, 32, True)), AutoencoderKL=keys(vae)),
        z_shape=list(vae.decoder.z_shape))


def perturb(module):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                v.add_(0.25 * torch.randn_like(v))


def save(name, arrs):
    """No committed file above 1 MiB: the state_dict goes to `<name>_w<i>.npz` (keys "sd/..."), the rest stays in `<name>.npz`."""
    gold = os.path.join(ROOT, "tests", "golden")
    parts, room = [{k: v for k, v in arrs.items() if not k.startswith("sd/")}], [0]
    for k in sorted((k for k in arrs if k.startswith("sd/")), key=lambda k: -arrs[k].numel()):
        n = arrs[k].numel() * 4
        i = next((i for i in range(1, len(parts)) if room[i] + n <= PART_BYTES), None)
        if i is None:
            parts.append({})
            room.append(0)
            i = len(parts) - 1
        parts[i][k] = arrs[k]
        room[i] += n
    size = 0
    for i, part in enumerate(parts):
        path = os.path.join(gold, name + (f"_w{i}" if i else "") + ".npz")
        np.savez_compressed(path, **{k: (np.asarray(v.detach().cpu().numpy()) if torch.is_tensor(v) else np.asarray(v))
                                     for k, v in part.items()})
        assert os.path.getsize(path) < 1 << 20, path
        size += os.path.getsize(path)
    return len(parts), size


def run_pair(net, net64, z):
    with torch.inference_mode():
        o32, o64 = net(z), net64(z.double())
    assert o64.dtype == torch.float64
    return o32, o64, float((o32.double() - o64).norm() / o64.norm())


def main():
    for tag, (mod, cfg_kw, dec_kw, shape, seed) in CASES.items():
        R = MODULES[mod]
        torch.manual_seed(seed)
        net = quiet(R.Decoder, R.ddconfig(**cfg_kw), **dec_kw).eval()
        perturb(net)
        sd = net.state_dict()
        net64 = quiet(R.Decoder, R.ddconfig(**cfg_kw), **dec_kw).double().eval()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        torch.manual_seed(seed + 1)
        z = torch.randn(*shape)
        info = dict(module=mod, ddconfig=cfg_kw, decoder=dec_kw)
        arrs = {"sd/" + k: v for k, v in sd.items()}
        arrs.update(z=z, info=json.dumps(info), keys=json.dumps(keys(net)), surface=json.dumps(surface(R, cfg_kw)))
        arrs["out_f32"], arrs["out_f64"], rel = run_pair(net, net64, z)
        nparts, size = save("ldm_" + tag, arrs)
        print(f"ldm_{tag}: {nparts} files, {size / 1024:.1f} KiB; {len(sd)} state_dict entries; out {tuple(arrs['out_f32'].shape)}; "
              f"fp32 vs fp64 {rel:.3e}", flush=True)
        if tag != "a":
            continue
        z2 = torch.randn(2, 4, 6, 10)
        o32, o64, rel = run_pair(net, net64, z2)
        save("ldm_a2", dict(z=z2, info=json.dumps(info), out_f32=o32, out_f64=o64))
        print(f"ldm_a2: out {tuple(o32.shape)}; fp32 vs fp64 {rel:.3e}", flush=True)
        vae = quiet(R.AutoencoderKL, R.ddconfig(**cfg_kw), no_loss(), embed_dim=3).eval()
        vae.decoder.load_state_dict(sd)
        perturb(vae.post_quant_conv)
        vae64 = quiet(R.AutoencoderKL, R.ddconfig(**cfg_kw), no_loss(), embed_dim=3).double().eval()
        vae64.load_state_dict({k: v.double() for k, v in vae.state_dict().items()})
        z3 = torch.randn(2, 3, 16, 16)
        with torch.inference_mode():
            o32, o64 = vae.decode(z3), vae64.decode(z3.double())
        rel = float((o32.double() - o64).norm() / o64.norm())
        save("ldm_ae", {"z": z3, "info": json.dumps(dict(info, embed_dim=3)), "out_f32": o32, "out_f64": o64,
                        "post_quant_conv.weight": vae.post_quant_conv.weight, "post_quant_conv.bias": vae.post_quant_conv.bias})
        print(f"ldm_ae: out {tuple(o32.shape)}; fp32 vs fp64 {rel:.3e}", flush=True)


if __name__ == "__main__":
    main()
