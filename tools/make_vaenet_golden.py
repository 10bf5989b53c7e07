"""Generate tests/golden/vaenet_{a,a2,b,c}.npz and their weight files (`_w1`, `_w2`, ...): the reference's VAENet
(diffsci/models/nets/vaenet.py) run on the CPU in fp32 and as fp64 copies (imported through oracle/tools/refshim.py; needs the
reference checkout that shim points at).  The fixtures are data only: the state_dict, the inputs, the reference's moments, a
recorded posterior draw (eps and the sampled z), decoder outputs, and -- as JSON strings -- the configuration, the state_dict
key -> shape list and the constructor signatures of the module's classes.

    a   2-D  ch=32 ch_mult=[1,2] num_res_blocks=1 resolution=32 attn_resolutions=[16] z_channels=4 z_dim=3
             x [2,1,32,32] -> moments [2,6,16,16]; z [2,3,16,16] -> [2,1,32,32]
    a2  case a's weights, encoder only, x [1,1,15,19]: odd planes into the Downsample, a 7 x 9 latent (L = 63: the attention
             kernel's generic path)
    b   2-D  ch=16 num_groups=8 ch_mult=[1,2,4] num_res_blocks=2 in_channels=2 out_channels=3 resamp_with_conv=False
             memory_efficient_variant=True input_bias=False output_bias=False tanh_out=True has_mid_attn=False
             use_flash_attention=False resolution=32; x [1,2,24,40] -> a 6 x 10 latent
    c   3-D  ch=32 ch_mult=[1,2] num_res_blocks=1 resolution=16; x [1,1,16,16,16]; encoder only on [1,1,7,10,12]

Norm affines and every bias are perturbed (+ 0.25 randn).

    python tools/make_vaenet_golden.py"""
import contextlib
import inspect
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
from diffsci.models.nets import vaenet as R  # noqa: E402

torch.set_num_threads(8)
PART_BYTES = 900 << 10
CASES = {
    "a": (dict(dimension=2, ch=32, ch_mult=[1, 2], num_res_blocks=1, resolution=32, attn_resolutions=[16], z_channels=4, z_dim=3),
          (2, 1, 32, 32), 510),
    "b": (dict(dimension=2, ch=16, num_groups=8, ch_mult=[1, 2, 4], num_res_blocks=2, in_channels=2, out_channels=3,
               resamp_with_conv=False, memory_efficient_variant=True, input_bias=False, output_bias=False, tanh_out=True,
               has_mid_attn=False, use_flash_attention=False, resolution=32), (1, 2, 24, 40), 512),
    "c": (dict(dimension=3, ch=32, ch_mult=[1, 2], num_res_blocks=1, resolution=16), (1, 1, 16, 16, 16), 514),
}
EXTRA_X = {"a": ("a2", (1, 1, 15, 19)), "c": ("c2", (1, 1, 7, 10, 12))}
CLASSES = ("VAENetConfig", "PatchedConv", "ResnetBlock", "AttnBlock", "Upsample", "Downsample", "VAEEncoder", "VAEDecoder", "VAENet")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def signature(cls):
    return [[n, p.kind.name, "<required>" if p.default is inspect.Parameter.empty else repr(p.default)]
            for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]


def keys(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


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


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def encode_pair(net, net64, x, seed):
    """moments in both precisions, and one recorded draw: the reference's own encode(x) under `seed`, the eps it drew (the same
    generator call replayed), and the fp64 sample from the fp64 moments with that eps."""
    with torch.inference_mode():
        m32, m64 = net.encode(x, sample=False), net64.encode(x.double(), sample=False)
        torch.manual_seed(seed)
        z32 = net.encode(x)
        torch.manual_seed(seed)
        eps = torch.randn_like(m32.chunk(2, dim=1)[0])
        mean, logvar = m64.chunk(2, dim=1)
        z64 = mean + torch.exp(0.5 * logvar) * eps.double()
        mean, logvar = m32.chunk(2, dim=1)
        assert torch.equal(z32, mean + torch.exp(0.5 * logvar) * eps)
    return dict(x=x, moments_f32=m32, moments_f64=m64, eps=eps, z_f32=z32, z_f64=z64)


def main():
    for tag, (cfg_kw, shape, seed) in CASES.items():
        torch.manual_seed(seed)
        net = quiet(R.VAENet, R.VAENetConfig(**cfg_kw)).eval()
        perturb(net)
        sd = net.state_dict()
        net64 = quiet(R.VAENet, R.VAENetConfig(**cfg_kw)).double().eval()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        torch.manual_seed(seed + 1)
        x = torch.randn(*shape)
        info = dict(config=cfg_kw)
        arrs = {"sd/" + k: v for k, v in sd.items()}
        arrs.update(info=json.dumps(info), keys=json.dumps(keys(net)),
                    signatures=json.dumps({c: signature(getattr(R, c)) for c in CLASSES}),
                    description=json.dumps(net.export_description()))
        arrs.update(encode_pair(net, net64, x, seed + 2))
        zin = torch.randn(shape[0], cfg_kw.get("z_dim", 4), *arrs["moments_f32"].shape[2:])
        with torch.inference_mode():
            arrs.update(zin=zin, dec_f32=net.decode(zin), dec_f64=net64.decode(zin.double()))
        nparts, size = save("vaenet_" + tag, arrs)
        print(f"vaenet_{tag}: {nparts} files, {size / 1024:.1f} KiB; {len(sd)} entries; moments {tuple(arrs['moments_f32'].shape)} "
              f"fp32 vs fp64 {rel(arrs['moments_f32'], arrs['moments_f64']):.3e}; decode {tuple(arrs['dec_f32'].shape)} "
              f"{rel(arrs['dec_f32'], arrs['dec_f64']):.3e}", flush=True)
        if tag in EXTRA_X:
            tag2, shape2 = EXTRA_X[tag]
            extra = encode_pair(net, net64, torch.randn(*shape2), seed + 3)
            extra["info"] = json.dumps(info)
            save("vaenet_" + tag2, extra)
            print(f"vaenet_{tag2}: moments {tuple(extra['moments_f32'].shape)} fp32 vs fp64 "
                  f"{rel(extra['moments_f32'], extra['moments_f64']):.3e}", flush=True)


if __name__ == "__main__":
    main()
