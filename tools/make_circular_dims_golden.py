"""Generate tests/golden/{pc2_h,pc2_w,pc2_k5,pc3_dh,pc3_w,padm_h,pc2_traj}.npz and their weight files (`_w1`, `_w2`, ...): trained-
as-zero-padded networks of the reference, made periodic along some axes by the reference's own
extra/punetg_converters.convert_conv_to_circular and run on the CPU in fp32 and as fp64 copies (imported through
oracle/tools/refshim.py; needs the reference checkout that shim points at).  Data only.  Every case records the state_dict AFTER
conversion (keys carry '.conv'), the input, t (and y where there is one), the reference's fp32 output, the output of an fp64
copy, count_conv_layers before and after (the reference also counts the inner .conv of a circular layer) and the converted key
list.  Cases that share weights with an earlier case (`pc2_w`, `pc3_w`, `pc2_traj`) name it in `weights_of` instead of
repeating them.

    tag       reference model                                                          circular_dims  input
    pc2_h     PUNetG(PUNetGConfig(model_channels=16))                                  [0]            [2,1,16,32]
    pc2_w     pc2_h's weights                                                          [1]            same
    pc2_k5    PUNetGConfig(model_channels=16, in_out_kernel_size=5)                    [1]            [1,1,16,32]
    pc3_dh    PUNetGConfig(dimension=3, model_channels=16, channel_expansion=[2])      [0,1]          [1,1,8,8,16]
    pc3_w     pc3_dh's weights                                                         [2]            same
    padm_h    ADM(ADMConfig(model_channels=16, time_embed_dim=16, output_embed_dim=32,
                            channel_expansion=[1,2]))                                  [0]            [2,1,16,32]
    pc2_traj  pc2_h's net in KarrasModule(from_edm())                                  [0]            Heun, N = 4: the end state

Norm affines and every bias are perturbed (+ 0.25 randn) so that no term is exercised at its initial value only.

    python tools/make_circular_dims_golden.py"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
import diffsci.models as M  # noqa: E402
from diffsci.extra import punetg_converters as C  # noqa: E402

torch.set_num_threads(8)
PART_BYTES = 900 << 10


def punetg(**kw):
    return lambda: M.nets.PUNetG(M.nets.PUNetGConfig(**kw))


def adm():
    from diffsci.models.nets import adm as A
    return A.ADM(A.ADMConfig(model_channels=16, time_embed_dim=16, output_embed_dim=32, channel_expansion=[1, 2]))


# tag -> (builder, circular_dims, input shape, seed, the case whose unconverted weights it shares)
CASES = {
    "pc2_h": (punetg(model_channels=16), [0], (2, 1, 16, 32), 510, None),
    "pc2_w": (punetg(model_channels=16), [1], (2, 1, 16, 32), 510, "pc2_h"),
    "pc2_k5": (punetg(model_channels=16, in_out_kernel_size=5), [1], (1, 1, 16, 32), 512, None),
    "pc3_dh": (punetg(dimension=3, model_channels=16, channel_expansion=[2]), [0, 1], (1, 1, 8, 8, 16), 514, None),
    "pc3_w": (punetg(dimension=3, model_channels=16, channel_expansion=[2]), [2], (1, 1, 8, 8, 16), 514, "pc3_dh"),
    "padm_h": (adm, [0], (2, 1, 16, 32), 516, None),
}


def quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


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


def converted_pair(build, sd_plain, dims):
    """The reference's network with sd_plain loaded, converted; and its fp64 copy."""
    net = quiet(build).eval()
    net.load_state_dict(sd_plain)
    before = C.count_conv_layers(net)
    conv = C.convert_conv_to_circular(net, dims)
    net64 = quiet(build).eval()
    net64.load_state_dict(sd_plain)
    conv64 = C.convert_conv_to_circular(net64, dims, inplace=True).double()
    return conv.eval(), conv64.eval(), before, C.count_conv_layers(conv)


def main():
    plain = {}
    for tag, (build, dims, shape, seed, share) in CASES.items():
        if share is None:
            torch.manual_seed(seed)
            net = quiet(build).eval()
            perturb(net)
            plain[tag] = {k: v.clone() for k, v in net.state_dict().items()}
        sd_plain = plain[share or tag]
        conv, conv64, before, after = converted_pair(build, sd_plain, dims)
        torch.manual_seed(seed + 1)
        x = torch.randn(*shape)
        t = torch.tensor([0.3, -1.1])[:shape[0]]
        with torch.inference_mode():
            o32, o64 = conv(x, t), conv64(x.double(), t.double())
        assert o64.dtype == torch.float64
        sd = conv.state_dict()
        arrs = dict(x=x, t=t, out_f32=o32, out_f64=o64, circular_dims=json.dumps(dims), keys=json.dumps(list(sd)),
                    count_before=json.dumps(before), count_after=json.dumps(after), weights_of=share or tag)
        if share is None:
            arrs.update({"sd/" + k: v for k, v in sd.items()})
        nparts, size = save(tag, arrs)
        rel = float((o32.double() - o64).norm() / o64.norm())
        print(f"{tag}: {nparts} files, {size / 1024:.1f} KiB; {len(sd)} keys; {before} -> {after}; fp32 vs fp64 {rel:.3e}", flush=True)
        if tag != "pc2_h":
            continue
        # the converted net under the EDM sampler: four Heun steps from given white noise, the end state
        wn = torch.randn(2, 1, 16, 32)
        mod = quiet(M.KarrasModule, conv, M.KarrasModuleConfig.from_edm()).eval()
        mod64 = quiet(M.KarrasModule, conv64, M.KarrasModuleConfig.from_edm()).double().eval()
        with torch.inference_mode():
            e32 = mod.propagate_white_noise(wn, nsteps=4)
            e64 = mod64.propagate_white_noise(wn.double(), nsteps=4)
        assert e64.dtype == torch.float64
        save("pc2_traj", dict(white_noise=wn, end_f32=e32, end_f64=e64, circular_dims=json.dumps(dims), weights_of="pc2_h", nsteps=4))
        print(f"pc2_traj: end state {tuple(e32.shape)}; fp32 vs fp64 {float((e32.double() - e64).norm() / e64.norm()):.3e}", flush=True)


if __name__ == "__main__":
    main()
