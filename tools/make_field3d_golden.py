"""Generate tests/golden/punetg8_3d_spatial_cond.npz and its weight files (`_w1`, `_w2`, ...): a dimension=3 PUNetG with a
field-valued conditional embedding, run by the reference implementation on the CPU (imported through oracle/tools/refshim.py; needs
the reference checkout that shim points at).  The volume counterpart of `spatial_cond()` in oracle/tools/make_golden.py.  The
fixture is data only: the state_dict, the inputs, the white noise and the reference's outputs.

    python tools/make_field3d_golden.py"""
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

torch.set_num_threads(8)
NAME = "punetg8_3d_spatial_cond"
PART_BYTES = 900 << 10


def build(dtype=torch.float32):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = M.nets.PUNetG(M.nets.PUNetGConfig(model_channels=8, dimension=3),
                            conditional_embedding=torch.nn.Conv3d(2, 8, kernel_size=1))
    return net.to(dtype).eval()


def main():
    torch.manual_seed(370)
    net = build()
    with torch.no_grad():                                     # perturbed norm affines and biases, as spatial_cond() does
        for k, v in net.state_dict().items():
            if "gnorm" in k or k.endswith(".bias"):
                v.add_(0.25 * torch.randn_like(v))
    sd = net.state_dict()
    torch.manual_seed(371)
    x = torch.randn(2, 1, 16, 16, 16)
    y = torch.randn(2, 2, 16, 16, 16)
    t = torch.tensor([0.3, -1.1])
    arrs = {"sd/" + k: v for k, v in sd.items()}
    arrs.update(x=x, y=y, t=t)
    emb = net.conditional_embedding
    with torch.inference_mode():
        arrs["out_f32"] = net(x, t, y)
        arrs["out_uncond_f32"] = net(x, t)
        # one level-1 block: the per-voxel shift of a 16^3 field, CornerPooled to 8^3
        te = net.time_projection(t).reshape(2, 8, 1, 1, 1) + emb(y)
        h = torch.randn(2, 16, 8, 8, 8)
        arrs["resblock_in"] = h
        arrs["resblock_te"] = te
        arrs["resblock_l1"] = net.downward_blocks[1][0](h, te)
    net64 = build(torch.float64)
    net64.load_state_dict({k: v.double() for k, v in sd.items()})
    with torch.inference_mode():
        arrs["out_f64"] = net64(x.double(), t.double(), y.double())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), conditional=True).eval()
    wn = torch.randn(2, 1, 16, 16, 16)
    arrs["white_noise"] = wn
    # the sampler's condition is un-batched (the module unsqueezes it): one field shared by the batch
    for g in (1, 2):
        arrs[f"hist_heun_N4_g{g}_f32"] = module.propagate_white_noise(wn, y=y[0], guidance=float(g), nsteps=4, record_history=True)
    # no committed file above 1 MiB: the fixture's state_dict is spread over weight files `<name>_w<i>.npz` (keys "sd/..."), the
    # inputs and the reference's outputs stay in `<name>.npz`; tests merge them
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
        path = os.path.join(gold, NAME + (f"_w{i}" if i else "") + ".npz")
        np.savez_compressed(path, **{k: np.asarray(v.detach().cpu().numpy()) for k, v in part.items()})
        assert os.path.getsize(path) < 1 << 20, path
        size += os.path.getsize(path)
    rel = float((arrs["out_f32"].double() - arrs["out_f64"]).norm() / arrs["out_f64"].norm())
    cond = float((arrs["out_f32"] - arrs["out_uncond_f32"]).norm() / arrs["out_uncond_f32"].norm())
    print(f"punetg8_3d_spatial_cond: {len(parts)} files, {size / 1024:.1f} KiB; fp32 vs fp64 {rel:.3e}; condition moves the output by {cond:.3e}")


if __name__ == "__main__":
    main()
