"""Generate the fixtures of the tiled volume sampling (tests/test_tiled_sampling.py, tests/test_gpu_tiled_sampling.py) from the
reference implementation on the CPU (imported through oracle/tools/refshim.py; needs the reference checkout that shim points at).
Data only:

    tests/golden/tiled_plan.npz        per (grid, periodicity) case what the reference's own helpers return: the generation order,
                                       the corner count, every cube's slices (start and stop per axis) and its inpainting mask
    tests/golden/tiled_net_w*.npz      the state_dict of the 3-D PUNetG (NET below) the runs use
    tests/golden/tiled_<case>.npz      one run of sample_grid_volume / sample_sequential_z at nsteps=4: the arguments (JSON), every
                                       standard-normal draw in the order drawn (torch.randn and torch.randn_like), the volume

    python tools/make_tiled_sampling_golden.py"""
import contextlib
import io
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
from diffsci.extra import fillinginpainting as G  # noqa: E402
from diffsci.extra import sequentialinpainting as S  # noqa: E402

torch.set_num_threads(8)
GOLD = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900 << 10
BASE, OVERLAP = [2, 8, 8, 8], 4
NONE, TTF, ALL = [False, False, False], [True, True, False], [True, True, True]
PLANS = [([2, 2, 2], NONE), ([2, 2, 2], TTF), ([2, 2, 2], ALL), ([3, 2, 1], NONE), ([3, 2, 2], NONE), ([3, 2, 2], [False, True, True])]
GRID_RUNS = {"grid222_none": ([2, 2, 2], NONE), "grid222_ttf": ([2, 2, 2], TTF), "grid222_all": ([2, 2, 2], ALL),
             "grid321_none": ([3, 2, 1], NONE)}
# one resolution level: the cubes' sides (10 and 12 at a clamped face, 12 inside and on periodic axes) need only be even
NET = dict(input_channels=2, output_channels=2, model_channels=8, dimension=3, channel_expansion=[2], number_resnet_downward_block=1,
           number_resnet_upward_block=1, number_resnet_attn_block=1, number_resnet_before_attn_block=1,
           number_resnet_after_attn_block=1)
SEQ_RUNS = {f"seq{n}_{mode}": (n, mode) for n in (1, 2, 3) for mode in ("cosine", "latest")}


class DrawRecorder:
    """Every torch.randn / torch.randn_like draw, in order (the generators' and the sampler's only RNG use)."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        self._randn, self._like = torch.randn, torch.randn_like

        def randn(*a, **k):
            e = self._randn(*a, **k)
            self.draws.append(e.clone())
            return e

        def like(x, *a, **k):
            e = self._like(x, *a, **k)
            self.draws.append(e.clone())
            return e
        torch.randn, torch.randn_like = randn, like
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._randn, self._like


def save(name, arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    return os.path.getsize(path)


def plans():
    arrs = {"info": json.dumps(dict(base_shape=BASE, overlap_size=OVERLAP, cases=[[g, p] for g, p in PLANS], net=NET))}
    for c, (grid, per) in enumerate(PLANS):
        final = [BASE[0]] + [b * g for b, g in zip(BASE[1:], grid)]
        order, corners = G._get_grid_generation_order(grid)
        arrs[f"p{c}/order"] = np.asarray(order, dtype=np.int64)
        arrs[f"p{c}/corners"] = np.asarray(corners)
        bounds, done = [], set()
        for j, pos in enumerate(order):
            sl = G._get_cube_spatial_bounds(pos, BASE, OVERLAP, final, per)
            bounds.append([s.start for s in sl] + [s.stop for s in sl])
            mask = G._build_inpaint_mask(pos, done, BASE, OVERLAP, final, per)
            assert bool((mask == mask[:1]).all())
            arrs[f"p{c}/mask{j}"] = mask[0].to(torch.uint8)
            done.add(pos)
        arrs[f"p{c}/bounds"] = np.asarray(bounds, dtype=np.int64)
    print(f"tiled_plan: {save('tiled_plan', arrs) / 1024:.1f} KiB")


def network():
    torch.manual_seed(520)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = M.nets.PUNetG(M.nets.PUNetGConfig(**NET)).eval()
    with torch.no_grad():                                     # perturbed norm affines and biases, as the other fixtures do
        for k, v in net.state_dict().items():
            if "gnorm" in k or k.endswith(".bias"):
                v.add_(0.25 * torch.randn_like(v))
    sd = net.state_dict()
    parts, room = [], []
    for k in sorted(sd, key=lambda k: -sd[k].numel()):
        n = sd[k].numel() * 4
        i = next((i for i in range(len(parts)) if room[i] + n <= PART_BYTES), None)
        if i is None:
            parts.append({})
            room.append(0)
            i = len(parts) - 1
        parts[i]["sd/" + k] = sd[k]
        room[i] += n
    size = sum(save(f"tiled_net_w{i + 1}", part) for i, part in enumerate(parts))
    print(f"tiled_net: {len(parts)} files, {size / 1024:.1f} KiB")
    return net


def run(name, fn, args, seed):
    torch.manual_seed(seed)
    out = io.StringIO()
    with DrawRecorder() as rec, warnings.catch_warnings(), contextlib.redirect_stdout(out):
        warnings.simplefilter("ignore")
        vol = fn()
    assert bool(torch.isfinite(vol).all())
    arrs = {"args": json.dumps(args), "out": vol, "ndraws": np.asarray(len(rec.draws))}
    for i, d in enumerate(rec.draws):
        arrs[f"eps{i:03d}"] = d
    print(f"tiled_{name}: {len(rec.draws)} draws, volume {tuple(vol.shape)}, {save('tiled_' + name, arrs) / 1024:.1f} KiB", flush=True)


def main():
    plans()
    net = network()
    module = M.SIModule(M.SIModuleConfig(scheduler="linear"), net).eval()
    for i, (name, (grid, per)) in enumerate(GRID_RUNS.items()):
        args = dict(grid_map=grid, base_shape=BASE, overlap_size=OVERLAP, nsteps=4, periodicity=per)
        run(name, lambda: G.sample_grid_volume(module, **args), args, 530 + i)
    for i, (name, (blocks, mode)) in enumerate(SEQ_RUNS.items()):
        args = dict(num_blocks=blocks, base_shape=BASE, overlap_size=OVERLAP, nsteps=4, blend_mode=mode)
        run(name, lambda: S.sample_sequential_z(module, **args), args, 540 + i)


if __name__ == "__main__":
    main()
