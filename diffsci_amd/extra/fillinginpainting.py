"""Large latent volumes from a grid of overlapping cubes (reference: diffsci/extra/fillinginpainting.py, sample_grid_volume):
the cubes at all-even grid positions are sampled on their own, every other cube is inpainted against what its neighbours left
in the volume, optionally with periodic axes.  The integers are the reference's; the data never leaves the GPU:

  the volume [C, X, Y, Z], the noise cube of the same shape and a one-channel "generated" volume live on the device;
  a cube is a periodic gather (ops.box_copy3d) of its noise, its known data and -- from the "generated" volume -- its mask,
  one run of the flow module (SIModule.sample_fused / inpaint_fused: the fused step kernel in a captured run, one graph for all
  cubes of a shape), and a periodic scatter (ops.box_scatter3d) of the result and of ones into the "generated" volume.

grid_plan exposes the integers without a GPU, as chunk_decode.decode_plan does."""
import contextlib
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch

from .. import ops


@dataclass
class Cube:
    """One cube of the grid, in generation order.  start / length: its box in the final volume per axis (a periodic axis wraps:
    start + length may pass the axis' end); mask_boxes: (start, length) boxes in the cube's own coordinates that earlier cubes
    cover (they may overlap each other)."""
    position: Tuple[int, int, int]
    is_corner: bool
    start: Tuple[int, int, int]
    length: Tuple[int, int, int]
    mask_boxes: List[Tuple[Tuple[int, int, int], Tuple[int, int, int]]]


def generation_order(grid_map):
    """fillinginpainting.py:10-126: the eight parity patterns (even, even, even), (even, even, odd), ... (odd, odd, odd) in turn,
    lexicographic within each; -> (positions, how many are in the first pattern: the corners)."""
    n = [int(v) for v in grid_map]
    if len(n) != 3:
        raise ValueError(f"grid_map must be [nx, ny, nz]; got {grid_map!r}")
    positions, corners = [], 0
    for pattern in range(8):
        par = ((pattern >> 2) & 1, (pattern >> 1) & 1, pattern & 1)
        for i in range(par[0], n[0], 2):
            for j in range(par[1], n[1], 2):
                for k in range(par[2], n[2], 2):
                    positions.append((i, j, k))
        if pattern == 0:
            corners = len(positions)
    return positions, corners


def _axis_bounds(i, base, overlap, final, periodic):
    """fillinginpainting.py:153-184 for one axis -> (start, length): clamped at a non-periodic face, wrapped at a periodic one
    (there the length is what periodic_getitem returns for slice(start % final, end % final), torchutils.py:107-153)."""
    start = i * base - overlap // 2
    end = start + base + overlap
    if not periodic:
        start, end = max(0, start), min(final, end)
        return start, max(0, end - start)
    start, end = start % final, end % final
    return start, (final - start + end) if end < start else end - start


def _segments(start, length, final):
    """The box [start, start + length) of an axis of `final` cells as in-range pieces (global start, local start, length)."""
    first = min(length, final - start)
    return [(start, 0, first)] + ([(0, first, length - first)] if length > first else [])


def _axis_overlaps(cur, prev, final):
    """Local intervals (start, length) of the current cube's axis box that the previous cube's box covers."""
    out = []
    for g, loc, n in _segments(cur[0], cur[1], final):
        for pg, _, pn in _segments(prev[0], prev[1], final):
            lo, hi = max(g, pg), min(g + n, pg + pn)
            if hi > lo:
                out.append((loc + lo - g, hi - lo))
    return out


def grid_plan(grid_map, base_shape, overlap_size, periodicity=(False, False, False)):
    """The cubes of sample_grid_volume in generation order (fillinginpainting.py:10-244), host integers only.
    base_shape: [channels, dx, dy, dz].  ValueError: an odd grid extent on a periodic axis (fillinginpainting.py:349-351), a cube
    without cells."""
    grid = [int(v) for v in grid_map]
    base = [int(v) for v in base_shape[1:]]
    per = [bool(p) for p in periodicity]
    if len(grid) != 3 or len(base) != 3 or len(per) != 3:
        raise ValueError("grid_plan: grid_map [nx, ny, nz], base_shape [channels, dx, dy, dz], periodicity of three")
    overlap = int(overlap_size)
    for a in range(3):
        if per[a] and grid[a] % 2 != 0:
            raise ValueError(f"Grid map for dimension {a} is not even, but periodicity is True")
    final = [b * g for b, g in zip(base, grid)]
    order, corners = generation_order(grid)
    cubes = []
    for ind, pos in enumerate(order):
        bounds = [_axis_bounds(pos[a], base[a], overlap, final[a], per[a]) for a in range(3)]
        if min(n for _, n in bounds) < 1 or any(n > f for (_, n), f in zip(bounds, final)):
            raise ValueError(f"grid_plan: the cube at {pos} has extent {[n for _, n in bounds]} in a volume of {final}")
        boxes = []
        for prev in cubes:
            pb = list(zip(prev.start, prev.length))
            ax = [_axis_overlaps(bounds[a], pb[a], final[a]) for a in range(3)]
            for s0, n0 in ax[0]:
                for s1, n1 in ax[1]:
                    for s2, n2 in ax[2]:
                        boxes.append(((s0, s1, s2), (n0, n1, n2)))
        cubes.append(Cube(pos, ind < corners, tuple(s for s, _ in bounds), tuple(n for _, n in bounds), boxes))
    return cubes


def device_scope(device):
    """Make `device` the current GPU for the launches inside (nothing to do for a host device: the first op refuses it)."""
    device = torch.device(device)
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


def _conditions(y, grid_map):
    """fillinginpainting.py:337-339: None or one dict for every cube, or an array of per-cube conditions indexed [i, j, k]."""
    if isinstance(y, dict) or y is None:
        total = int(np.prod(grid_map))
        cells = np.empty(total, dtype=object)
        for i in range(total):
            cells[i] = y
        return cells.reshape(tuple(grid_map))
    return y


def sample_grid_volume(flow_module, grid_map, base_shape, overlap_size, y=None, guidance: float = 1.0, nsteps: int = 30,
                       integrate_on_sigma: bool = False, noise_injection: bool = False, blend_mode='latest',
                       periodicity=[False, False, False], mask_falloff: int = 0, resample_steps: int = 0, jump_length: int = 1,
                       noise=None, **kwargs):
    """fillinginpainting.py:298-437 -> [1, channels, dx*nx, dy*ny, dz*nz].
    noise (extension, for parity runs): an iterator of the standard-normal draws in the reference's order -- the noise cube
    [1, *final_shape], then per cube what its run consumes (SIModule.sample_fused / inpaint_fused)."""
    if blend_mode != 'latest':
        raise ValueError(f"Unknown blend_mode: {blend_mode}")              # fillinginpainting.py:289-293
    y = _conditions(y, grid_map)
    plan = grid_plan(grid_map, base_shape, overlap_size, periodicity)
    C = int(base_shape[0])
    final = [int(b) * int(g) for b, g in zip(base_shape[1:], grid_map)]
    device = flow_module.device
    draws = iter(noise) if noise is not None else None
    sample = getattr(flow_module, "sample_fused", None)
    inpaint = getattr(flow_module, "inpaint_fused", None)
    extra = {} if draws is None else {"noise": draws}
    with torch.inference_mode(), device_scope(device):
        cube0 = next(draws) if draws is not None else torch.randn(1, C, *final)
        if tuple(cube0.shape) != (1, C, *final):
            raise ValueError(f"injected noise has shape {tuple(cube0.shape)}, expected {(1, C, *final)}")
        noise_cube = cube0[0].to(device=device, dtype=torch.float32).contiguous()
        volume = torch.zeros(C, *final, device=device)
        generated = torch.zeros(1, *final, device=device)
        ones = {}
        for cube in plan:
            ext = tuple(cube.length)
            new = lambda c: torch.empty((c,) + ext, dtype=torch.float32, device=device)        # noqa: E731
            noise_slice = ops.box_copy3d(noise_cube, cube.start, new(C), (0, 0, 0), ext).unsqueeze(0)
            cond = y[cube.position[0], cube.position[1], cube.position[2]]
            if cube.is_corner:
                kw = dict(nsamples=1, shape=[C] + list(ext), y=cond, guidance=guidance, nsteps=nsteps, is_latent_shape=True,
                          integrate_on_sigma=integrate_on_sigma, noise_injection=noise_injection, orig_noise=noise_slice,
                          return_latents=True)
                out = sample(**kw, **extra) if sample is not None else flow_module.sample(**kw)
            else:
                x_orig = ops.box_copy3d(volume, cube.start, new(C), (0, 0, 0), ext)
                mask = ops.box_copy3d(generated, cube.start, new(1), (0, 0, 0), ext).expand(C, *ext).contiguous()
                kw = dict(x_orig=x_orig, mask=mask, nsamples=1, y=cond, guidance=guidance, nsteps=nsteps,
                          integrate_on_sigma=integrate_on_sigma, noise_injection=noise_injection, orig_noise=noise_slice,
                          mask_falloff=mask_falloff, resample_steps=resample_steps, jump_length=jump_length)
                out = inpaint(**kw, **extra) if inpaint is not None else flow_module.inpaint(**kw, **extra)
            ops.box_scatter3d(out[0].contiguous(), (0, 0, 0), volume, cube.start, ext)          # 'latest': overwrite
            if ext not in ones:
                ones[ext] = torch.ones((1,) + ext, device=device)
            ops.box_scatter3d(ones[ext], (0, 0, 0), generated, cube.start, ext)
        return volume.unsqueeze(0)
