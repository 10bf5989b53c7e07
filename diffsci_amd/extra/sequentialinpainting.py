"""Volumes extended block by block along the last axis (reference: diffsci/extra/sequentialinpainting.py, sample_sequential_z):
the first block is sampled, every later one is inpainted against the last `overlap_size` cells of the block before it, and
the blocks are stitched with cosine weights over the overlap (or the later block overwrites).  On the device throughout:
the runs are SIModule.sample_fused / inpaint_fused (the fused step kernel in a captured run; the middle blocks share one
graph), the known region and the placements are ops.box_copy3d, the stitch is ops.mask_blend."""
import math

import numpy as np
import torch

from .. import ops
from .fillinginpainting import device_scope


def cosine_blend_weights(overlap_size):
    """sequentialinpainting.py:37-55: (1 - cos(pi * linspace(0, 1, overlap))) / 2, 0 at the earlier block's side."""
    t = torch.linspace(0, 1, overlap_size)
    return (1 - torch.cos(math.pi * t)) / 2


def block_extents(num_blocks, base_dz, overlap_size):
    """sequentialinpainting.py:179-195: the extended length of every block along the last axis -- the base alone for a single
    block, half an overlap more for the first and the last, a whole one for those between."""
    half = overlap_size // 2
    if num_blocks == 1:
        return [base_dz]
    return [base_dz + (half if i in (0, num_blocks - 1) else overlap_size) for i in range(num_blocks)]


def sample_sequential_z(flow_module, num_blocks: int, base_shape, overlap_size: int, y=None, guidance: float = 1.0,
                        nsteps: int = 30, integrate_on_sigma: bool = False, noise_injection: bool = True, blend_mode='cosine',
                        mask_falloff: int = 0, resample_steps: int = 0, jump_length: int = 1, noise=None, **kwargs):
    """sequentialinpainting.py:83-299 -> [1, channels, dx, dy, dz * num_blocks].
    noise (extension, for parity runs): an iterator of the standard-normal draws in the reference's order -- per block its
    start noise [1, *block shape], then what its run consumes (SIModule.sample_fused / inpaint_fused)."""
    if num_blocks < 1:
        raise ValueError("num_blocks must be at least 1")
    if overlap_size < 0:
        raise ValueError("overlap_size must be non-negative")
    if overlap_size % 2 != 0:
        raise ValueError("overlap_size must be even")
    if overlap_size >= base_shape[3]:
        raise ValueError("overlap_size must be less than base block z-dimension")
    half = overlap_size // 2
    if isinstance(y, dict) or y is None:
        conditions = [y for _ in range(num_blocks)]
    elif isinstance(y, np.ndarray):
        conditions = list(y)
    else:
        conditions = y
    if len(conditions) != num_blocks:
        raise ValueError(f"Expected {num_blocks} conditions, got {len(conditions)}")

    C, dx, dy, dz = (int(v) for v in base_shape)
    device = flow_module.device
    draws = iter(noise) if noise is not None else None
    sample = getattr(flow_module, "sample_fused", None)
    inpaint = getattr(flow_module, "inpaint_fused", None)
    extra = {} if draws is None else {"noise": draws}
    extents = block_extents(num_blocks, dz, overlap_size)
    with torch.inference_mode(), device_scope(device):
        volume = torch.zeros(C, dx, dy, dz * num_blocks, device=device)
        new = lambda n: torch.empty(C, dx, dy, n, dtype=torch.float32, device=device)        # noqa: E731
        weights = None
        prev = None
        for i, ext in enumerate(extents):
            core = i * dz
            if i == 0:
                kw = dict(nsamples=1, shape=[C, dx, dy, ext], y=conditions[i], guidance=guidance, nsteps=nsteps,
                          is_latent_shape=True, integrate_on_sigma=integrate_on_sigma, noise_injection=noise_injection,
                          return_latents=True)
                block = (sample(**kw, **extra) if sample is not None else flow_module.sample(**kw))[0].contiguous()
                ops.box_copy3d(block, (0, 0, 0), volume, (0, 0, core), (dx, dy, dz))
            else:
                # the known region: the previous block's last overlap_size cells at the start of this one
                x_orig = torch.zeros(C, dx, dy, ext, device=device)
                ops.box_copy3d(prev, (0, 0, prev.shape[-1] - overlap_size), x_orig, (0, 0, 0), (dx, dy, overlap_size))
                mask = torch.zeros(C, dx, dy, ext, device=device)
                mask[..., :overlap_size] = 1.0
                kw = dict(x_orig=x_orig, mask=mask, nsamples=1, y=conditions[i], guidance=guidance, nsteps=nsteps,
                          integrate_on_sigma=integrate_on_sigma, noise_injection=noise_injection, mask_falloff=mask_falloff,
                          resample_steps=resample_steps, jump_length=jump_length)
                if draws is not None:
                    kw["orig_noise"] = next(draws)                       # the reference's inpaint draws its start noise first
                block = (inpaint(**kw, **extra) if inpaint is not None else flow_module.inpaint(**kw, **extra))[0].contiguous()
                lo, hi = core - half, core + half                        # the overlap in the volume
                if blend_mode == 'cosine':
                    if overlap_size:
                        if weights is None:
                            weights = cosine_blend_weights(overlap_size).to(device).expand(C, dx, dy, overlap_size).contiguous()
                        current = ops.box_copy3d(volume, (0, 0, lo), new(overlap_size), (0, 0, 0), (dx, dy, overlap_size))
                        fresh = ops.box_copy3d(block, (0, 0, 0), new(overlap_size), (0, 0, 0), (dx, dy, overlap_size))
                        blended = ops.mask_blend(current.unsqueeze(0), fresh.unsqueeze(0), weights)[0]
                        ops.box_copy3d(blended, (0, 0, 0), volume, (0, 0, lo), (dx, dy, overlap_size))
                    ops.box_copy3d(block, (0, 0, overlap_size), volume, (0, 0, hi), (dx, dy, core + dz - hi))
                else:                                                    # 'latest': overwrite
                    ops.box_copy3d(block, (0, 0, 0), volume, (0, 0, lo), (dx, dy, half + dz))
            prev = block
        return volume.unsqueeze(0)
