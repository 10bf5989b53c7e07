"""DiffusionPeriodizer (reference: diffsci/extra/periodizer.py): periodic output from any shape-preserving score network, by
expanding the state periodically, running the network on the expanded state, cropping the centre and cross-fading opposite borders
with cosine weights.  The complement of `convert_conv_to_circular`, which needs a network with a periodic kernel route.

It runs once per network evaluation of every sampler step, so both sides are HIP: the expansion is one ds_box_copy3d
(ops.periodic_expand), crop and blend are one fused pass (ops.crop_blend, ds_periodize.hip) instead of the reference's slice,
clone and three strip updates.  Around a HIP-native network the wrapper is itself a *planned* source for KarrasModule, SIModule and
DDPMModule: it offers the duck-typed protocol engine.ModuleSource reads -- `forward_with_shifts` plus the time-path and guard
attributes, delegated to the inner network -- exactly when the inner network does, so the run keeps its tabulated time path and
its captured hipGraph.  It offers no `field_shifts`: a field-valued conditional embedding is evaluated as given (and the inner
network then refuses a field that does not match the expanded resolution).

What a captured plan bakes in is read through the wrapper: the kernel switches of engine.MODEL_SWITCHES get and set the inner
network's (precision.escalate assigns `model.conv_precision`), `plan_signature` adds pad, blend_width and dimension to the plan key,
and the range guard's device words (nets/precision.py: `_input_flags`) are ONE dict shared with the inner network, which raises
its input-layer flag on itself while the run's last step kernel raises the result word it got from the wrapper.

Kept semantics: the axes are blended in tensor order, each on the values the previous one blended; an axis whose blend_width is
<= 0, or not smaller than half the CROPPED size, is skipped; `cosine_blend_boundaries` returns a new tensor."""
from typing import Tuple, Union

import torch
import torch.nn as nn

from .. import ops
from ..models.karras.engine import MODEL_SWITCHES

# read and written through the wrapper: what engine.model_signature keys a plan on, and what the range guard and its escalation
# read of a network (nets/precision.py)
_INNER = MODEL_SWITCHES + ("auto_precision", "config", "circular", "input_layer", "dim")
# the planned protocol's methods that are the inner network's own
_PROTOCOL = ("embed_time", "time_shifts", "embed_condition", "condition_is_field")


class DiffusionPeriodizer(nn.Module):
    """periodizer.py:23-256.  net: [B, C, *spatial] -> [B, C, *spatial], one of our networks or any torch module on the device;
    pad, blend_width: an int or one per spatial axis; dimension: 2 or 3."""

    def __init__(
        self,
        net: nn.Module,
        pad: Union[int, Tuple[int, ...]],
        blend_width: Union[int, Tuple[int, ...]] = 8,
        dimension: int = 3,
    ):
        super().__init__()
        self.net = net
        self.dimension = dimension

        if isinstance(pad, int):
            self.pad = tuple([pad] * dimension)
        else:
            assert len(pad) == dimension, f"pad must have {dimension} elements"
            self.pad = tuple(pad)

        if isinstance(blend_width, int):
            self.blend_width = tuple([blend_width] * dimension)
        else:
            assert len(blend_width) == dimension, f"blend_width must have {dimension} elements"
            self.blend_width = tuple(blend_width)

        self.__dict__["_expanded"] = {}

    # ------------------------------------------------------------------ what is read through the wrapper
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name in ("net", "_modules"):
                raise
            net = self._modules.get("net")
            if name in _INNER or name in _PROTOCOL:
                return getattr(net, name)                          # AttributeError when the inner network has none either
            # a channel condition (PUNetGCond._split_condition) lives at the network's own resolution: evaluated as given
            if name == "forward_with_shifts" and getattr(net, "forward_with_shifts", None) is not None \
                    and not hasattr(net, "_split_condition"):
                return self._forward_with_shifts
            if name == "forward_unguarded" and getattr(net, "forward_unguarded", None) is not None:
                return self._forward_unguarded
            raise

    def __setattr__(self, name, value):
        net = self.__dict__.get("_modules", {}).get("net")
        # only what the inner network has is the inner network's: nothing is planted on a module that never had the attribute
        if name in _INNER and net is not None and name not in self.__dict__ and hasattr(net, name):
            setattr(net, name, value)
            return
        super().__setattr__(name, value)
        if name == "net":
            # one owner of the guard words: precision.guard_words(self, ...) and the inner network's own find the same tensors;
            # whenever the inner network is assigned, the wrapper's entry becomes that network's
            if isinstance(value, nn.Module):
                self.__dict__["_input_flags"] = value.__dict__.setdefault("_input_flags", {})
            else:
                self.__dict__.pop("_input_flags", None)

    def plan_signature(self):
        """What a captured run bakes in of the wrapper itself (engine.model_signature); the input shape does not determine it."""
        return ("periodizer", self.pad, self.blend_width, self.dimension)

    # ------------------------------------------------------------------ the reference's methods
    def _check(self, x):
        spatial_shape = x.shape[2:]
        assert len(spatial_shape) == self.dimension, \
            f"Expected {self.dimension}D spatial input, got {len(spatial_shape)}D"

    def expand_periodic(self, x: torch.Tensor) -> torch.Tensor:
        """periodizer.py:76-101: [B, C, *S] -> [B, C, *(S + 2 pad)]."""
        self._check(x)
        return ops.periodic_expand(x.contiguous(), self.pad)

    def crop_center(self, x: torch.Tensor, original_shape: Tuple[int, ...]) -> torch.Tensor:
        """periodizer.py:103-124 (a view, as there)."""
        slices = [slice(None), slice(None)]
        for p, orig_size in zip(self.pad, original_shape):
            slices.append(slice(p, p + orig_size))
        return x[tuple(slices)]

    def cosine_blend_boundaries(self, x: torch.Tensor) -> torch.Tensor:
        """periodizer.py:126-199: a new tensor; the kernel with zero pads."""
        self._check(x)
        return ops.crop_blend(x.contiguous(), 0, self.blend_width)

    @ops.device_guard
    def forward(self, x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        """periodizer.py:201-236: expand, net(x_expanded, *args, **kwargs), crop and blend."""
        return self._around(x, self.net, self.blend_width, args, kwargs)

    @ops.device_guard
    def forward_no_blend(self, x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        """periodizer.py:238-247: zero widths."""
        return self._around(x, self.net, 0, args, kwargs)

    @ops.device_guard
    def forward_expand_only(self, x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        """periodizer.py:249-256."""
        return self.net(self.expand_periodic(x), *args, **kwargs)

    def _around(self, x, net, blend_width, args, kwargs):
        y_expanded = net(self.expand_periodic(x), *args, **kwargs)
        ops.require_device(y_expanded, "network output")
        return ops.crop_blend(y_expanded.contiguous(), self.pad, blend_width)

    # ------------------------------------------------------------------ the planned protocol (engine.ModuleSource)
    def _forward_unguarded(self, x, *args, **kwargs):
        """forward around the inner network's unguarded evaluation: a sampler run checks the range guards once, at its end."""
        return self._around(x, self.net.forward_unguarded, self.blend_width, args, kwargs)

    def _buffer(self, role, shape, device):
        """An expanded tensor owned here ("x": the network's input, "y": its output), one per role, expanded shape and device,
        never evicted: a captured plan has its address baked in and keeps reading and writing the buffer of its shape for as long
        as the plan may be replayed (the rule of the networks' own plan buffers).  Keyed on the EXPANDED shape, so a pad assigned
        after construction finds a buffer of its own."""
        key = (role, tuple(shape), str(device))
        buf = self._expanded.get(key)
        if buf is None:
            with torch.inference_mode(False):
                buf = self._expanded[key] = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        return buf

    def _forward_with_shifts(self, x, shifts, row=None, out=None):
        """Expand into a buffer owned here, the inner network's planned evaluation at the expanded shape, crop and blend into
        out: one ds_box_copy3d, the network's own launches, one ds_crop_blend."""
        self._check(x)
        spatial = tuple(s + 2 * p for s, p in zip(x.shape[2:], self.pad))
        xe = ops.periodic_expand(x.contiguous(), self.pad, out=self._buffer("x", tuple(x.shape[:2]) + spatial, x.device))
        # (no out: the network allocates its result, as it does for its caller)
        ye = None if out is None else self._buffer("y", (x.shape[0], out.shape[1]) + spatial, x.device)
        ye = self.net.forward_with_shifts(xe, shifts, row=row, out=ye)
        return ops.crop_blend(ye, self.pad, self.blend_width, out=out)


class PeriodicSamplerWrapper:
    """periodizer.py:259-310, unchanged: every apply_every_n_steps-th step goes through the periodizer, the others through the
    sampler."""

    def __init__(
        self,
        sampler,
        periodizer: DiffusionPeriodizer,
        apply_every_n_steps: int = 1,
    ):
        self.sampler = sampler
        self.periodizer = periodizer
        self.apply_every_n_steps = apply_every_n_steps
        self._step_count = 0

    def step(self, x: torch.Tensor, t: torch.Tensor, **kwargs) -> torch.Tensor:
        self._step_count += 1

        if self._step_count % self.apply_every_n_steps == 0:
            return self.periodizer(x, t=t, **kwargs)
        else:
            return self.sampler.step(x, t, **kwargs)

    def reset(self):
        """Reset step counter (call before each new sample)."""
        self._step_count = 0


def measure_periodicity_error(x: torch.Tensor, dimension: int = 3) -> dict:
    """periodizer.py:313-356: how far x [B, C, *spatial] is from periodic -- per spatial axis the mean square and the largest
    absolute difference between its first and its last slice, as host floats: mse_<H|W|D>, max_diff_<H|W|D>, and the lists
    mse_per_dim, max_diff_per_dim with total_mse = sum(mse_per_dim)."""
    names = ['H', 'W', 'D'][:dimension]
    errors, mses, maxima = {}, [], []
    for axis, name in enumerate(names, start=2):
        diff = x.select(axis, 0) - x.select(axis, -1)
        mses.append((diff ** 2).mean().item())
        maxima.append(diff.abs().max().item())
        errors[f'mse_{name}'], errors[f'max_diff_{name}'] = mses[-1], maxima[-1]
    errors['total_mse'] = sum(mses)
    errors['mse_per_dim'] = mses
    errors['max_diff_per_dim'] = maxima
    return errors
