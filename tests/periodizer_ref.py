"""The reference's DiffusionPeriodizer (diffsci/extra/periodizer.py) restated as plain torch functions, in the dtype and on the
device of their input: what the tests compare the HIP path against at shapes that have no fixture.  Own code, in the manner of
tests/vaenet_ref.py; the reference's lines are cited.  tests/test_periodizer.py pins it against fixtures the reference itself
produced (tests/golden/periodizer_*.npz).

The arithmetic of `blend` is the reference's, operation by operation -- fl(fl(w a) + fl(fl(1 - w) b)) in the tensor's dtype -- so
on the same weight table it gives the reference's bits; only the way the strips are addressed differs (one mirrored copy of the
axis and a mask, where the reference slices and flips two strips)."""
import math

import torch


def per_axis(v, n):
    """periodizer.py:62-74: an int serves every axis."""
    return (v,) * n if isinstance(v, int) else tuple(v)


def expand(x, pad):
    """expand_periodic (periodizer.py:76-101; periodic_getitem_extended on slice(-p, size + p), torchutils.py): position q of the
    expanded axis holds position (q - p) mod size, whatever the number of periods."""
    pad = per_axis(pad, x.dim() - 2)
    for axis, p in enumerate(pad, start=2):
        size = x.shape[axis]
        index = torch.remainder(torch.arange(-p, size + p, device=x.device), size)
        x = x.index_select(axis, index)
    return x


def crop(x, pad, shape):
    """crop_center (periodizer.py:103-124)."""
    pad = per_axis(pad, x.dim() - 2)
    for axis, (p, size) in enumerate(zip(pad, shape), start=2):
        x = x.narrow(axis, p, size)
    return x


def weights(bw, dtype=torch.float32, device="cpu"):
    """periodizer.py:160-161, evaluated as written."""
    positions = torch.arange(bw, device=device, dtype=dtype)
    return 0.5 * (1 - torch.cos(torch.pi * (positions + 0.5) / bw))


def blend(x, blend_width, tables=None):
    """cosine_blend_boundaries (periodizer.py:126-199): the axes in order, each on the result of the one before; an axis with
    bw <= 0 or 2 bw >= size untouched (periodizer.py:148-156).  Inside the strips -- m = min(q, size-1-q) < bw -- position q
    becomes w[m] * x[q] + (1 - w[m]) * x[size-1-q], both read before either strip is written (periodizer.py:191-197).
    tables: the weights per axis (default: `weights` in x's dtype)."""
    widths = per_axis(blend_width, x.dim() - 2)
    x = x.clone()
    for a, bw in enumerate(widths):
        axis, size = a + 2, x.shape[a + 2]
        if bw <= 0 or 2 * bw >= size:
            continue
        w = weights(bw, x.dtype, x.device) if tables is None else tables[a][:bw].to(x)
        q = torch.arange(size, device=x.device)
        m = torch.minimum(q, size - 1 - q)
        inside = m < bw
        shape = [1] * x.dim()
        shape[axis] = size
        wq = w[m.clamp(max=bw - 1)].reshape(shape)
        blended = wq * x + (1 - wq) * x.flip(axis)
        x = torch.where(inside.reshape(shape), blended, x)
    return x


def forward(net, x, pad, blend_width, *args, tables=None, **kwargs):
    """forward (periodizer.py:201-236) around any callable."""
    return blend(crop(net(expand(x, pad), *args, **kwargs), pad, x.shape[2:]), blend_width, tables)


def analytic_net(x, *args, **kwargs):
    """A shape-preserving "network" that is not periodic in what it does to a periodic input's borders: half the input plus the
    input rolled by (1, 2[, 3]) cells, times a ramp along the last axis -- exact in fp32 for the fixtures' dyadic inputs."""
    shifts = tuple(range(1, x.dim() - 1))
    ramp = torch.arange(x.shape[-1], dtype=x.dtype, device=x.device) / 8
    return 0.5 * x + torch.roll(x, shifts, tuple(range(2, x.dim()))) * (1 + ramp)


def periodicity_error(x, dimension=3):
    """measure_periodicity_error (periodizer.py:313-356) in fp64 on the host."""
    x = x.detach().double().cpu()
    out = {"mse_per_dim": [], "max_diff_per_dim": []}
    for a, name in enumerate("HWD"[:dimension]):
        d = x.select(a + 2, 0) - x.select(a + 2, x.shape[a + 2] - 1)
        out["mse_per_dim"].append(float((d * d).mean()))
        out["max_diff_per_dim"].append(float(d.abs().max()))
        out["mse_" + name], out["max_diff_" + name] = out["mse_per_dim"][-1], out["max_diff_per_dim"][-1]
    out["total_mse"] = math.fsum(out["mse_per_dim"])
    return out


# (shape, pad, blend_width) of the cases the fixtures and the GPU tests share; what each is for is said in tests/test_gpu_periodizer.py
FIELDS = [((2, 3, 6, 7), (1, 2), (2, 3)), ((1, 2, 4, 16), (1, 4), (2, 4)), ((1, 1, 8, 16), (3, 3), (0, 5)),
          ((1, 2, 3, 5), (5, 0), (1, 2)), ((2, 1, 5, 9), 0, 4)]
VOLUMES = [((1, 2, 5, 6, 7), (2, 0, 3), (2, 1, 3)), ((2, 1, 4, 4, 8), 2, (2, 2, 3)), ((1, 3, 8, 8, 8), 4, 0)]


def case_name(shape, pad, bw):
    return "x".join(map(str, shape)) + "_p" + "".join(map(str, per_axis(pad, len(shape) - 2))) + "_b" + \
        "".join(map(str, per_axis(bw, len(shape) - 2)))


def case_input(shape, seed=0):
    """Dyadic values in (-4, 4): every product with the analytic network's factors is exact, and the fixture compresses."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(-63, 64, shape, generator=g).to(torch.float32) / 16
