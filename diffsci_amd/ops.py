"""Tensor-level wrappers over the C ABI: shape / dtype / device checks on the host, then a raw
pointer + stream call.  PyTorch is used only as the owner of device memory and of the stream."""
import ctypes
import gc

import torch

from . import _native as N
from ._native import EvalCoef  # noqa: F401  (re-export)


def _off_device(t):
    """Why tensor t cannot be handed to a launch on the current stream: "host" when it is not in GPU memory, "other" when it
    lives on another GPU than the current one; None for a device tensor on the current device.  The one place that decides."""
    if not t.is_cuda:
        return "host"
    return None if t.device.index == torch.cuda.current_device() else "other"


def require_device(t, what="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    off = _off_device(t)
    if not off and t.dtype == torch.float32:
        return
    if off == "host":
        raise RuntimeError(
            f"{what} lives on {t.device}: diffsci_amd computes only on an AMD GPU through "
            "libdiffsci_hip.so (there is no CPU path; move the module and inputs to 'cuda').")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} has dtype {t.dtype}; the HIP path is fp32 only")
    # the C ABI launches on the stream it is handed and never switches devices: a launch on cuda:0's stream
    # with cuda:1 pointers would fault (or silently compute on the wrong GPU's copy of a kernel attribute)
    raise RuntimeError(f"{what} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                       "wrap the call in `with torch.cuda.device(tensor.device):` (KarrasModule / SIModule / the "
                       "networks do this for their own entry points)")


def on_device_of(t):
    """Context manager: make t's GPU the current device (and its current stream the launch stream)."""
    return torch.cuda.device(t.device)


def device_guard(fn):
    """Decorator for the public entry points of the modules: run with the GPU of the first CUDA tensor argument as
    the current device, so a module on cuda:1 works while the caller's current device is cuda:0 (the C ABI launches
    on the stream it is handed and never switches devices; every op checks its tensors against the current device)."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return wrapped


def _p(t, what="tensor"):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or _off_device(t) or t.dtype != torch.float32:
        require_device(t, what)                  # raises, and says which (here only the test: one frame less per pointer)
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- the checking vocabulary of the wrappers below
# The C side refuses NULL and non-positive sizes but cannot know how large a buffer is, so no pointer reaches the ABI without
# an extent check made here.  Each decision is written once; a message that takes formatting is built only
# when its check fails -- the eager paths pay Python per launch.
def _out(out, shape, like, msg="out has shape {}, expected {}"):
    """The output of a kernel that indexes by `shape`: a fresh fp32 tensor on like's device, or the given one verified.
    msg is formatted with (the given shape, the expected one)."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(msg.format(tuple(out.shape), tuple(shape)))
    return out


_STATS_MSG, _TABLE_MSG = "stats must be {1}", "table must be {1}"       # _out messages of the norm statistics and tables


def _same_numel(*ts):
    n = None
    for t in ts:
        if t is None:
            continue
        if n is None:
            n = t.numel()
        elif t.numel() != n:
            raise ValueError(f"size mismatch: {t.numel()} vs {n} elements")
    return n


def _out_flat(out, *same, like=None):
    """The flat twin, for kernels that index one range of n elements whatever the shapes (callers pass views of the same
    size): a fresh tensor like `like` (default: the first of `same`), or the given one; all of `same` and out must hold the
    same number of elements.  -> (out, n)."""
    if out is None:
        out = torch.empty_like(same[0] if like is None else like)
    return out, _same_numel(*same, out)


def _row_stride(t, B, width, msg):
    """Per-sample rows [1 or B, width] (None: none) -> the stride in floats between the samples' rows: 0 when one row serves
    all, else width.  msg is formatted with the shape given."""
    if t is None:
        return 0
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] not in (1, B):
        raise ValueError(msg.format(tuple(t.shape)))
    return 0 if t.shape[0] == 1 else width


_SHIFT_MSG = "shift must be [1 or B, Cout]; got {}"      # every convolution's per-sample shift [1 or B, Cout]


def _film_args(film, B, C):
    """(scale pointer, shift pointer, stride) of FiLM rows [1 or B, 2C] (embed_linear(te)), or (None, None, 0)."""
    if film is None:
        return None, None, 0
    stride = _row_stride(film, B, 2 * C, "film must be [1 or B, 2C]")
    p = _p(film, "film")                 # on the device and contiguous: a strided view of a wider table has other rows
    return p, p + 4 * C, stride


def _residuals(shape, *rs):
    for r in rs:
        if r is not None and tuple(r.shape) != shape:
            raise ValueError("residual shape mismatch")


def _entries(t, n, msg, *fmt):
    """A per-channel vector (bias, norm weight, ...) holds n entries; None passes.  msg.format(*fmt) on failure."""
    if t is not None and t.numel() != n:
        raise ValueError(msg.format(*fmt))


def _affine(w, b, C, what):
    """_entries for a norm's weight and bias (one frame for the pair: norms sit on the eager paths)."""
    if w is not None and w.numel() != C:
        raise ValueError(f"{what}: norm weight must have C={C} entries")
    if b is not None and b.numel() != C:
        raise ValueError(f"{what}: norm bias must have C={C} entries")


def _gnorm1_inputs(stats, w, b, B, C, what):
    """What a gnorm1 apply kernel reads next to x: stats [B, 2] (None for kind 2, the identity) and C-entry affines."""
    if stats is not None and tuple(stats.shape) != (B, 2):
        raise ValueError(f"{what}: stats must be {(B, 2)}; got {tuple(stats.shape)}")
    _affine(w, b, C, what)


def _tile_stats(ts, B, Cout, H, W, got=False):
    """tile_stats of an fp16x3 convolution's [B, Cout, H, W] output (None passes)."""
    if ts is not None and tuple(ts.shape) != (B, Cout, conv_tile_count(H, W), 4):
        raise ValueError(f"tile_stats must be {(B, Cout, conv_tile_count(H, W), 4)}" + (f"; got {tuple(ts.shape)}" if got else ""))


def _images(buf, B, C, H, W, msg, like=None):
    """The pre-split image buffer of a [B, C, H, W] activation: conv_images_floats elements; like: allocate when None."""
    n = conv_images_floats(B, C, H, W)
    if buf is None and like is not None:
        return torch.empty(n, dtype=torch.float32, device=like.device)
    if buf.numel() != n:
        raise ValueError(msg)
    return buf


def _groups(C, G, what):
    G = int(G)
    if G < 1 or C % G:
        raise ValueError(f"{what}: C={C} is not a multiple of num_groups={G}")
    return G


def _workspace(workspace, nbytes, like, msg):
    """Scratch of at least nbytes for a kernel: the given fp32 tensor verified, or a fresh one."""
    if workspace is None:
        return torch.empty(nbytes // 4, dtype=torch.float32, device=like.device)
    if workspace.numel() * 4 < nbytes:
        raise ValueError(msg)
    return workspace


def _load_sides(load_mode, sides):
    """Output sides of a convolution whose loader pools or upsamples by two (AVGPOOL2 exists on fields only: the volume
    kernels read it as a plain load)."""
    if load_mode == N.DS_LOAD_PLAIN:
        return sides
    if load_mode == N.DS_LOAD_MAXPOOL2 or (load_mode == N.DS_LOAD_AVGPOOL2 and len(sides) == 2):
        if any(s % 2 for s in sides):
            raise ValueError("pooling load needs even input H, W" if len(sides) == 2 else "pooling load needs an even input volume")
        return tuple(s // 2 for s in sides)
    if load_mode == N.DS_LOAD_UPSAMPLE2:
        return tuple(2 * s for s in sides)
    return sides


class _Scratch:
    """The temporaries of one composed call: from the pool `ws` (take(shape, device) / give(tensor); a captured loop must not
    allocate) or, ws=None, from torch's allocator.  give() hands back everything taken, in the order it was taken."""
    __slots__ = ("ws", "device", "taken")

    def __init__(self, ws, device):
        self.ws, self.device, self.taken = ws, device, []

    def take(self, shape):
        if self.ws is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        t = self.ws.take(shape, self.device)
        self.taken.append(t)
        return t

    def amax(self, rows):
        """Zeroed amax slots (see below): a pool buffer cleared by a launch, or a fresh zeroed tensor."""
        return amax_new(rows, self.device) if self.ws is None else amax_zero(self.take((rows,)).view(torch.int32))

    def give(self):
        for t in self.taken:
            self.ws.give(t)


# ---------------------------------------------------------------- per-sample activation exponents of the fp16x3 kernels
# fp16 has 5 exponent bits; the reference's fp32 convolutions take raw user fields (punetg.py:719-735) and c_in = 1
# parameterisations (preconditioners.py:139-161) at any magnitude.  A launch whose input is not normalised by construction
# scales sample b by a power of two taken from max |x_b| (include/diffsci_hip.h: in_amax / out_amax).  "amax" tensors are
# int32 [rows] holding float bits; they are MERGED into (atomicMax), so they start from zero.
class _Normalised:
    """in_amax=NORMALISED: the input is normalised by construction (a norm + SiLU output): no scaling, no reduction."""

    def __repr__(self):
        return "ops.NORMALISED"


NORMALISED = _Normalised()


def _pi(t, n, what="amax"):
    if t is None:
        return None
    off = _off_device(t) if isinstance(t, torch.Tensor) else "host"
    if off == "host" or not (t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
        raise TypeError(f"{what} must be a contiguous int32 device tensor of {n} entries (float bits of per-sample max |x|)")
    if off:
        raise RuntimeError(f"{what} lives on another device than the current one")
    return t.data_ptr()


def amax_zero(t):
    """Zero amax slots (a one-line kernel: hipGraph memset nodes replay unreliably on this ROCm, see ds_amax.hip)."""
    N.check(N.lib().ds_fill_u32(_pi(t, t.numel()), 0, t.numel(), _stream()), "ds_fill_u32")
    return t


def amax_new(rows, device):
    return torch.zeros(int(rows), dtype=torch.int32, device=device)


def absmax_rows(x, rows=None, out=None):
    """out[r] = max(out[r], float bits of max |x[r]|) over the rows of x viewed as [rows, -1] (default: the batch dimension).
    x: contiguous, or a channel slice x_full[:, c0:c1] of a contiguous tensor (rows = samples, dense inside a row).
    out=None: a fresh zeroed tensor (an allocation: captured code passes its own, zeroed, slots)."""
    require_device(x, "x")
    if x.is_contiguous():
        rows = x.shape[0] if rows is None else int(rows)
        n = x.numel() // max(rows, 1)
        stride = n
    else:
        if rows not in (None, x.shape[0]) or x.dim() < 2 or not x[0].is_contiguous():
            raise ValueError("absmax_rows: x must be contiguous or a channel slice of a contiguous tensor")
        rows, n, stride = x.shape[0], x[0].numel(), x.stride(0)
    if out is None:
        out = amax_new(rows, x.device)
    N.check(N.lib().ds_absmax_rows(_pi(out, rows), x.data_ptr(), rows, n, stride, _stream()), "ds_absmax_rows")
    return out


CHANNEL_GAP = 14     # binades: see ds_absmax_channels


def absmax_channels(x, out, scratch, flag=None, wmax=None, gap=CHANNEL_GAP):
    """absmax_rows for an input layer's x [B, C, *spatial]: out [B] (zeroed slots) <- per-sample maxima; scratch: zeroed int32
    [B*C]; flag (int32 [1] or None) is OR-ed with 1 when one exponent per sample cannot serve the layer given its weights (wmax
    [C]: largest |weight| per input channel) -- the caller's signal to run that layer on the exact-fp32 kernel (nets/precision.py)."""
    require_device(x, "x")
    if not x.is_contiguous():
        raise ValueError("absmax_channels: x must be contiguous")
    B, C = x.shape[0], x.shape[1]
    if wmax is not None and wmax.numel() != C:
        raise ValueError("absmax_channels: wmax must hold one entry per input channel")
    N.check(N.lib().ds_absmax_channels(_pi(out, B), _pi(flag, 1, "flag"), _pi(scratch, B * C, "scratch"), x.data_ptr(), _p(wmax, "wmax"),
                                       B, C, x.numel() // max(B * C, 1), int(gap), _stream()), "ds_absmax_channels")
    return out


INPUT_AMAX_MAX_FLOATS = 1 << 20      # per sample: above this one workgroup per sample would be the slow way


def input_amax(arena, out_row, x, flag=None, wmax=None, gap=CHANNEL_GAP):
    """One launch at the head of a network evaluation: zero the amax arena (int32 [rows, B]) and fill its row `out_row` with the
    per-sample maxima of the input x [B, C, *spatial] (C <= 64, C * spatial <= INPUT_AMAX_MAX_FLOATS), with absmax_channels'
    channel criterion.  Returns the row."""
    require_device(x, "x")
    rows, B = arena.shape
    C = x.shape[1]
    if x.shape[0] != B or not x.is_contiguous() or not arena.is_contiguous() or arena.dtype != torch.int32:
        raise ValueError("input_amax: arena int32 [rows, B] and a contiguous x [B, C, ...]")
    N.check(N.lib().ds_input_amax(arena.data_ptr(), rows, int(out_row), _pi(flag, 1, "flag"), x.data_ptr(), _p(wmax, "wmax"), B, C,
                                  x.numel() // max(B * C, 1), int(gap), _stream()), "ds_input_amax")
    return arena[out_row]


def amax_merge(out, a, b=None):
    """out[i] = max(out[i], a[i], b[i]): the amax of a channel concatenation from those of its parts."""
    n = out.numel()
    N.check(N.lib().ds_amax_merge(_pi(out, n), _pi(a, n), _pi(b, n), n, _stream()), "ds_amax_merge")
    return out


def _in_amax(x, in_amax, rows, raw):
    """Pointer for a kernel's in_amax argument.  raw: the launch reads x without a normalising loader (with one, the table's
    fourth column carries the exponent)."""
    if in_amax is NORMALISED or not raw:
        return None
    if in_amax is None:
        in_amax = absmax_rows(x, rows)
    return _pi(in_amax, rows, "in_amax")


def _xin_numel(x, xin_out, copies):
    """xin_out of the step kernels: numel of x, or twice that when the kernel writes two copies (batched guidance)."""
    if xin_out is not None and xin_out.numel() != x.numel() * (2 if copies == 2 else 1):
        raise ValueError(f"xin_out holds {xin_out.numel()} elements; expected {x.numel() * (2 if copies == 2 else 1)}")


def scale(x, s, out=None):
    out, n = _out_flat(out, x)
    N.check(N.lib().ds_karras_scale(_p(out, "out"), _p(x, "x"), float(s), n, _stream()), "ds_karras_scale")
    return out


def add(a, b, out=None):
    out, n = _out_flat(out, a, b)
    N.check(N.lib().ds_add(_p(out), _p(a), _p(b), n, _stream()), "ds_add")
    return out


def mask_blend(x, y, mask, out=None):
    """x*(1-mask) + y*mask with mask [*shape] broadcast over the batch."""
    B = x.shape[0]
    nps = x.numel() // max(B, 1)
    if y.shape != x.shape or mask.numel() != nps:
        raise ValueError(f"mask_blend: x {tuple(x.shape)}, y {tuple(y.shape)}, mask {tuple(mask.shape)}")
    out, _ = _out_flat(out, x)
    N.check(N.lib().ds_mask_blend(_p(out), _p(x), _p(y), _p(mask), nps, B, _stream()), "ds_mask_blend")
    return out


def axpby(x, a, y=None, b=0.0, out=None):
    """a*x + b*y (y optional)."""
    out, n = _out_flat(out, x, y)
    N.check(N.lib().ds_axpby(_p(out), _p(x), float(a), _p(y), float(b), n, _stream()), "ds_axpby")
    return out


def div_scalar(x, s, out=None):
    """x / s."""
    out, n = _out_flat(out, x)
    N.check(N.lib().ds_div_scalar(_p(out), _p(x), float(s), n, _stream()), "ds_div_scalar")
    return out


def batchnorm_eval(x, mean, var, weight=None, bias=None, eps=1e-5, sigma=1.0, inverse=False, out=None):
    """DimensionAgnosticBatchNorm.forward / .unnorm with running statistics; x [B, C, *spatial]."""
    require_device(x, "x")
    out, _ = _out_flat(out, x)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1)
    nc = mean.numel()
    if var.numel() != nc or nc not in (1, C) or (weight is not None and (weight.numel() != nc or bias.numel() != nc)):
        raise ValueError("batch-norm statistics / affine must hold 1 or C entries")
    N.check(N.lib().ds_batchnorm_eval(_p(out), _p(x), _p(mean), _p(var), _p(weight), _p(bias), float(eps), float(sigma),
                                      1 if inverse else 0, B, C, nc, HW, _stream()), "ds_batchnorm_eval")
    return out


def lerp_stack(x1, x2, n):
    """stack([x1 + (x2 - x1)*i/(n-1) for i in range(n)])."""
    _same_numel(x1, x2)
    out = torch.empty((n,) + tuple(x1.shape), dtype=torch.float32, device=x1.device)
    N.check(N.lib().ds_lerp_stack(_p(out), _p(x1), _p(x2), int(n), x1.numel(), _stream()), "ds_lerp_stack")
    return out


def drift(x, f, k, fu=None, out=None):
    out, n = _out_flat(out, x, f, fu, like=f)
    N.check(N.lib().ds_karras_drift(_p(out), _p(x), _p(f), _p(fu), ctypes.byref(k), n, _stream()),
            "ds_karras_drift")
    return out


def score(x, f, k, fu=None, out=None):
    out, n = _out_flat(out, x, f, fu, like=f)
    N.check(N.lib().ds_karras_score(_p(out), _p(x), _p(f), _p(fu), ctypes.byref(k), n, _stream()),
            "ds_karras_score")
    return out


def _philox(philox):
    """(state tensor int64[2] on the device, offset) -> (pointer, offset) or (None, 0)."""
    if philox is None:
        return None, 0
    state, offset = philox
    off = _off_device(state) if isinstance(state, torch.Tensor) else "host"
    if off == "host" or not (state.dtype == torch.int64 and state.numel() == 2 and state.is_contiguous()):
        raise TypeError("philox state must be a contiguous int64[2] device tensor (seed, base offset)")
    if off:
        raise RuntimeError("philox state lives on another device than the current one")
    return state.data_ptr(), int(offset)


def philox_counters(n):
    """Philox counters one noise tensor of n elements consumes (4 normals per counter)."""
    return (int(n) + 3) // 4


def philox_normal(state, offset, shape, out=None):
    """The standard-normal stream the stepper kernels generate in place for (state, offset): element e <- counter
    state[1] + offset + e/4, output e%4."""
    if out is None:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=state.device)
    ps, po = _philox((state, offset))
    N.check(N.lib().ds_philox_normal(_p(out, "out"), ps, po, out.numel(), _stream()), "ds_philox_normal")
    return out


def euler(x, f, k, dt, fu=None, x_out=None, xin_out=None, c_in_next=1.0, eps=None, noise_coef=0.0,
          sqrt_abs_dt=0.0, philox=None):
    n = _same_numel(x, f, fu, x_out, eps)
    _xin_numel(x, xin_out, k.xin_copies)
    ps, po = _philox(philox)
    N.check(N.lib().ds_karras_euler(_p(x_out), _p(xin_out), _p(x), _p(f), _p(fu), ctypes.byref(k),
                                    float(dt), float(c_in_next), _p(eps), ps, po, float(noise_coef),
                                    float(sqrt_abs_dt), n, _stream()), "ds_karras_euler")
    return x_out


DDPM_FORMS = {"classical": N.DS_DDPM_CLASSICAL, "generalized": N.DS_DDPM_GENERALIZED, "forward": N.DS_DDPM_FORWARD}


def ddpm_step(x, f, k, form, eps=None, philox=None, out=None):
    """One DDPM / DDIM step (ds_ddpm.hip) under k (DDPMCoef): form "classical" c1*(x - c0*f) + c2*e, "generalized"
    (c2*((x - f*c0)/c1) + c3*f) + c4*e, or "forward" c0*x + c1*e (f is None).  e: eps (injected, x's extent), philox = (state,
    offset) (drawn in the kernel), or neither -- the noise term is then dropped.  out: x itself (in place), or any other buffer of
    x's shape (a history row); default a new tensor.  ValueError / TypeError before any launch for what a kernel would overrun or
    misread."""
    if form not in DDPM_FORMS:
        raise ValueError(f"ddpm_step: form must be one of {sorted(DDPM_FORMS)}; got {form!r}")
    if not isinstance(k, N.DDPMCoef):
        raise TypeError("ddpm_step: k must be a DDPMCoef")
    require_device(x, "x")
    if form == "forward":
        if f is not None:
            raise ValueError("ddpm_step: the forward form reads no network output (f must be None)")
    elif f is None:
        raise ValueError(f"ddpm_step: the {form} form reads the network output f")
    if eps is not None and philox is not None:
        raise ValueError("ddpm_step: give injected eps or a Philox state, not both")
    out = _out(out, x.shape, x)
    n = _same_numel(x, f, eps, out)
    if out.data_ptr() != x.data_ptr() and _overlap(out, x):
        raise ValueError("ddpm_step: out overlaps x (it may only be x itself)")
    if any(_overlap(out, t) for t in (f, eps)):
        raise ValueError("ddpm_step: out overlaps an input")
    ps, po = _philox(philox)
    flags = DDPM_FORMS[form] | (N.DS_DDPM_NOISE_EPS if eps is not None else N.DS_DDPM_NOISE_PHILOX if ps is not None
                                else N.DS_DDPM_NOISE_NONE)
    N.check(N.lib().ds_ddpm_step(_p(out, "out"), _p(x, "x"), _p(f, "f"), ctypes.byref(k), _p(eps, "eps"), ps, po, n, _stream(),
                                 flags), "ds_ddpm_step")
    return out


def _overlap(a, b):
    """Do two tensors share bytes?  (contiguous tensors: their address ranges)"""
    if a is None or b is None or not a.numel() or not b.numel():
        return False
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def si_inpaint_counters(B, n, blend=False, renoise=False):
    """Philox counters one si_inpaint_step launch consumes (ds_si_inpaint_counters: the step's [B, n], with the blend the
    patch's [n], with the jump both again).  Host arithmetic of the library: no launch."""
    flags = (N.DS_SI_BLEND if blend or renoise else 0) | (N.DS_SI_RENOISE if renoise else 0)
    return int(N.lib().ds_si_inpaint_counters(int(B), int(n), flags))


def si_inpaint_step(x, f, k, s, fu=None, x_orig=None, mask=None, blend=False, renoise=False, eps=None, philox=None, x_out=None,
                    xin_out=None):
    """One inner iteration of SIModule.inpaint after the network call, fused (ds_inpaint.hip): the Euler-Maruyama step under
    k (EvalCoef) and s (SIStep), with blend the known region x_orig [n] re-imposed under mask [n], with renoise the jump back
    and its blend; x [B, n...] -> x_out (may be x itself) and xin_out = c_in_next * result (k.xin_copies copies).  Noise: eps =
    (step [B, n], patch [n], jump [B, n], jump patch [n]) as far as the mode draws, or philox = (state, offset).  ValueError
    before any launch for sizes that disagree, a missing draw, outputs that overlap an input."""
    if renoise and not blend:
        raise ValueError("si_inpaint_step: renoise goes with blend")
    if (eps is None) == (philox is None):
        raise ValueError("si_inpaint_step: give injected eps or a Philox state, exactly one")
    if x_out is None and xin_out is None:
        raise ValueError("si_inpaint_step: no output requested")
    B = x.shape[0] if x.dim() else 0
    n = _same_numel(x, f, fu, x_out)
    nps = n // B if B else 0
    if B < 1 or nps < 1:
        raise ValueError(f"si_inpaint_step: empty state {tuple(x.shape)}")
    _xin_numel(x, xin_out, k.xin_copies)
    if blend:
        if x_orig is None or mask is None or x_orig.numel() != nps or mask.numel() != nps:
            raise ValueError(f"si_inpaint_step: x_orig and mask must hold one sample ({nps} elements)")
    else:
        x_orig = mask = None
    draws = [None] * 4
    if eps is not None:
        want = 4 if renoise else (2 if blend else 1)
        eps = tuple(eps)
        if len(eps) < want or any(e is None for e in eps[:want]):
            raise ValueError(f"si_inpaint_step: this mode reads {want} injected draws; got {len(eps)}")
        for i in range(want):
            if eps[i].numel() != (n if i % 2 == 0 else nps):
                raise ValueError(f"si_inpaint_step: draw {i} holds {eps[i].numel()} elements; expected {n if i % 2 == 0 else nps}")
            draws[i] = eps[i]
    ins = [t for t in (f, fu, x_orig, mask) + tuple(draws) if t is not None]
    if x_out is not None and x_out.data_ptr() != x.data_ptr() and _overlap(x_out, x):
        raise ValueError("si_inpaint_step: x_out overlaps x (it may only be x itself)")
    if any(_overlap(x_out, t) for t in ins) or any(_overlap(xin_out, t) for t in ins + [x, x_out]):
        raise ValueError("si_inpaint_step: an output overlaps an input")
    ps, po = _philox(philox)
    flags = (N.DS_SI_BLEND if blend else 0) | (N.DS_SI_RENOISE if renoise else 0)
    ptrs = [_p(t, what) for t, what in ((x_out, "x_out"), (xin_out, "xin_out"), (x, "x"), (f, "f"), (fu, "fu"), (x_orig, "x_orig"),
                                        (mask, "mask"))] + [_p(e, "eps") for e in draws]
    N.check(N.lib().ds_si_inpaint_step(*ptrs[:5], ctypes.byref(k), ctypes.byref(s), *ptrs[5:], ps, po, B, nps, _stream(), flags),
            "ds_si_inpaint_step")
    return x_out


def heun(x, f1, k1, f2, k2, dt, f1u=None, f2u=None, x_out=None, xin_out=None, c_in_next=1.0):
    n = _same_numel(x, f1, f2, f1u, f2u, x_out)
    _xin_numel(x, xin_out, k2.xin_copies)
    N.check(N.lib().ds_karras_heun(_p(x_out), _p(xin_out), _p(x), _p(f1), _p(f1u), ctypes.byref(k1),
                                   _p(f2), _p(f2u), ctypes.byref(k2), float(dt), float(c_in_next), n,
                                   _stream()), "ds_karras_heun")
    return x_out


def churn(x, eps, coef, xhat_out, xin_out=None, c_in=1.0, philox=None, ratio=1.0, scale=1.0, xin_copies=1):
    """x_hat = ratio*x + coef*eps, with eps injected (a tensor) or, eps=None, generated in the kernel from
    philox = (state, offset); xin_out = c_in * (x_hat / scale), written xin_copies (1 or 2) times back to back."""
    n = _same_numel(x, eps, xhat_out)
    _xin_numel(x, xin_out, xin_copies)
    ps, po = _philox(philox)
    N.check(N.lib().ds_karras_churn(_p(xhat_out), _p(xin_out), _p(x), _p(eps), ps, po, float(coef), float(c_in), float(ratio),
                                    float(scale), int(xin_copies), n, _stream()), "ds_karras_churn")
    return xhat_out


def denoiser(x, f, c_out, c_skip, fu=None, guidance=1.0, out=None):
    B = x.shape[0]
    if c_out.numel() != B or c_skip.numel() != B:
        raise ValueError("c_out / c_skip must have one entry per sample")
    out, _ = _out_flat(out, x, f, fu)
    N.check(N.lib().ds_karras_denoiser(_p(out), _p(x), _p(f), _p(fu), float(guidance), float(1 - guidance),
                                       _p(c_out), _p(c_skip), B, x.numel() // max(B, 1), _stream()),
            "ds_karras_denoiser")
    return out


def inorm_silu(x, w, b, kind, eps=1e-5, out=None):
    """kind 0: GroupNorm(C, C)+SiLU, kind 1: GroupRMSNorm(C, C)+SiLU; x [B, C, *spatial]."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1)
    if w is not None and (w.numel() != C or b.numel() != C):
        raise ValueError("norm affine parameters must have C entries")
    out, _ = _out_flat(out, x)
    N.check(N.lib().ds_inorm_silu(_p(out), _p(x), _p(w), _p(b), B, C, HW, float(eps), int(kind), _stream()),
            "ds_inorm_silu")
    return out


def circular_axes(circular, ndim):
    """circular= of the convolutions as one bool per spatial axis, in tensor-axis order ((H, W) or (D, H, W)): False, True
    (every axis), or a sequence of ndim bools (circular_dims of CircularConv2d / CircularConv3d, commonlayers.py:918-1034)."""
    if not hasattr(circular, "__iter__"):
        return (bool(circular),) * ndim
    axes = tuple(bool(a) for a in circular)
    if len(axes) != ndim:
        raise ValueError(f"circular: one flag per spatial axis ({ndim}: {'(D, H, W)' if ndim == 3 else '(H, W)'}); got {len(axes)}")
    return axes


def pad_word(circular, ndim):
    """The padding bits of a load_mode / flags word (include/diffsci_hip.h) for circular= (see circular_axes): 0 when no axis is
    periodic, DS_PAD_CIRCULAR when all are, and DS_PAD_CIRCULAR with a DS_PAD_ZERO_* bit for every axis that stays zero-padded.
    Pure: no library call."""
    axes = circular_axes(circular, ndim)
    if not any(axes):
        return 0
    zero = (N.DS_PAD_ZERO_D, N.DS_PAD_ZERO_H, N.DS_PAD_ZERO_W)[3 - ndim:]
    return N.DS_PAD_CIRCULAR | sum(z for a, z in zip(axes, zero) if not a)


def conv3d(x, w, bias=None, shift=None, res1=None, res2=None, load_mode=N.DS_LOAD_PLAIN, circular=False, out=None):
    """3x3x3 'same' convolution of a volume [B, Cin, Di, Hi, Wi] with raw torch weights [Cout, Cin, 3, 3, 3], exact
    fp32; MaxPool3d(2) / nearest x2 upsampling fused in the loader; shift [1 or B, Cout].  circular: False, True or
    (D, H, W) flags (circular_axes)."""
    pad = pad_word(circular, 3)
    require_device(x, "x")
    B, Cin, Di, Hi, Wi = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, Cin, 3, 3, 3):
        raise ValueError(f"conv3d: weight must be [Cout, {Cin}, 3, 3, 3]; got {tuple(w.shape)}")
    D, H, W = _load_sides(load_mode, (Di, Hi, Wi))
    out = _out(out, (B, Cout, D, H, W), x)
    stride = _row_stride(shift, B, Cout, _SHIFT_MSG)
    _residuals((B, Cout, D, H, W), res1, res2)
    _entries(bias, Cout, "bias must have Cout entries")
    N.check(N.lib().ds_conv3d_direct(_p(out), _p(x.contiguous()), _p(w.contiguous()), _p(bias), _p(shift), stride, _p(res1),
                                     _p(res2), B, Cin, Cout, D, H, W,
                                     load_mode | pad, _stream()), "ds_conv3d_direct")
    return out


def pack_conv3d(w, upsampled=False):
    """A k x k x k weight [Cout, Cin, k, k, k] (k = 1, 3, 5, 7) as k fp16x3-packed k x k weights, one per depth tap (see
    conv3d_mfma); the parity kernels of a nearest-x2 upsampled input (upsampled) exist for k = 3."""
    k = w.shape[2] if w.dim() == 5 else 0
    if w.dim() != 5 or tuple(w.shape[2:]) != (k, k, k) or k not in (1, 3, 5, 7):
        raise ValueError("pack_conv3d: weight must be [Cout, Cin, k, k, k] with k in (1, 3, 5, 7)")
    return [pack_conv(w[:, :, kz].contiguous(), "fp16x3", upsampled=upsampled and k == 3) for kz in range(k)]


def volume_stat_tiles(D, HW):
    """Entries per (sample, channel) of the statistics ds_slices_to_volume_stats leaves for a [.., D, H, W] volume."""
    return N.lib().ds_volume_stat_tiles(int(D), int(HW))


def _slice_rows(shift, B, D, Cout, scratch, pad=1):
    """Per-slice rows of a per-sample time shift for the 2-D batch of all slices but the outermost `pad` on each end.  The
    expansion lands in a buffer of `scratch` (with a pool: a captured loop must not allocate)."""
    if not _row_stride(shift, B, Cout, _SHIFT_MSG):
        return shift
    DP = D + 2 * pad
    ns = B * DP
    if scratch.ws is None:
        return shift.repeat_interleave(DP, dim=0)[pad:ns - pad].contiguous()
    buf = scratch.take((B, DP, Cout))
    buf.copy_(shift[:, None, :].expand(B, DP, Cout))
    return buf.view(ns, Cout)[pad:ns - pad]


def _depth_taps(s_in, s_out, packs, bias, rows, load_mode, circular, prenorm=None, tile_stats=None, in_amax=None):
    """The depth-tap launches of a k x k x k convolution over slice-major volumes (k = len(packs); three for 3x3x3): the centre
    tap initialises the accumulator (all slices of s_out but the outermost k/2 on each end), the others add to it; prenorm:
    per-SLICE table [B*(D+2), ceil16(Cin), 4] (ds_slice_tables) for the fused norm + SiLU loader; tile_stats: filled by the last
    launch.  in_amax: per-SLICE max |s_in| [B*(D+2 pad)] (every slice is a 2-D sample with its own exponent), NORMALISED, or
    None = computed here.  circular: the PLANE's padding, False, True or (H, W) flags; the depth is the pad slices' business."""
    ns = s_in.shape[0]
    P = len(packs) // 2
    acc = s_out[P:ns - P]
    if prenorm is not None:
        in_amax = NORMALISED
    elif in_amax is None:
        in_amax = absmax_rows(s_in)
    order = [0] + [d for q in range(1, P + 1) for d in (-q, q)]
    for n, dz in enumerate(order):
        conv(s_in[P + dz:ns - P + dz], packs[dz + P], bias=bias if n == 0 else None, shift=rows if n == 0 else None,
             res1=None if n == 0 else acc, load_mode=load_mode, circular=circular, out=acc,
             prenorm=None if prenorm is None else prenorm[P + dz:ns - P + dz], tile_stats=tile_stats if n == len(order) - 1 else None,
             in_amax=in_amax if in_amax is NORMALISED else in_amax[P + dz:ns - P + dz])
    return acc


def _from_slices(out, s_out, res1, res2, B, C, D, HW, out_stats=None, pad=1):
    if out_stats is None:
        N.check(N.lib().ds_slices_to_volume(_p(out), _p(s_out), _p(res1), _p(res2), B, C, D, HW, int(pad), _stream()),
                "ds_slices_to_volume")
    else:
        if tuple(out_stats.shape) != (B, C, volume_stat_tiles(D, HW), 4):
            raise ValueError(f"out_stats must be {(B, C, volume_stat_tiles(D, HW), 4)}")
        N.check(N.lib().ds_slices_to_volume_stats(_p(out), _p(s_out), _p(res1), _p(res2), _p(out_stats), B, C, D, HW, int(pad),
                                                  _stream()), "ds_slices_to_volume_stats")
    return out


def resblock3d_fused(h, tab1, packs1, bias1, shift, packs2, bias2, w2, b2, kind2, res2=None, out=None, out_stats=None,
                     ws=None, eps=1e-5, circular=False):
    """ResnetBlockC on a volume (commonlayers.py:824-833) with both norms folded and the intermediate kept slice-major:
        S1 = SiLU(norm1(h))         by the volume -> slice copy (tab1 = ds_inorm_table rows of h's statistics)
        S2 = conv1(S1) + shift      three depth-tap launches; the last one leaves S2's tile statistics
        T  = per-slice table of norm2 over the sample's real slices, zero rows for the pad slices (ds_slice_tables)
        S3 = conv2(SiLU(norm2(S2))) three launches with the fused loader reading S2 in place
        out = S3 + h [+ res2]       by the slice -> volume copy, which also leaves out's statistics (out_stats)
    against norm, copy, 3 launches, copy, norm, copy, 3 launches, copy.  Plain loads, fp16x3 packings.  circular: periodic
    padding on all three axes, or (D, H, W) flags (commonlayers.py:918-1034) -- in the plane by the convolution's loader, along the depth by pad
    slices that hold wrapped copies: S1's from the volume -> slice copy, S2's from one small copy after conv1 (the pad rows of T
    are then the sample's row, not zeros)."""
    wrap_d, *plane = circular_axes(circular, 3)
    plane = tuple(plane)
    require_device(h, "h")
    B, C, D, H, W = h.shape
    if packs1[0].Cout != C or packs2[0].Cout != C:
        raise ValueError("resblock3d_fused keeps the channel count")
    ns, scratch = B * (D + 2), _Scratch(ws, h.device)
    out = _out(out, (B, C, D, H, W), h)
    _residuals((B, C, D, H, W), res2)
    if tuple(tab1.shape) != (B, table_channels(C), 4):
        raise ValueError(f"tab1 must be {(B, table_channels(C), 4)}; got {tuple(tab1.shape)}")
    _affine(w2, b2, C, "resblock3d_fused")
    s1 = scratch.take((ns, C, H, W))
    circ = 1 if wrap_d else 0
    N.check(N.lib().ds_volume_to_slices_act(_p(s1), _p(h.contiguous()), _p(tab1), B, C, D, H * W, circ, _stream()),
            "ds_volume_to_slices_act")
    s2 = scratch.take((ns, C, H, W))
    if not wrap_d:
        s2[0].zero_()                                       # the outermost pad slices are never written by the launches
        s2[ns - 1].zero_()
    ts = scratch.take((ns - 2, C, conv_tile_count(H, W), 4))
    rows = _slice_rows(shift, B, D, C, scratch)
    _depth_taps(s1, s2, packs1, bias1, rows, N.DS_LOAD_PLAIN, plane, tile_stats=ts, in_amax=NORMALISED)   # S1 = SiLU(norm1(h))
    if wrap_d:
        N.check(N.lib().ds_wrap_pad_slices(_p(s2), B, C, D, H * W, _stream()), "ds_wrap_pad_slices")
    tab2 = scratch.take((ns, table_channels(C), 4))
    N.check(N.lib().ds_slice_tables(_p(tab2), _p(ts), _p(w2), _p(b2), B, C, D, ts.shape[2], D * H * W, float(eps), int(kind2),
                                    circ, _stream()), "ds_slice_tables")
    _depth_taps(s2, s1, packs2, bias2, None, N.DS_LOAD_PLAIN, plane, prenorm=tab2)  # S1 is dead: reuse it for S3
    _from_slices(out, s1, h, res2, B, C, D, H * W, out_stats)
    scratch.give()
    return out


def conv3d_mfma(x, packs, bias=None, shift=None, res1=None, res2=None, load_mode=N.DS_LOAD_PLAIN, circular=False, out=None,
                ws=None, out_stats=None, in_amax=None):
    """k x k x k 'same' convolution of a volume on the matrix cores (k = len(packs): 1, 3, 5, 7): k 2-D fp16x3 convolutions
    (one per depth tap; each a sum of shifted 3 x 3 blocks when k > 3) over a slice-major copy of the volume padded by k/2
    slices in depth (ds_volume_to_slices / ds_slices_to_volume).  Same arguments and
    fusions as conv3d; packs = pack_conv3d(weight).  ws: an optional buffer pool (take(shape, device) / give(tensor)) for
    the two slice copies, so that a captured loop allocates nothing.  out_stats: [B, Cout, volume_stat_tiles(D, H*W), 4],
    filled with the result's shifted partial sums (the consumer's norm table, ds_inorm_table with count D*H*W).
    in_amax: NORMALISED for a norm + SiLU output; otherwise the per-slice activation exponents are taken from a reduction over the
    slice copy (in a pool buffer when ws is given).  circular: False, True or (D, H, W) flags (circular_axes): the depth flag fills
    the pad slices with wrapped neighbours instead of zeros, the other two go to the 2-D launches."""
    wrap_d, *plane = circular_axes(circular, 3)
    require_device(x, "x")
    B, Cin, Din, Hi, Wi = x.shape
    Cout = packs[0].Cout
    D, H, W = _load_sides(load_mode, (Din, Hi, Wi))
    depth_mode = {N.DS_LOAD_MAXPOOL2: 1, N.DS_LOAD_UPSAMPLE2: 2}.get(load_mode, 0)
    out = _out(out, (B, Cout, D, H, W), x)
    _residuals((B, Cout, D, H, W), res1, res2)
    P = len(packs) // 2
    if wrap_d and P > D:
        raise ValueError(f"periodic padding of {P} slices needs a depth of at least {P}; got {D}")
    ns, scratch = B * (D + 2 * P), _Scratch(ws, x.device)
    s_in = scratch.take((ns, Cin, Hi, Wi))
    N.check(N.lib().ds_volume_to_slices(_p(s_in), _p(x.contiguous()), B, Cin, D, Hi * Wi, depth_mode, 1 if wrap_d else 0, P,
                                        _stream()), "ds_volume_to_slices")
    s_out = scratch.take((ns, Cout, H, W))
    rows = _slice_rows(shift, B, D, Cout, scratch, pad=P)
    if in_amax is not NORMALISED:
        in_amax = absmax_rows(s_in, out=scratch.amax(ns))
    _depth_taps(s_in, s_out, packs, bias, rows, load_mode, tuple(plane), in_amax=in_amax)
    _from_slices(out, s_out, res1, res2, B, Cout, D, H * W, out_stats, pad=P)
    scratch.give()
    return out


def avgpool3d(x, out=None):
    """AvgPool3d(2) of a volume [B, C, 2D, 2H, 2W]."""
    require_device(x, "x")
    B, C, Di, Hi, Wi = x.shape
    if Di % 2 or Hi % 2 or Wi % 2:
        raise ValueError("avgpool3d needs even D, H, W")
    out = _out(out, (B, C, Di // 2, Hi // 2, Wi // 2), x)
    N.check(N.lib().ds_avgpool3d(_p(out, "out"), _p(x, "x"), B * C, Di // 2, Hi // 2, Wi // 2, _stream()), "ds_avgpool3d")
    return out


def upsample3d(x, out=None):
    """Nearest x2 upsampling of a volume [B, C, D, H, W]."""
    require_device(x, "x")
    B, C, Di, Hi, Wi = x.shape
    out = _out(out, (B, C, 2 * Di, 2 * Hi, 2 * Wi), x)
    N.check(N.lib().ds_upsample3d(_p(out, "out"), _p(x, "x"), B * C, Di, Hi, Wi, _stream()), "ds_upsample3d")
    return out


def _factor(factor):
    import operator
    try:
        f = operator.index(factor)                   # ints and integer numpy scalars; floats and bools refused below
    except TypeError:
        f = None
    if f is None or isinstance(factor, bool) or f < 1:
        raise ValueError(f"resampling factor {factor!r} must be an integer >= 1")
    return f


def gnorm1_apply_poolf(x, stats, w, b, kind, factor, film=None, out=None):
    """gnorm1_apply followed by AvgPool2d(factor) for any integer factor >= 1 (floor output size, as torch):
    x [B, C, H, W] -> [B, C, H // f, W // f].  kind 2 pools the raw x."""
    f = _factor(factor)
    require_device(x, "x")
    B, C, H, W = x.shape
    if f > min(H, W):
        raise ValueError(f"pooling factor {f} exceeds the field {H}x{W}")
    out = _out(out, (B, C, H // f, W // f), x)
    f1, f2, stride = _film_args(film, B, C)
    _gnorm1_inputs(stats, w, b, B, C, "gnorm1_apply_poolf")
    N.check(N.lib().ds_gnorm1_apply_poolf(_p(out), _p(x), _p(stats), _p(w), _p(b), f1, f2, stride, B, C, H, W, int(kind), f,
                                          _stream()), "ds_gnorm1_apply_poolf")
    return out


def avgpool_f(x, factor, out=None):
    """AvgPool2d / AvgPool3d(kernel_size=factor) of a field [B, C, H, W] or a volume [B, C, D, H, W], any integer factor >= 1
    (stride = factor, no padding, floor output size)."""
    f = _factor(factor)
    require_device(x, "x")
    if x.dim() == 4:
        return gnorm1_apply_poolf(x, None, None, None, 2, f, out=out)
    if x.dim() != 5:
        raise ValueError("avgpool_f takes [B, C, H, W] fields or [B, C, D, H, W] volumes")
    B, C, Di, Hi, Wi = x.shape
    if f > min(Di, Hi, Wi):
        raise ValueError(f"pooling factor {f} exceeds the volume {Di}x{Hi}x{Wi}")
    shape = (B, C, Di // f, Hi // f, Wi // f)
    out = _out(out, shape, x)
    N.check(N.lib().ds_avgpool3d_f(_p(out, "out"), _p(x, "x"), B * C, Di, Hi, Wi, f, _stream()), "ds_avgpool3d_f")
    return out


def upsample_f(x, factor, out=None):
    """Upsample(scale_factor=factor, mode='nearest') of a field [B, C, H, W] or a volume [B, C, D, H, W], any integer
    factor >= 1: out[..., y, x] = x[..., y // f, x // f] (and z // f on volumes)."""
    f = _factor(factor)
    require_device(x, "x")
    if x.dim() not in (4, 5):
        raise ValueError("upsample_f takes [B, C, H, W] fields or [B, C, D, H, W] volumes")
    vol = x.dim() == 5
    B, C = x.shape[:2]
    Di, Hi, Wi = (x.shape[2:] if vol else (1,) + tuple(x.shape[2:]))
    shape = (B, C) + ((f * Di,) if vol else ()) + (f * Hi, f * Wi)
    out = _out(out, shape, x)
    N.check(N.lib().ds_upsample_f(_p(out, "out"), _p(x, "x"), B * C, Di, Hi, Wi, f, 1 if vol else 0, _stream()),
            "ds_upsample_f")
    return out


def maxpool_f(x, factor, out=None):
    """MaxPool2d / MaxPool3d(kernel_size=factor) of a field [B, C, H, W] or a volume [B, C, D, H, W], any integer factor >= 1
    (stride = factor, no padding, floor output size), bit-identical to torch (NaN windows give NaN)."""
    f = _factor(factor)
    if x.dim() not in (4, 5):
        raise ValueError("maxpool_f takes [B, C, H, W] fields or [B, C, D, H, W] volumes")
    require_device(x, "x")
    vol = x.dim() == 5
    B, C = x.shape[:2]
    sides = tuple(x.shape[2:])
    if f > min(sides):
        raise ValueError(f"pooling factor {f} exceeds the {'volume' if vol else 'field'} {'x'.join(map(str, sides))}")
    Di, Hi, Wi = sides if vol else (1,) + sides
    shape = (B, C) + tuple(v // f for v in sides)
    out = _out(out, shape, x)
    N.check(N.lib().ds_maxpool_f(_p(out, "out"), _p(x, "x"), B * C, Di, Hi, Wi, f, 1 if vol else 0, _stream()), "ds_maxpool_f")
    return out


def cornerpool_f(x, factor, te=None, out=None, out_amax=None):
    """CornerPool2d / CornerPool3d(factor) of a field [Bx, C, H, W] or a volume [Bx, C, D, H, W] (the top-left corner of every
    window), plus a per-(sample, channel) addend: out[b, c, o] = x[b or 0, c, o * f] (+ te[b or 0, c]), bit-identical to
    x[..., ::f, ::f(, ::f)] + te[:, :, None, ...].  Any integer factor >= 1; every side must divide by it.  x and te [1 or B, C]
    broadcast over the batch B (that of `out` when given, else the larger of the two).  out_amax: zeroed int32 [B] slots that
    receive the per-sample max |out| (float bits, merged as absmax_rows does).  Shapes are checked before anything is launched."""
    f = _factor(factor)
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise ValueError("cornerpool_f takes [B, C, H, W] fields or [B, C, D, H, W] volumes")
    vol = x.dim() == 5
    Bx, C = x.shape[:2]
    sides = tuple(x.shape[2:])
    if any(v % f for v in sides):
        raise ValueError(f"every side of the {'volume' if vol else 'field'} {'x'.join(map(str, sides))} must divide by the "
                         f"factor {f}")
    if te is not None and (te.dim() != 2 or te.shape[1] != C):
        raise ValueError(f"te must be [1 or B, {C}]; got {tuple(te.shape)}")
    B = out.shape[0] if out is not None else max(Bx, 1 if te is None else te.shape[0])
    if Bx not in (1, B) or (te is not None and te.shape[0] not in (1, B)):
        raise ValueError(f"x {tuple(x.shape)} and te {None if te is None else tuple(te.shape)} must have batch 1 or {B}")
    shape = (B, C) + tuple(v // f for v in sides)
    if out is not None:
        _out(out, shape, x)
    require_device(x, "x")
    out = _out(out, shape, x)
    Di, Hi, Wi = sides if vol else (1,) + sides
    N.check(N.lib().ds_cornerpool_f(_p(out, "out"), _p(x, "x"), _p(te, "te"), _pi(out_amax, B, "out_amax"), B, C, Di, Hi, Wi, f,
                                    1 if vol else 0, Bx, 1 if te is None else te.shape[0], _stream()), "ds_cornerpool_f")
    return out


def gnorm1_stats(x, kind, eps=1e-5, stats=None, workspace=None):
    """Per-sample (mean, rstd) [kind 0] or (0, rms denominator) [kind 1] over (C, H, W)."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1)
    workspace = _workspace(workspace, N.lib().ds_gnorm1_workspace_bytes(B), x, "gnorm1 workspace too small")
    stats = _out(stats, (B, 2), x, _STATS_MSG)
    N.check(N.lib().ds_gnorm1_stats(_p(stats), _p(workspace), _p(x), B, C, HW, float(eps), int(kind), _stream()),
            "ds_gnorm1_stats")
    return stats


def gnorm1_apply(x, stats, w, b, kind, pool=False, film=None, out=None):
    """kind 0: GroupNorm(1, C), kind 1: GroupRMSNorm(1, C), each followed by FiLM when `film` is given, then SiLU;
    kind 2: identity; then optional 2x2 average pooling.  film: [1 or B, 2C] rows of embed_linear(te)."""
    B, C, H, W = x.shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    f1, f2, stride = _film_args(film, B, C)
    _gnorm1_inputs(stats, w, b, B, C, "gnorm1_apply")
    out = _out(out, (B, C, Ho, Wo), x)
    N.check(N.lib().ds_gnorm1_apply(_p(out), _p(x), _p(stats), _p(w), _p(b), f1, f2, stride, B, C, H, W, int(kind),
                                    1 if pool else 0, _stream()), "ds_gnorm1_apply")
    return out


# ---------------------------------------------------------------- GroupNorm(G, C) with several channels per group (ds_groupnorm.hip)
def _groupnorm_dims(x, G, what):
    require_device(x, "x")
    if x.dim() < 3:
        raise ValueError(f"{what}: x must be [B, C, *spatial]")
    B, C = x.shape[0], x.shape[1]
    return B, C, _groups(C, G, what), x.numel() // max(B * C, 1)


def groupnorm_stats(x, G, eps=1e-6, stats=None, workspace=None):
    """(mean, rstd) [B, G, 2] of GroupNorm(G, C) over x [B, C, *spatial] (biased variance, fp64 accumulation)."""
    B, C, G, n = _groupnorm_dims(x, G, "groupnorm_stats")
    stats = _out(stats, (B, G, 2), x, _STATS_MSG)
    workspace = _workspace(workspace, N.lib().ds_gnorm1_workspace_bytes(B * G), x, "groupnorm workspace too small")
    N.check(N.lib().ds_groupnorm_stats(_p(stats, "stats"), _p(workspace, "workspace"), _p(x, "x"), B, C, G, n, float(eps), _stream()),
            "ds_groupnorm_stats")
    return stats


def groupnorm_apply(x, stats, w, b, G, act=False, out=None, out_amax=None):
    """(x - mean[b,g]) * rstd[b,g] * w[c] + b[c], then SiLU when act; x [B, C, *spatial], stats [B, G, 2].  out_amax: zeroed
    int32 [B] slots that receive the per-sample max |out| (as conv2d's)."""
    B, C, G, n = _groupnorm_dims(x, G, "groupnorm_apply")
    if tuple(stats.shape) != (B, G, 2):
        raise ValueError(f"stats must be {(B, G, 2)}; got {tuple(stats.shape)}")
    _affine(w, b, C, "groupnorm_apply")
    out = _out(out, x.shape, x, "groupnorm_apply: out must have x's shape")
    N.check(N.lib().ds_groupnorm_apply(_p(out, "out"), _p(x, "x"), _p(stats, "stats"), _p(w, "weight"), _p(b, "bias"), B, C, G, n,
                                       1 if act else 0, _pi(out_amax, B, "out_amax"), _stream()), "ds_groupnorm_apply")
    return out


def groupnorm_stats_tiles(tile_stats, G, count, eps=1e-6, stats=None):
    """groupnorm_stats [B, G, 2] from the tile statistics [B, C, ntiles, 4] of the tensor's producing convolution instead of
    a pass over the tensor; count: positions per channel."""
    require_device(tile_stats, "tile_stats")
    B, C, nt, _ = tile_stats.shape
    G = _groups(C, G, "groupnorm_stats_tiles")
    stats = _out(stats, (B, G, 2), tile_stats, _STATS_MSG)
    N.check(N.lib().ds_groupnorm_stats_tiles(_p(stats, "stats"), _p(tile_stats, "tile_stats"), B, C, G, nt, int(count), float(eps),
                                             _stream()), "ds_groupnorm_stats_tiles")
    return stats


def groupnorm_table(w, b, G, count, tile_stats=None, stats=None, eps=1e-6, out=None):
    """GroupNorm(G, C) + SiLU as the prenorm table [B, ceil16(C), 4] of the consuming 3x3 fp16x3 convolution (rows as
    inorm_table), from the producer's tile_stats [B, C, ntiles, 4] or from plain stats [B, G, 2]; count: positions per channel."""
    if (tile_stats is None) == (stats is None):
        raise ValueError("groupnorm_table: give tile_stats or stats")
    G = int(G)
    if tile_stats is not None:
        require_device(tile_stats, "tile_stats")
        B, C, nt, _ = tile_stats.shape
    else:
        require_device(stats, "stats")
        if w is None or stats.dim() != 3 or tuple(stats.shape[1:]) != (G, 2):
            raise ValueError("groupnorm_table: stats must be [B, G, 2] and the weight gives the channel count")
        B, C, nt = stats.shape[0], w.numel(), 0
    G = _groups(C, G, "groupnorm_table")
    _affine(w, b, C, "groupnorm_table")
    out = _out(out, (B, table_channels(C), 4), tile_stats if stats is None else stats, _TABLE_MSG)
    N.check(N.lib().ds_groupnorm_table(_p(out, "table"), _p(tile_stats, "tile_stats"), _p(stats, "stats"), _p(w, "weight"), _p(b, "bias"),
                                       B, C, G, nt, int(count), float(eps), _stream()), "ds_groupnorm_table")
    return out


def tanh(x, out=None):
    """tanh(x), any shape."""
    require_device(x, "x")
    if x.numel() >= 1 << 31:
        raise ValueError("tanh: at most 2^31 - 1 elements")
    out, n = _out_flat(out, x)
    N.check(N.lib().ds_add_act(_p(out, "out"), _p(x, "x"), None, 0, 1, n, 3, _stream()), "ds_add_act")
    return out


def concat2(a, b, out=None):
    """cat([a, b], dim=1) for [B, C, H, W] tensors."""
    B = a.shape[0]
    na, nb = a.numel() // max(B, 1), b.numel() // max(B, 1)
    # the kernel appends nb floats of b to na floats of a per sample: the same batch and the same spatial sides, axes of length
    # one aside (PUNetGCond hands in [B, C, 1, H, W] fields next to a [B, C, H, W] input)
    if a.dim() < 2 or b.dim() < 2 or b.shape[0] != B or [n for n in b.shape[2:] if n != 1] != [n for n in a.shape[2:] if n != 1]:
        raise ValueError(f"concat2: a {tuple(a.shape)} and b {tuple(b.shape)} must agree in all but the channel axis")
    out = _out(out, (B, a.shape[1] + b.shape[1]) + tuple(a.shape[2:]), a)
    N.check(N.lib().ds_concat2(_p(out), _p(a), _p(b), B, na, nb, _stream()), "ds_concat2")
    return out


def add_act(a, add=None, act=0, out=None):
    M, Nn = a.shape
    rows = 0
    if add is not None:
        add = add.reshape(-1, Nn)
        rows = add.shape[0]
    out, _ = _out_flat(out, a)
    N.check(N.lib().ds_add_act(_p(out), _p(a), _p(add), rows, M, Nn, int(act), _stream()), "ds_add_act")
    return out


def pack_conv_weight(w):
    """torch [Cout, Cin, k, k] (device, fp32) -> packed MFMA operand stream."""
    require_device(w, "conv weight")
    Cout, Cin, k, k2 = w.shape
    if k != k2 or k not in (1, 3):
        raise NotImplementedError(f"conv kernel {k}x{k2}: only 1x1 and 3x3 are implemented")
    n = N.lib().ds_conv2d_packed_floats(Cout, Cin, k)
    packed = torch.empty(n, dtype=torch.float32, device=w.device)
    N.check(N.lib().ds_conv2d_pack_weights(_p(packed), _p(w.contiguous()), Cout, Cin, k, _stream()),
            "ds_conv2d_pack_weights")
    return packed


class PackedConv:
    """A convolution weight repacked for one of the MFMA kernels.
    kind: "fp32" (exact-fp32 MFMA), "bf16x6" or "fp16x3" (fp32 emulated on the 16-bit matrix cores)."""
    __slots__ = ("data", "Cout", "Cin", "ks", "kind", "wshift", "up", "up_wshift", "subs")

    def __init__(self, data, Cout, Cin, ks, kind, wshift=0, up=None, up_wshift=0, subs=None):
        self.data, self.Cout, self.Cin, self.ks, self.kind, self.wshift = data, Cout, Cin, ks, kind, wshift
        # fp16x3 3x3 only: the four 2x2 parity kernels of "upsample x2, then this convolution" and their scale
        self.up, self.up_wshift = up, up_wshift
        # ks = 5, 7, ...: the kernel as ceil(ks/3)^2 zero-padded 3x3 blocks [(oy, ox, PackedConv 3x3)], see conv()
        self.subs = subs

    @property
    def x6(self):
        return self.kind == "bf16x6"


CONV_PRECISIONS = ("fp16x3", "bf16x6", "fp32")


def pack_conv(w, precision="bf16x6", upsampled=False):
    """Repack a torch conv weight [Cout, Cin, k, k] (device, fp32).  3x3 kernels honour
    `precision`; 1x1 kernels use the fp16x3 kernel for "fp16x3" and the exact-fp32 MFMA kernel otherwise.
    upsampled: the convolution follows a nearest x2 upsampling; the fp16x3 packing then also carries the
    collapsed parity kernels of ds_conv2d_h3_up."""
    require_device(w, "conv weight")
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"unknown conv precision {precision!r}; choose from {CONV_PRECISIONS}")
    Cout, Cin, k, k2 = w.shape
    w = w.contiguous()
    if k != k2 or k % 2 == 0:
        raise NotImplementedError(f"conv kernel {k}x{k2}: square kernels of odd size are implemented")
    if k > 3:
        # k x k = sum of ceil(k/3)^2 shifted 3x3 convolutions over blocks of the taps (DS_TAP_OFFSET).  Block g starts at tap
        # min(3g, k - 3) -- the last block is pulled back inside the kernel, its taps already served by the previous block zeroed --
        # so no block reaches further out than the kernel itself does (k // 2 pixels: what periodic padding can wrap on a plane
        # that small); its centre tap start + 1 sits at offset start + 1 - k // 2
        if precision != "fp16x3":
            raise NotImplementedError(f"{k}x{k} kernels are implemented on the fp16x3 convolution only (conv_precision={precision!r})")
        ng = (k + 2) // 3
        starts = [min(3 * g, k - 3) for g in range(ng)]
        subs = []
        for gy, sy in enumerate(starts):
            for gx, sx in enumerate(starts):
                blk = w[:, :, sy:sy + 3, sx:sx + 3].clone()
                blk[:, :, :3 * gy - sy, :] = 0
                blk[:, :, :, :3 * gx - sx] = 0
                subs.append((sy + 1 - k // 2, sx + 1 - k // 2, pack_conv(blk.contiguous(), "fp16x3")))
        return PackedConv(None, Cout, Cin, k, "fp16x3", subs=subs)
    if precision == "bf16x6" and k == 3:
        nbytes = N.lib().ds_conv2d_x6_packed_bytes(Cout, Cin)
        data = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        N.check(N.lib().ds_conv2d_x6_pack_weights(data.data_ptr(), _p(w), Cout, Cin, _stream()),
                "ds_conv2d_x6_pack_weights")
        return PackedConv(data, Cout, Cin, 3, "bf16x6")
    if precision == "fp16x3" and k in (1, 3):
        # per-layer power-of-two scale: largest weight lands in [2^13, 2^14), far inside fp16's
        # range, and typical weights get normal (not subnormal) low pieces
        wmax = float(w.abs().max())
        wshift = 0
        if wmax > 0 and wmax == wmax and wmax != float("inf"):
            import math
            wshift = max(-40, min(40, 13 - math.floor(math.log2(wmax))))
        size_fn, pack_fn = ((N.lib().ds_conv2d_h3_packed_bytes, N.lib().ds_conv2d_h3_pack_weights) if k == 3 else
                            (N.lib().ds_conv1x1_h3_packed_bytes, N.lib().ds_conv1x1_h3_pack_weights))
        data = torch.empty(size_fn(Cout, Cin) // 4, dtype=torch.float32, device=w.device)
        N.check(pack_fn(data.data_ptr(), _p(w), Cout, Cin, wshift, _stream()), "ds_conv*_h3_pack_weights")
        up, up_wshift = None, 0
        if upsampled and k == 3:
            up_wshift = max(-40, wshift - 2)          # a collapsed tap sums up to four weights: two bits of headroom
            up = torch.empty(N.lib().ds_conv2d_h3_up_packed_bytes(Cout, Cin) // 4, dtype=torch.float32, device=w.device)
            N.check(N.lib().ds_conv2d_h3_up_pack_weights(up.data_ptr(), _p(w), Cout, Cin, up_wshift, _stream()),
                    "ds_conv2d_h3_up_pack_weights")
        return PackedConv(data, Cout, Cin, k, "fp16x3", wshift, up, up_wshift)
    return PackedConv(pack_conv_weight(w), Cout, Cin, k, "fp32")


class PoolOut:
    """A place for MaxPool2d(2) of a convolution's result (conv2d / conv_img, pool=): tensor [B, Cout, H/2, W/2]; written is set by
    the call -- True when the launch was one the persistent 3x3 kernel takes in its pooled form and the tensor holds the pooled
    result, False when it was left untouched (the caller pools by other means).  The answer depends on shapes and switches only,
    so it is the same at capture and at replay."""

    def __init__(self, tensor):
        self.tensor, self.written = tensor, False


def _pool_out(pool, B, Cout, H, W, like):
    if pool is None:
        return None
    if H % 2 or W % 2:
        raise ValueError(f"pool: the convolution's output must have even sides; got {H}x{W}")
    pool.written = False
    return _out(pool.tensor, (B, Cout, H // 2, W // 2), like)


def conv(x, pw, **kw):
    """Dispatch on the packing: ds_conv2d_h3, ds_conv2d_x6 or ds_conv2d; kernels larger than 3x3 as a sum of shifted
    3x3 blocks accumulated in place (the first launch carries bias / shift / residuals, the last one the statistics)."""
    if pw.subs is None:
        return conv2d(x, pw.data, pw.Cout, pw.ks, kind=pw.kind, wshift=pw.wshift, w_up=pw.up, up_wshift=pw.up_wshift, **kw)
    if kw.get("res1_upsampled", False):
        raise NotImplementedError("res1_upsampled with kernels larger than 3x3")
    if kw.pop("pool", None) is not None or kw.pop("pc_raw", False):
        raise NotImplementedError("pool / pc_raw with kernels larger than 3x3")
    stats, out, out_amax = kw.pop("tile_stats", None), kw.pop("out", None), kw.pop("out_amax", None)
    first = dict(bias=kw.pop("bias", None), shift=kw.pop("shift", None), res1=kw.pop("res1", None), res2=kw.pop("res2", None))
    if kw.get("in_amax", None) is None and kw.get("prenorm", None) is None:
        kw["in_amax"] = absmax_rows(x)                                # one reduction for all the blocks
    n = len(pw.subs)
    for i, (oy, ox, sub) in enumerate(pw.subs):
        extra = first if i == 0 else dict(res1=out)
        out = conv2d(x, sub.data, sub.Cout, 3, kind="fp16x3", wshift=sub.wshift, tap_offset=(oy, ox), out=out,
                     tile_stats=stats if i == n - 1 else None, out_amax=out_amax if i == n - 1 else None, **extra, **kw)
    return out


def conv_direct(x, w, bias=None, circular=False, out=None):
    """3x3 'same' convolution with Cout <= 4, exact fp32, raw torch weight layout (output layers).  circular: False, True
    or (H, W) flags (circular_axes)."""
    pad = pad_word(circular, 2)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, Cin, 3, 3):
        raise ValueError("conv_direct: weight must be [Cout, Cin, 3, 3]")
    out = _out(out, (B, Cout, H, W), x)
    _entries(bias, Cout, "bias must have Cout entries")
    N.check(N.lib().ds_conv2d_direct(_p(out), _p(x), _p(w), _p(bias), B, Cin, Cout, H, W,
                                     (pad & ~N.DS_PAD_CIRCULAR) | 1 if pad else 0, _stream()), "ds_conv2d_direct")
    return out


# ---------------------------------------------------------------- stride-2 3x3(x3) convolution, zero pad at the far end (ds_conv_s2.hip)
def _s2_sides(spatial, what):
    if any(int(n) < 2 for n in spatial):
        raise ValueError(f"{what}: the stride-2 convolution needs spatial sides of at least 2; got {tuple(int(n) for n in spatial)}")
    return tuple(int(n) // 2 for n in spatial)


def pack_conv_s2(w, precision="fp16x3"):
    """A Downsample weight [Cout, Cin, 3, 3] for conv_s2: the fp16x3 packing (pack_conv's: the layout is the stride-1 kernel's)
    at precision "fp16x3" when neither channel count is thin (> 4), else the raw weight (kind "direct") for the exact-fp32
    kernel -- the routing of the stride-1 convolutions."""
    require_device(w, "conv weight")
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"unknown conv precision {precision!r}; choose from {CONV_PRECISIONS}")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_conv_s2: weight must be [Cout, Cin, 3, 3]; got {tuple(w.shape)}")
    if precision == "fp16x3" and min(w.shape[0], w.shape[1]) > 4:
        return pack_conv(w, "fp16x3")
    return PackedConv(w.detach().contiguous().clone(), w.shape[0], w.shape[1], 3, "direct")


def conv_s2(x, pw, bias=None, res1=None, in_amax=None, out_amax=None, out=None):
    """out[b,co,i,j] = bias[co] + sum w[co,ci,ky,kx] x[b,ci,2i+ky,2j+kx] (+ res1), x = 0 past the far edge: F.conv2d(F.pad(x,
    (0,1,0,1)), w, b, stride=2); x [B, Cin, H, W] with H, W >= 2 -> [B, Cout, H//2, W//2].  pw = pack_conv_s2(w, precision).
    fp16x3 form: in_amax / out_amax as conv2d's.  No tile statistics are produced."""
    require_device(x, "x")
    if x.dim() != 4 or x.shape[1] != pw.Cin or pw.ks != 3:
        raise ValueError(f"conv_s2: x must be [B, {pw.Cin}, H, W] and the weight 3x3; got {tuple(x.shape)}")
    B, Cin, Hin, Win = x.shape
    H, W = _s2_sides((Hin, Win), "conv_s2")
    out = _out(out, (B, pw.Cout, H, W), x)
    _residuals((B, pw.Cout, H, W), res1)
    _entries(bias, pw.Cout, "bias must have Cout entries")
    x = x.contiguous()
    if pw.kind == "fp16x3":
        pin = _in_amax(x, in_amax, B, raw=True)
        N.check(N.lib().ds_conv2d_s2_h3(_p(out, "out"), _p(x), _p(pw.data), int(pw.wshift), _p(bias), _p(res1), B, Cin, pw.Cout, Hin, Win,
                                        1, 1, 0, pin, _pi(out_amax, B, "out_amax"), _stream()), "ds_conv2d_s2_h3")
    elif pw.kind == "direct":
        N.check(N.lib().ds_conv2d_s2_direct(_p(out, "out"), _p(x), _p(pw.data), _p(bias), _p(res1), B, Cin, pw.Cout, Hin, Win, _stream()),
                "ds_conv2d_s2_direct")
        if out_amax is not None:
            absmax_rows(out, out=out_amax)
    else:
        raise ValueError(f"conv_s2: packing of kind {pw.kind!r}; use pack_conv_s2")
    return out


def pack_conv3d_s2(w, precision="fp16x3"):
    """A Downsample weight [Cout, Cin, 3, 3, 3] for conv3d_s2: three fp16x3 packings, one per depth tap, or the raw weight
    (thin layers, other precisions: the exact-fp32 direct kernel)."""
    require_device(w, "conv weight")
    if precision not in CONV_PRECISIONS:
        raise ValueError(f"unknown conv precision {precision!r}; choose from {CONV_PRECISIONS}")
    if w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"pack_conv3d_s2: weight must be [Cout, Cin, 3, 3, 3]; got {tuple(w.shape)}")
    if precision == "fp16x3" and min(w.shape[0], w.shape[1]) > 4:
        return [pack_conv(w[:, :, kz].contiguous(), "fp16x3") for kz in range(3)]
    return PackedConv(w.detach().contiguous().clone(), w.shape[0], w.shape[1], 3, "direct")


def conv3d_s2(x, packs, bias=None, res1=None, out=None, ws=None):
    """The same on a volume [B, Cin, D, H, W] (sides >= 2) -> [B, Cout, D//2, H//2, W//2]: F.conv3d(F.pad(x, (0,1)*3), w, b,
    stride=2).  packs = pack_conv3d_s2(w, precision).  Matrix-core form, composed as conv3d_mfma: one slice-major copy with a zero
    slice past either end (ds_volume_to_slices), then one 2-D stride-2 launch per depth tap over the batch of OUTPUT slices --
    output slice d of a sample reads its slices 2d + kz, which the launch addresses by a sample stride of two slices, so there is
    no gather pass -- accumulated in place, and the slice -> volume copy (which adds res1).  ws: buffer pool, as conv3d_mfma's."""
    require_device(x, "x")
    direct = isinstance(packs, PackedConv)
    Cin, Cout = (packs.Cin, packs.Cout) if direct else (packs[0].Cin, packs[0].Cout)
    if x.dim() != 5 or x.shape[1] != Cin:
        raise ValueError(f"conv3d_s2: x must be [B, {Cin}, D, H, W]; got {tuple(x.shape)}")
    B, _, Din, Hin, Win = x.shape
    D, H, W = _s2_sides((Din, Hin, Win), "conv3d_s2")
    out = _out(out, (B, Cout, D, H, W), x)
    _residuals((B, Cout, D, H, W), res1)
    _entries(bias, Cout, "bias must have Cout entries")
    x = x.contiguous()
    if direct:
        if packs.kind != "direct":
            raise ValueError("conv3d_s2: use pack_conv3d_s2")
        N.check(N.lib().ds_conv3d_s2_direct(_p(out, "out"), _p(x), _p(packs.data), _p(bias), _p(res1), B, Cin, Cout, Din, Hin, Win,
                                            _stream()), "ds_conv3d_s2_direct")
        return out
    ns, scratch = B * (Din + 2), _Scratch(ws, x.device)
    s_in = scratch.take((ns, Cin, Hin, Win))
    N.check(N.lib().ds_volume_to_slices(_p(s_in), _p(x), B, Cin, Din, Hin * Win, 0, 0, 1, _stream()), "ds_volume_to_slices")
    am = absmax_rows(s_in, out=scratch.amax(ns))
    s_out = scratch.take((B * D, Cout, H, W))
    for kz in range(3):                                  # slice 1 + 2d + kz of the sample's D + 2
        pk = packs[kz]
        N.check(N.lib().ds_conv2d_s2_h3(_p(s_out), s_in[1 + kz].data_ptr(), _p(pk.data), int(pk.wshift), _p(bias) if kz == 0 else None,
                                        None if kz == 0 else _p(s_out), B * D, Cin, Cout, Hin, Win, D, Din + 2, 2,
                                        am.data_ptr() + 4 * (1 + kz), None, _stream()), "ds_conv2d_s2_h3")
    _from_slices(out, s_out, res1, None, B, Cout, D, H * W, pad=0)
    scratch.give()
    return out


def posterior_sample(moments, eps=None, clamp=None, out=None):
    """z = mean + exp(0.5 logvar) eps for moments [B, 2Z, *spatial] = (mean | logvar) -> [B, Z, *spatial]: the draw of
    VAENet.encode (vaenet.py:1244-1248).  clamp = (lo, hi) clamps logvar first (the reference's DiagonalGaussianDistribution uses
    (-30, 20); VAENet none).  eps given: read.  eps=None: drawn inside the kernel by the steppers' Philox stream, seeded from
    torch's CUDA generator -- reproducible from torch.manual_seed, and the generator advances by what the draw consumes.  Under
    stream capture the 16-byte (seed, offset) state is itself drawn on the device from that generator (host code cannot read
    it while capturing), so every replay draws fresh noise."""
    require_device(moments, "moments")
    if moments.dim() < 3 or moments.shape[1] % 2:
        raise ValueError(f"posterior_sample: moments must be [B, 2Z, *spatial]; got {tuple(moments.shape)}")
    moments = moments.contiguous()
    B, Z = moments.shape[0], moments.shape[1] // 2
    shape = (B, Z) + tuple(moments.shape[2:])
    per = moments.numel() // max(2 * B, 1)
    out = _out(out, shape, moments)
    lo, hi, has = 0.0, 0.0, 0
    if clamp is not None:
        lo, hi = (float(v) for v in clamp)
        if not lo <= hi:
            raise ValueError(f"posterior_sample: clamp {clamp!r}")
        has = 1
    if per == 0 or B == 0:
        return out
    state, seed, offset = None, 0, 0
    if eps is not None:
        if tuple(eps.shape) != shape:
            raise ValueError(f"eps has shape {tuple(eps.shape)}, expected {shape}")
        eps = eps.contiguous()
    elif torch.cuda.is_current_stream_capturing():
        state = torch.randint(0, 1 << 62, (2,), dtype=torch.int64, device=moments.device)
    else:
        gen = torch.cuda.default_generators[moments.device.index]
        seed, offset = int(gen.initial_seed()), int(gen.get_offset())
        gen.set_offset(offset + (philox_counters(B * per) + 3) // 4 * 4)          # torch keeps its offset a multiple of 4
    N.check(N.lib().ds_posterior_sample(_p(out, "out"), _p(moments), _p(eps, "eps"), None if state is None else state.data_ptr(),
                                        seed & ((1 << 64) - 1), offset, B, per, has, lo, hi, _stream()), "ds_posterior_sample")
    return out


def _triple(v, what):
    if not isinstance(v, (tuple, list, torch.Size)) or len(v) != 3:
        raise ValueError(f"box_copy3d: {what} must be three integers; got {v!r}")
    return tuple(int(a) for a in v)


def box_copy3d(src, src_start, dst, dst_start, size):
    """dst[..., d0+i, d1+j, d2+k] = src[..., (s0+i) % S0, (s1+j) % S1, (s2+k) % S2] for 0 <= (i, j, k) < size, plane by plane
    (ds_window.hip).  src and dst: contiguous fp32 tensors whose last three axes are the box's and whose leading axes hold the
    same number of planes.  The source is periodic -- a start may be negative and a box longer than the axis -- the destination
    box must lie inside dst.  ValueError before any launch: a non-fp32 tensor, different plane counts, a destination box
    outside dst, src and dst sharing storage.  An empty box launches nothing.  Returns dst."""
    for t, what in ((src, "src"), (dst, "dst")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"box_copy3d: {what} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"box_copy3d: {what} has dtype {t.dtype}; the copy is fp32 only")
        if t.dim() < 3:
            raise ValueError(f"box_copy3d: {what} needs at least three axes; got {tuple(t.shape)}")
    s, d, L = _triple(src_start, "src_start"), _triple(dst_start, "dst_start"), _triple(size, "size")
    S, D = tuple(src.shape[-3:]), tuple(dst.shape[-3:])
    planes = src.numel() // max(S[0] * S[1] * S[2], 1)
    if min(S) < 1 or min(D) < 1:
        raise ValueError(f"box_copy3d: empty spatial axes (src {S}, dst {D})")
    if planes != dst.numel() // (D[0] * D[1] * D[2]):
        raise ValueError(f"box_copy3d: src {tuple(src.shape)} and dst {tuple(dst.shape)} hold different numbers of planes")
    if min(L) < 0 or any(a < 0 or a + n > m for a, n, m in zip(d, L, D)):
        raise ValueError(f"box_copy3d: destination box start {d} size {L} leaves dst {D}")
    if src.untyped_storage().data_ptr() == dst.untyped_storage().data_ptr() and src.numel() and dst.numel():
        raise ValueError("box_copy3d: src and dst share storage")
    if max(S + D) >= 1 << 31 or L[0] * L[1] >= (1 << 31) - (1 << 20) or planes >= 1 << 31:
        raise ValueError(f"box_copy3d: axes beyond 31 bits (src {S}, dst {D}, box {L})")
    ps, pd = _p(src, "src"), _p(dst, "dst")
    if planes == 0 or min(L) == 0:
        return dst
    N.check(N.lib().ds_box_copy3d(pd, ps, planes, S[0], S[1], S[2], s[0], s[1], s[2], D[0], D[1], D[2], d[0], d[1], d[2],
                                  L[0], L[1], L[2], _stream()), "ds_box_copy3d")
    return dst


def box_scatter3d(src, src_start, dst, dst_start, size):
    """dst[..., (d0+i) % D0, (d1+j) % D1, (d2+k) % D2] = src[..., s0+i, s1+j, s2+k] for 0 <= (i, j, k) < size, plane by plane
    (ds_window.hip): the counterpart of box_copy3d with the periodic side the destination (torchutils.py:238-309,
    periodic_setitem).  The source box must lie inside src; a destination start may be negative.  ValueError before any launch:
    what box_copy3d refuses, a source box outside src, and a box longer than a destination axis -- a write of more than one
    period, which periodic_setitem refuses too.  An empty box launches nothing.  Returns dst."""
    for t, what in ((src, "src"), (dst, "dst")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"box_scatter3d: {what} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"box_scatter3d: {what} has dtype {t.dtype}; the copy is fp32 only")
        if t.dim() < 3:
            raise ValueError(f"box_scatter3d: {what} needs at least three axes; got {tuple(t.shape)}")
    s, d, L = _triple(src_start, "src_start"), _triple(dst_start, "dst_start"), _triple(size, "size")
    S, D = tuple(src.shape[-3:]), tuple(dst.shape[-3:])
    if min(S) < 1 or min(D) < 1:
        raise ValueError(f"box_scatter3d: empty spatial axes (src {S}, dst {D})")
    planes = src.numel() // (S[0] * S[1] * S[2])
    if planes != dst.numel() // (D[0] * D[1] * D[2]):
        raise ValueError(f"box_scatter3d: src {tuple(src.shape)} and dst {tuple(dst.shape)} hold different numbers of planes")
    if min(L) < 0 or any(a < 0 or a + n > m for a, n, m in zip(s, L, S)):
        raise ValueError(f"box_scatter3d: source box start {s} size {L} leaves src {S}")
    if any(n > m for n, m in zip(L, D)):
        raise ValueError(f"box_scatter3d: box {L} is longer than a destination axis {D}: a periodic write of more than one period")
    if src.untyped_storage().data_ptr() == dst.untyped_storage().data_ptr() and src.numel() and dst.numel():
        raise ValueError("box_scatter3d: src and dst share storage")
    if max(S + D) >= 1 << 31 or L[0] * L[1] >= (1 << 31) - (1 << 20) or planes >= 1 << 31:
        raise ValueError(f"box_scatter3d: axes beyond 31 bits (src {S}, dst {D}, box {L})")
    ps, pd = _p(src, "src"), _p(dst, "dst")
    if planes == 0 or min(L) == 0:
        return dst
    N.check(N.lib().ds_box_scatter3d(pd, ps, planes, D[0], D[1], D[2], d[0], d[1], d[2], S[0], S[1], S[2], s[0], s[1], s[2],
                                     L[0], L[1], L[2], _stream(), 0), "ds_box_scatter3d")
    return dst


# ---------------------------------------------------------------- DiffusionPeriodizer's two sides (extra/periodizer.py)
def _per_axis(v, n, what, who):
    """pad / blend_width: an int, or one int per spatial axis -> a tuple of n ints."""
    if isinstance(v, bool) or (not isinstance(v, int) and not isinstance(v, (tuple, list, torch.Size))):
        raise TypeError(f"{who}: {what} must be an int or {n} ints; got {v!r}")
    if isinstance(v, int):
        return (v,) * n
    if len(v) != n or any(isinstance(a, bool) or not isinstance(a, int) for a in v):
        raise ValueError(f"{who}: {what} must be an int or {n} ints; got {v!r}")
    return tuple(int(a) for a in v)


def _spatial(t, what, who):
    """A [B, C, *S] tensor of 2 or 3 spatial axes -> (planes, box axes): a field's box is (1, H, W) over B*C planes."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {what} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {what} has dtype {t.dtype}; the HIP path is fp32 only")
    if t.dim() not in (4, 5):
        raise ValueError(f"{who}: {what} must be [B, C, H, W] or [B, C, D, H, W]; got {tuple(t.shape)}")
    S = tuple(t.shape[2:])
    if min(S) < 1:
        raise ValueError(f"{who}: {what} has an empty spatial axis {S}")
    if max(S) >= 1 << 31 or t.shape[0] * t.shape[1] >= 1 << 31:
        raise ValueError(f"{who}: {what} has axes beyond 31 bits {tuple(t.shape)}")
    return t.shape[0] * t.shape[1], S


def periodic_expand(x, pad, out=None):
    """x [B, C, *S] (2 or 3 spatial axes) -> [B, C, *(S + 2 pad)]: x tiled periodically by `pad` cells per side (an int or one per
    axis; longer than the axis spans several periods) -- DiffusionPeriodizer.expand_periodic (periodizer.py:76-101), whose
    periodic_getitem_extended on slice(-p, size + p) is ds_box_copy3d's wrap.  One launch; a field's box is (1, H, W) over B*C
    planes.  out: the result buffer (not sharing bytes with x)."""
    who = "periodic_expand"
    planes, S = _spatial(x, "x", who)
    p = _per_axis(pad, len(S), "pad", who)
    if min(p) < 0:
        raise ValueError(f"{who}: negative pad {p}")
    E = tuple(s + 2 * a for s, a in zip(S, p))
    if max(E) >= 1 << 31:
        raise ValueError(f"{who}: expanded axes beyond 31 bits {E}")
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError(f"{who}: out must be a torch.Tensor")
    out = _out(out, tuple(x.shape[:2]) + E, x)
    if _overlap(x, out):
        raise ValueError(f"{who}: x and out share storage")
    px, po = _p(x, "x"), _p(out, "out")
    if planes == 0:
        return out
    S3, E3, p3 = (1,) * (3 - len(S)) + S, (1,) * (3 - len(S)) + E, (0,) * (3 - len(S)) + p
    if E3[0] * E3[1] >= (1 << 31) - (1 << 20):
        raise ValueError(f"{who}: axes beyond 31 bits {E}")
    N.check(N.lib().ds_box_copy3d(po, px, planes, S3[0], S3[1], S3[2], -p3[0], -p3[1], -p3[2], E3[0], E3[1], E3[2], 0, 0, 0,
                                  E3[0], E3[1], E3[2], _stream()), "ds_box_copy3d")
    return out


_BLEND_WEIGHTS = {}


def blend_weights(blend_width, device):
    """The cosine tables of cosine_blend_boundaries (periodizer.py:160-161), one fp32 tensor of bw floats on `device` per axis
    (None for a width <= 0): the reference's torch expression evaluated in fp32 on the CPU, so the kernel multiplies by the
    reference's own weights.  blend_width: an int or a tuple of ints.  Cached per (width, device)."""
    widths = (blend_width,) if isinstance(blend_width, int) and not isinstance(blend_width, bool) else tuple(blend_width)
    device = torch.device(device)
    out = []
    for bw in widths:
        if isinstance(bw, bool) or not isinstance(bw, int):
            raise TypeError(f"blend_weights: blend_width must be ints; got {blend_width!r}")
        if bw <= 0:
            out.append(None)
            continue
        w = _BLEND_WEIGHTS.get((bw, str(device)))
        if w is None:
            with torch.inference_mode(False):
                positions = torch.arange(bw, dtype=torch.float32)
                w = (0.5 * (1 - torch.cos(torch.pi * (positions + 0.5) / bw))).to(device)
            _BLEND_WEIGHTS[(bw, str(device))] = w
        out.append(w)
    return tuple(out)


def crop_blend(y, pad, blend_width, out=None, weights=None):
    """y [B, C, *(S + 2 pad)] -> [B, C, *S]: crop_center then cosine_blend_boundaries (periodizer.py:103-199) in one launch
    (ds_crop_blend: the axes in tensor order, an axis with width <= 0 or 2 width >= size skipped, bit-equal to the reference's
    fp32 arithmetic on the same weights).  pad, blend_width: an int or one per spatial axis.  weights: the per-axis tables
    (default: blend_weights(blend_width, y.device)); out: the result buffer (not sharing bytes with y)."""
    who = "crop_blend"
    planes, E = _spatial(y, "y", who)
    nd = len(E)
    p, bw = _per_axis(pad, nd, "pad", who), _per_axis(blend_width, nd, "blend_width", who)
    if min(p) < 0 or min(bw) < 0:
        raise ValueError(f"{who}: negative pad {p} or blend_width {bw}")
    S = tuple(e - 2 * a for e, a in zip(E, p))
    if min(S) < 1:
        raise ValueError(f"{who}: pad {p} leaves nothing of y's spatial axes {E}")
    if weights is None:
        weights = blend_weights(bw, y.device)
    if not isinstance(weights, (tuple, list)) or len(weights) != nd:
        raise ValueError(f"{who}: weights must be one table (or None) per spatial axis")
    for w, b, s in zip(weights, bw, S):
        if w is None:
            if b > 0 and 2 * b < s:
                raise ValueError(f"{who}: no weight table for an axis that is blended (width {b} of {s})")
        elif not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() < b:
            raise ValueError(f"{who}: a weight table must be a 1-D tensor of at least blend_width floats")
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError(f"{who}: out must be a torch.Tensor")
    out = _out(out, tuple(y.shape[:2]) + S, y)
    if _overlap(y, out):
        raise ValueError(f"{who}: y and out share storage")
    if (S[0] * S[1] if nd == 3 else S[0]) >= (1 << 31) - (1 << 20):            # the launch's rows per plane
        raise ValueError(f"{who}: axes beyond 31 bits {S}")
    py, po = _p(y, "y"), _p(out, "out")
    pw = [_p(w, "weights") for w in weights]
    if planes == 0:
        return out
    lead = 3 - nd
    S3, p3, b3, w3 = (1,) * lead + S, (0,) * lead + p, (0,) * lead + bw, [None] * lead + pw
    N.check(N.lib().ds_crop_blend(po, py, planes, S3[0], S3[1], S3[2], p3[0], p3[1], p3[2], b3[0], b3[1], b3[2], w3[0], w3[1],
                                  w3[2], _stream(), 0), "ds_crop_blend")
    return out


def conv_tile_count(H, W):
    """Pixel tiles per channel plane in the fp16x3 kernels' tile_stats layout."""
    return N.lib().ds_conv_tile_count(int(H), int(W))


def table_channels(C):
    """Rows per sample of a prenorm table: channels padded to whole 16-channel chunks."""
    return (C + 15) // 16 * 16


def inorm_table(tile_stats, w, b, kind, count, eps=1e-5, out=None):
    """PUNetG norm table [B, ceil16(C), 4] from a convolution's tile statistics [B, C, ntiles, 4]: rows (M, A, C, 2^-k), k the
    sample's activation exponent for the consuming loader."""
    B, C, nt, _ = tile_stats.shape
    out = _out(out, (B, table_channels(C), 4), tile_stats, _TABLE_MSG)
    _affine(w, b, C, "inorm_table")
    N.check(N.lib().ds_inorm_table(_p(out), _p(tile_stats), _p(w), _p(b), B, C, nt, int(count), float(eps), int(kind),
                                   _stream()), "ds_inorm_table")
    return out


def gnorm1_table(stats_a, w, b, kind, count, stats_b=None, film=None, eps=1e-5, out=None):
    """ADM norm table [B, ceil16(Ca+Cb), 4] from tile statistics of one tensor or of the two halves of a concat (rows as
    inorm_table)."""
    B, Ca, nta, _ = stats_a.shape
    Cb, ntb = (0, 0) if stats_b is None else (stats_b.shape[1], stats_b.shape[2])
    C = Ca + Cb
    out = _out(out, (B, table_channels(C), 4), stats_a, _TABLE_MSG)
    f1, f2, stride = _film_args(film, B, C)
    _affine(w, b, C, "gnorm1_table")
    N.check(N.lib().ds_gnorm1_table(_p(out), _p(stats_a), Ca, nta, _p(stats_b), Cb, ntb, _p(w), _p(b), f1, f2, stride,
                                    B, int(count), float(eps), int(kind), _stream()), "ds_gnorm1_table")
    return out


def gnorm1_stats_tiles(stats_a, kind, count, stats_b=None, eps=1e-5, stats=None):
    """gnorm1_stats [B, 2] from the tile statistics of the tensor's producer(s) instead of a pass over the tensor."""
    require_device(stats_a, "stats_a")
    B, Ca, nta, _ = stats_a.shape
    Cb, ntb = (0, 0) if stats_b is None else (stats_b.shape[1], stats_b.shape[2])
    stats = _out(stats, (B, 2), stats_a, _STATS_MSG)
    N.check(N.lib().ds_gnorm1_stats_tiles(_p(stats), _p(stats_a), Ca, nta, _p(stats_b), Cb, ntb, B, int(count), float(eps),
                                          int(kind), _stream()), "ds_gnorm1_stats_tiles")
    return stats


def conv2d(x, w_packed, Cout, ks, bias=None, shift=None, res1=None, res2=None,
           load_mode=N.DS_LOAD_PLAIN, out=None, kind="fp32", wshift=0, prenorm=None, tile_stats=None, circular=False,
           res1_upsampled=False, w_up=None, up_wshift=0, tap_offset=None, in_amax=None, out_amax=None, amax_split=0,
           pool=None, pc_raw=False):
    """'same' zero-padded conv; x [B, Cin, Hin, Win]; shift [1 or B, Cout] or None.
    fp16x3 kernels only: prenorm [B, ceil16(Cin), 4] (3x3) applies SiLU((x-M)*A+C) in the loader; tile_stats
    [B, Cout, conv_tile_count(H, W), 4] receives per-tile (K, sum(x-K), sum((x-K)^2), n) of the output;
    in_amax: int32 [B] per-sample max |x| (float bits) left by x's producer, NORMALISED for a norm + SiLU output, None = reduce
    x here (one extra read pass and an allocation: captured code passes slots); out_amax: zeroed int32 [B] slots that receive the
    per-sample max |out| for the next raw-input launch; amax_split (fp16x3 1x1 only): out_amax is [2, B] and channels >=
    amax_split report to its second row (the attention in-projection: q, k | v).
    fp16x3 3x3, plain load only (ds_conv2d_h3_pc): pool = PoolOut that may receive MaxPool2d(2) of the result; pc_raw: a launch
    without prenorm may take the persistent kernel.  circular: False, True or (H, W) flags (circular_axes)."""
    pad = pad_word(circular, 2)
    B, Cin, Hin, Win = x.shape
    H, W = _load_sides(load_mode, (Hin, Win))
    if pool is not None:
        pool.written = False                                             # the kernels that have no pooled form leave it so
    if load_mode in (N.DS_LOAD_MAXPOOL2, N.DS_LOAD_AVGPOOL2):
        if (load_mode == N.DS_LOAD_AVGPOOL2) != (kind == "fp16x3" and ks == 1):
            raise ValueError("load modes: AVGPOOL2 is for the fp16x3 1x1 kernel, MAXPOOL2 for the others")
    out = _out(out, (B, Cout, H, W), x)
    expect = {"bf16x6": lambda: N.lib().ds_conv2d_x6_packed_bytes(Cout, Cin) // 4,
              "fp16x3": lambda: (N.lib().ds_conv2d_h3_packed_bytes if ks == 3 else
                                 N.lib().ds_conv1x1_h3_packed_bytes)(Cout, Cin) // 4,
              "fp32": lambda: N.lib().ds_conv2d_packed_floats(Cout, Cin, ks)}[kind]()
    if w_packed.numel() != expect or (kind == "bf16x6" and ks != 3) or ks not in (1, 3):
        raise ValueError("packed weight size does not match (Cout, Cin, ks)")
    stride = _row_stride(shift, B, Cout, _SHIFT_MSG)
    if res1_upsampled:
        if kind != "fp16x3" or ks != 3 or res1 is None or H % 2 or W % 2 or tuple(res1.shape) != (B, Cout, H // 2, W // 2):
            raise ValueError("res1_upsampled: fp16x3 3x3 convolution with res1 of shape [B, Cout, H/2, W/2]")
    _residuals((B, Cout, H, W), None if res1_upsampled else res1, res2)
    _entries(bias, Cout, "bias must have Cout entries")
    if (prenorm is not None or tile_stats is not None) and kind != "fp16x3":
        raise ValueError("prenorm / tile_stats are features of the fp16x3 kernels")
    pin = pout = None
    if kind == "fp16x3":
        pin = _in_amax(x, in_amax, B, raw=prenorm is None)
        if amax_split and (ks != 1 or amax_split % 64):
            raise ValueError("amax_split: the fp16x3 1x1 convolution, a multiple of 64")
        pout = _pi(out_amax, 2 * B if amax_split else B, "out_amax")
    elif out_amax is not None:
        raise ValueError("out_amax is a feature of the fp16x3 kernels (use absmax_rows on the result)")
    if pad and ks == 3 and kind != "fp16x3":
        raise NotImplementedError("periodic padding is implemented in the fp16x3 convolution only")
    if prenorm is not None and (ks != 3 or tuple(prenorm.shape) != (B, table_channels(Cin), 4)):
        raise ValueError(f"prenorm must be [B, ceil16(Cin), 4] on a 3x3 convolution; got {tuple(prenorm.shape)}")
    _tile_stats(tile_stats, B, Cout, H, W, got=True)
    tap = 0
    if tap_offset is not None and tuple(tap_offset) != (0, 0):
        oy, ox = (int(v) for v in tap_offset)
        if kind != "fp16x3" or ks != 3 or not (-8 <= oy <= 7 and -8 <= ox <= 7):
            raise ValueError("tap_offset: fp16x3 3x3 convolution, offsets in [-8, 7]")
        tap = ((oy & 15) << 8) | ((ox & 15) << 12)                      # DS_TAP_OFFSET(oy, ox)
        w_up = None                                                      # the parity kernel has no offset form
    if kind == "fp16x3" and ks == 1:
        N.check(N.lib().ds_conv1x1_h3(_p(out), _p(x), _p(w_packed), int(wshift), _p(bias), _p(shift), stride,
                                      _p(res1), _p(res2), B, Cin, Cout, H, W, load_mode, _p(tile_stats), pin, pout,
                                      int(amax_split), _stream()), "ds_conv1x1_h3")
    elif kind == "fp16x3" and load_mode == N.DS_LOAD_UPSAMPLE2 and w_up is not None \
            and N.lib().ds_conv2d_h3_up_supported(Hin, Win):
        if w_up.numel() != N.lib().ds_conv2d_h3_up_packed_bytes(Cout, Cin) // 4:
            raise ValueError("w_up size does not match (Cout, Cin)")
        N.check(N.lib().ds_conv2d_h3_up(_p(out), _p(x), _p(w_up), int(up_wshift), _p(bias), _p(shift), stride,
                                        _p(res1), _p(res2), B, Cin, Cout, Hin, Win,
                                        pad | (N.DS_RES1_UPSAMPLED if res1_upsampled else 0),
                                        _p(prenorm), _p(tile_stats), pin, pout, _stream()), "ds_conv2d_h3_up")
    elif kind == "fp16x3" and (pool is not None or pc_raw):
        if load_mode != N.DS_LOAD_PLAIN:
            raise ValueError("pool / pc_raw: plain-load convolutions")
        pp = _pool_out(pool, B, Cout, H, W, x)
        did = ctypes.c_int(0)
        N.check(N.lib().ds_conv2d_h3_pc(_p(out), _p(x), _p(w_packed), int(wshift), _p(bias), _p(shift), stride,
                                        _p(res1), _p(res2), B, Cin, Cout, H, W,
                                        tap | pad | (N.DS_RES1_UPSAMPLED if res1_upsampled else 0),
                                        _p(prenorm), _p(tile_stats), pin, pout, _stream(), _p(pp), ctypes.byref(did),
                                        N.DS_PC_RAW if pc_raw else 0), "ds_conv2d_h3_pc")
        if pool is not None:
            pool.written = bool(did.value)
    elif kind == "fp16x3":
        N.check(N.lib().ds_conv2d_h3(_p(out), _p(x), _p(w_packed), int(wshift), _p(bias), _p(shift), stride,
                                     _p(res1), _p(res2), B, Cin, Cout, H, W,
                                     load_mode | tap | pad | (N.DS_RES1_UPSAMPLED if res1_upsampled else 0),
                                     _p(prenorm), _p(tile_stats), pin, pout,
                                     _stream()), "ds_conv2d_h3")
    elif kind == "bf16x6":
        N.check(N.lib().ds_conv2d_x6(_p(out), _p(x), _p(w_packed), _p(bias), _p(shift), stride, _p(res1),
                                     _p(res2), B, Cin, Cout, H, W, load_mode, _stream()), "ds_conv2d_x6")
    else:
        N.check(N.lib().ds_conv2d(_p(out), _p(x), _p(w_packed), _p(bias), _p(shift), stride, _p(res1), _p(res2),
                                  B, Cin, Cout, H, W, ks, load_mode, _stream()), "ds_conv2d")
    return out


def conv_images_floats(B, C, H, W):
    """Floats of the pre-split image buffer of a [B, C, H, W] activation (ds_inorm_silu_images / conv_img)."""
    return N.lib().ds_conv_images_bytes(int(B), int(C), int(H), int(W)) // 4


def inorm_silu_images_supported(H, W):
    return bool(N.lib().ds_inorm_silu_images_supported(int(H), int(W)))


def inorm_silu_images(x, w, b, kind, eps=1e-5, out=None):
    """inorm_silu with the result written as the consuming convolution's pre-split fp16 hi / lo images (conv_img)."""
    require_device(x, "x")
    B, C, H, W = x.shape
    out = _images(out, B, C, H, W, "images buffer size does not match x", like=x)
    if w is not None and (w.numel() != C or b.numel() != C):
        raise ValueError("norm affine parameters must have C entries")
    N.check(N.lib().ds_inorm_silu_images(_p(out), _p(x), _p(w), _p(b), B, C, H, W, float(eps), int(kind), _stream()),
            "ds_inorm_silu_images")
    return out


def conv_img(images, pw, B, Cin, H, W, bias=None, shift=None, res1=None, res2=None, tile_stats=None, out=None,
             res1_upsampled=False, out_amax=None, pool=None):
    """3x3 'same' zero-padded fp16x3 convolution whose input is given as pre-split fp16 hi / lo images (the layout
    ds_inorm_silu_images writes): patches are staged by LDS-DMA, no split in the kernel.  pw = pack_conv(weight, "fp16x3")."""
    require_device(images, "images")
    if pw.kind != "fp16x3" or pw.ks != 3 or pw.subs is not None:
        raise ValueError("conv_img: a 3x3 fp16x3 packing")
    Cout = pw.Cout
    _images(images, B, Cin, H, W, "images size does not match (B, Cin, H, W)")
    out = _out(out, (B, Cout, H, W), images)
    stride = _row_stride(shift, B, Cout, _SHIFT_MSG)
    if res1_upsampled and (res1 is None or H % 2 or W % 2 or tuple(res1.shape) != (B, Cout, H // 2, W // 2)):
        raise ValueError("res1_upsampled: res1 of shape [B, Cout, H/2, W/2]")
    _residuals((B, Cout, H, W), None if res1_upsampled else res1, res2)
    _tile_stats(tile_stats, B, Cout, H, W)
    _entries(bias, Cout, "bias must have Cout entries")
    if pool is not None:                                                  # pool: as conv2d's
        pp = _pool_out(pool, B, Cout, H, W, images)
        did = ctypes.c_int(0)
        N.check(N.lib().ds_conv2d_h3_pc(_p(out), _p(images), _p(pw.data), int(pw.wshift), _p(bias), _p(shift), stride, _p(res1),
                                        _p(res2), B, Cin, Cout, H, W, N.DS_RES1_UPSAMPLED if res1_upsampled else 0, None,
                                        _p(tile_stats), None, _pi(out_amax, B, "out_amax"), _stream(), _p(pp), ctypes.byref(did),
                                        N.DS_PC_IMAGES), "ds_conv2d_h3_pc")
        pool.written = bool(did.value)
        return out
    N.check(N.lib().ds_conv2d_h3_img(_p(out), _p(images), _p(pw.data), int(pw.wshift), _p(bias), _p(shift), stride, _p(res1),
                                     _p(res2), B, Cin, Cout, H, W, N.DS_RES1_UPSAMPLED if res1_upsampled else 0,
                                     _p(tile_stats), _pi(out_amax, B, "out_amax"), _stream()), "ds_conv2d_h3_img")
    return out


def table_apply_images(x, table, out=None):
    """SiLU((x - M) * A + C) from a norm table [B, ceil16(C), 4] (inorm_table / gnorm1_table: the fused loader's arithmetic),
    written as the convolution's pre-split images (conv_img / conv_up_img).  Any plane size."""
    require_device(x, "x")
    require_device(table, "table")
    B, C, H, W = x.shape
    if tuple(table.shape) != (B, table_channels(C), 4):
        raise ValueError(f"table must be {(B, table_channels(C), 4)}; got {tuple(table.shape)}")
    out = _images(out, B, C, H, W, "images buffer size does not match x", like=x)
    N.check(N.lib().ds_table_apply_images(_p(out), _p(x), _p(table), B, C, H, W, _stream()), "ds_table_apply_images")
    return out


def conv_up_img_supported(pw, Hl, Wl):
    """conv_up_img takes this packing and low-resolution size."""
    return (pw.kind == "fp16x3" and pw.ks == 3 and pw.subs is None and pw.up is not None
            and bool(N.lib().ds_conv2d_h3_up_supported(int(Hl), int(Wl))))


def conv_up_img(images, pw, B, Cin, Hl, Wl, bias=None, shift=None, res1=None, res2=None, tile_stats=None, out=None,
                out_amax=None):
    """conv3x3(nearest_x2(a)) as the four collapsed parity kernels (ds_conv2d_h3_up) with the low-resolution activation a given as
    pre-split images; output [B, Cout, 2 Hl, 2 Wl].  pw = pack_conv(weight, "fp16x3", upsampled=True)."""
    require_device(images, "images")
    if not conv_up_img_supported(pw, Hl, Wl):
        raise ValueError("conv_up_img: a 3x3 fp16x3 packing with parity kernels and an input of whole 8x32 / 16x16 tiles")
    Cout, H, W = pw.Cout, 2 * Hl, 2 * Wl
    _images(images, B, Cin, Hl, Wl, "images size does not match (B, Cin, Hl, Wl)")
    out = _out(out, (B, Cout, H, W), images)
    stride = _row_stride(shift, B, Cout, _SHIFT_MSG)
    _residuals((B, Cout, H, W), res1, res2)
    _tile_stats(tile_stats, B, Cout, H, W)
    _entries(bias, Cout, "bias must have Cout entries")
    N.check(N.lib().ds_conv2d_h3_up_img(_p(out), _p(images), _p(pw.up), int(pw.up_wshift), _p(bias), _p(shift), stride, _p(res1),
                                        _p(res2), B, Cin, Cout, Hl, Wl, _p(tile_stats), _pi(out_amax, B, "out_amax"), _stream()),
            "ds_conv2d_h3_up_img")
    return out


def gnorm1_apply_images(x, stats, w, b, kind, pool=False, film=None, out=None):
    """gnorm1_apply (kinds 0 / 1) with the result written as the consuming convolution's pre-split images (conv_img)."""
    require_device(x, "x")
    B, C, H, W = x.shape
    if pool and (H % 2 or W % 2):
        raise ValueError("pooling needs even H, W")
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = _images(out, B, C, Ho, Wo, "images buffer size does not match x", like=x)
    f1, f2, stride = _film_args(film, B, C)
    _gnorm1_inputs(stats, w, b, B, C, "gnorm1_apply_images")
    N.check(N.lib().ds_gnorm1_apply_images(_p(out), _p(x), _p(stats), _p(w), _p(b), f1, f2, stride, B, C, Ho, Wo, int(kind),
                                           1 if pool else 0, _stream()), "ds_gnorm1_apply_images")
    return out


def token_l2_normalize(x, c0, C, eps=1e-8, gain=1.0):
    """In place: channels [c0, c0+C) of x [B, Ctot, L] divided by (per-token L2 norm + eps), times gain."""
    require_device(x, "x")
    B, Ctot, L = x.shape
    N.check(N.lib().ds_token_l2_normalize(_p(x), B, Ctot, int(c0), int(C), L, float(eps), float(gain), _stream()),
            "ds_token_l2_normalize")
    return x


# Pre-split K / V images + LDS-DMA staging (ds_attention_h3_ws) against staging in every workgroup (ds_attention_h3),
# measured on MI355X (tools/attn_time.py): E = 256: 332 vs 353 us at L = 1024 (B = 64), 975 vs 1181 us at L = 4096
# (B = 16); E = 128 / 64 at L = 1024: 162 vs 160 / 91 vs 85 us.  A tile is re-split L/128 times without the images.
ATTN_IMAGES_MIN_L = 2048     # any head width
ATTN_IMAGES_MIN_L_WIDE = 1024    # E = 256


def _attention_uses_images(E, L, precision):
    if precision != "fp16x3" or E not in (32, 64, 128, 256) or L % 32:
        return False
    return L >= ATTN_IMAGES_MIN_L or (E == 256 and L >= ATTN_IMAGES_MIN_L_WIDE)


def _check_heads(E, heads):
    heads = int(heads)
    if heads < 1 or E % heads:
        raise ValueError(f"attention: E={E} is not a multiple of heads={heads}")
    return heads


def attention_workspace_floats(B, E, L, precision="fp16x3", heads=1):
    """Floats of scratch attention() can use (0: none) -- for callers that keep buffers in a pool."""
    heads = _check_heads(E, heads)
    if heads > 1:       # the image form by the head width: a head's K / V tiles are re-split once per 128 of its queries
        if _attention_uses_images(E // heads, L, precision):
            return N.lib().ds_attention_h3_heads_workspace_bytes(B, E, heads, L) // 4
        return 0
    if _attention_uses_images(E, L, precision):
        return N.lib().ds_attention_h3_workspace_bytes(B, E, L) // 4
    return 0


def attention(qkv, E, out=None, precision="fp32", workspace=None, in_amax=None, out_amax=None, heads=1):
    """qkv [B, 3E, L] channel-major -> out [B, E, L].  precision "fp16x3": split-fp16 MFMA
    (fp32-level accuracy, E <= 256); anything else, or wider heads: exact-fp32 MFMA.
    workspace: float tensor of attention_workspace_floats(...) elements; allocated here when needed and not given.
    in_amax: int32 [2, B] -- per-sample max |q, k| and max |v| (conv2d(..., amax_split=2E) leaves them), None = reduced here;
    out_amax [B]: as conv2d.  The fp16x3 kernels stage q, k and v times the sample's powers of two; the exact-fp32 kernels need
    none, and an out_amax request is served by a reduction over their result.
    heads: nn.MultiheadAttention(E, heads) -- E % heads == 0; head h attends over rows [h d, (h+1) d) of each third of qkv,
    d = E / heads, with logits scaled by 1/sqrt(d).  fp16x3 at d in {32, 64, 128, 256} and L % 32 == 0: the split-fp16 kernel
    with a head axis; any other d or L, or precision "fp32": the exact-fp32 per-head kernel.  heads=1 is the single-head call."""
    B, E3, L = qkv.shape
    if E3 != 3 * E:
        raise ValueError("qkv must be [B, 3E, L]")
    heads = _check_heads(E, heads)
    out = _out(out, (B, E, L), qkv)
    lib, d = N.lib(), E // heads
    if not (precision == "fp16x3" and L % 32 == 0 and d in (32, 64, 128, 256)):
        if heads > 1:
            N.check(lib.ds_attention_heads_generic(_p(out), _p(qkv), B, E, heads, L, _stream()), "ds_attention_heads_generic")
        elif L % 32 != 0 or E not in (32, 64, 128, 256, 384, 512):
            N.check(lib.ds_attention_generic(_p(out), _p(qkv), B, E, L, _stream()), "ds_attention_generic")
        else:
            N.check(lib.ds_attention(_p(out), _p(qkv), B, E, L, _stream()), "ds_attention")
        if out_amax is not None:
            absmax_rows(out, B, out=out_amax)
        return out
    if in_amax is None:          # one exponent pair per sample serves all its heads
        in_amax = amax_new(2 * B, qkv.device)
        absmax_rows(qkv[:, :2 * E], out=in_amax[:B])
        absmax_rows(qkv[:, 2 * E:], out=in_amax[B:])
    pin, pout = (None if in_amax is NORMALISED else _pi(in_amax, 2 * B, "in_amax")), _pi(out_amax, B, "out_amax")
    need = attention_workspace_floats(B, E, L, precision, heads)      # the image form by the head width (0: staged per workgroup)
    pws = _p(_workspace(workspace, 4 * need, qkv, "attention workspace too small"), "workspace") if need else None
    if heads > 1:
        N.check(lib.ds_attention_h3_heads(_p(out), _p(qkv), pws, B, E, heads, L, pin, pout, _stream()), "ds_attention_h3_heads")
    elif need:
        N.check(lib.ds_attention_h3_ws(_p(out), _p(qkv), pws, B, E, L, pin, pout, _stream()), "ds_attention_h3_ws")
    else:
        N.check(lib.ds_attention_h3(_p(out), _p(qkv), B, E, L, pin, pout, _stream()), "ds_attention_h3")
    return out


def attention_xkv(q, x, E, out=None, workspace=None, q_amax=None, x_amax=None, out_amax=None):
    """Single-head fp16x3 attention in the image form with x as keys AND values (the folded block):
    q [B, E, L], x [B, E, L] channel-major -> out [B, E, L].  Only where the image form runs (_attention_uses_images(E, L,
    "fp16x3")): anything else is refused, not rerouted.  workspace: attention_workspace_floats(B, E, L) floats, allocated here
    when not given.  q_amax, x_amax: int32 [B] each, the exponent rows of q and of x (x's serves the keys and the values);
    None = reduced here, NORMALISED = no scaling.  out_amax [B]: as attention()."""
    B, Eq, L = q.shape
    if Eq != E or tuple(x.shape) != (B, E, L):
        raise ValueError(f"attention_xkv: q and x must be [B, E={E}, L]; got {tuple(q.shape)} and {tuple(x.shape)}")
    if not _attention_uses_images(E, L, "fp16x3"):
        raise ValueError(f"attention_xkv: E={E}, L={L} is outside the image form (E in 32, 64, 128, 256; L % 32 == 0; "
                         f"L >= {ATTN_IMAGES_MIN_L}, or {ATTN_IMAGES_MIN_L_WIDE} at E = 256)")
    out = _out(out, (B, E, L), q)
    pq, px = _p(q, "q"), _p(x, "x")
    if B == 0:
        return out
    if (pq | px) & 15:
        raise ValueError("attention_xkv: q and x must be 16-byte aligned")
    if q_amax is None:
        q_amax = absmax_rows(q, B)
    if x_amax is None:
        x_amax = absmax_rows(x, B)
    paq = None if q_amax is NORMALISED else _pi(q_amax, B, "q_amax")
    pax = None if x_amax is NORMALISED else _pi(x_amax, B, "x_amax")
    need = N.lib().ds_attention_h3_workspace_bytes(B, E, L)
    pws = _p(_workspace(workspace, need, q, "attention workspace too small"), "workspace")
    N.check(N.lib().ds_attention_h3_xkv(_p(out), pq, px, pws, B, E, L, paq, pax, pax, _pi(out_amax, B, "out_amax"), _stream(), 0),
            "ds_attention_h3_xkv")
    return out


def linear(x, w, b=None, act=0, out=None):
    M, K = x.shape
    Nn, K2 = w.shape
    if K != K2:
        raise ValueError("linear: inner dimensions differ")
    _entries(b, Nn, "linear: b must have N={} entries", Nn)
    out = _out(out, (M, Nn), x)
    N.check(N.lib().ds_linear(_p(out), _p(x), _p(w), _p(b), M, K, Nn, act, _stream()), "ds_linear")
    return out


def fourier_features(t, W, add=None, out=None):
    M, half = t.numel(), W.numel()
    add_rows = 0
    if add is not None:
        if add.dim() < 1 or add.shape[-1] != 2 * half:
            raise ValueError(f"fourier_features: add must hold rows of {2 * half} entries; got {tuple(add.shape)}")
        add = add.reshape(-1, 2 * half)
        add_rows = add.shape[0]
    out = _out(out, (M, 2 * half), t)
    N.check(N.lib().ds_fourier_features(_p(out), _p(t), _p(W), _p(add), add_rows, M, half, _stream()),
            "ds_fourier_features")
    return out


# ---------------------------------------------------------------- token-wise layers of the DiffusionTransformer (ds_tokens.hip)
def _mod_rows(table, E, B, row, what):
    """A modulation table [rows, n*E] (chunks of E along its rows) for B samples -> (first float of sample 0's row, stride in
    floats between samples).  row=None: the table has 1 (shared) or B rows; row=r: row r serves the whole batch."""
    require_device(table, what)
    if table.dim() != 2 or table.shape[1] % E or not table.is_contiguous():
        raise ValueError(f"{what} must be a contiguous [rows, n*{E}] table; got {tuple(table.shape)}")
    width = table.shape[1]
    if row is not None:
        row = int(row)
        if not 0 <= row < table.shape[0]:
            raise ValueError(f"{what}: row {row} outside the table's {table.shape[0]} rows")
        return row * width, 0
    if table.shape[0] not in (1, B):
        raise ValueError(f"{what} must have 1 or {B} rows; got {table.shape[0]}")
    return 0, (0 if table.shape[0] == 1 else width)


def token_layernorm(x, w, b, mod=None, shift_chunk=0, scale_chunk=1, row=None, eps=1e-5, out=None, out_amax=None):
    """LayerNorm(E) of every token of x [B, E, L] (channel-major), then adaLN modulation
    out = LN(x) * (1 + scale) + shift, with shift / scale the chunks `shift_chunk` / `scale_chunk` (of E floats) of the rows of
    `mod` [rows, n*E]: 1 or B rows, or the single row `row` for the whole batch (the captured sampler's table).  mod=None: the
    plain LayerNorm.  out_amax: int32 [B] slots (zeroed) that receive the per-sample max |out| for an fp16x3 consumer."""
    require_device(x, "x")
    if x.dim() != 3:
        raise ValueError("token_layernorm: x must be [B, E, L]")
    B, E, L = x.shape
    _entries(w, E, "token_layernorm: weight must have E={} entries", E)
    _entries(b, E, "token_layernorm: bias must have E={} entries", E)
    if out is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("token_layernorm: out must be a [B, E, L] tensor other than x")
    out = _out(out, (B, E, L), x, "token_layernorm: out must be a [B, E, L] tensor other than x")
    psc = psh = None
    stride = 0
    if mod is not None:
        first, stride = _mod_rows(mod, E, B, row, "mod")
        n = mod.shape[1] // E
        if not (0 <= shift_chunk < n and 0 <= scale_chunk < n):
            raise ValueError("token_layernorm: chunk outside the table")
        psh = mod.data_ptr() + 4 * (first + shift_chunk * E)
        psc = mod.data_ptr() + 4 * (first + scale_chunk * E)
    N.check(N.lib().ds_token_layernorm(_p(out, "out"), _p(x, "x"), _p(w, "weight"), _p(b, "bias"), psc, psh, stride, B, E, L, float(eps),
                                       _pi(out_amax, B, "out_amax"), _stream()), "ds_token_layernorm")
    return out


def token_gate(x, y, mod, chunk=0, row=None, out=None):
    """x + gate * y on [B, E, L] with gate the chunk `chunk` of the rows of mod (as token_layernorm); out may be x (in place)."""
    require_device(x, "x")
    if x.dim() != 3 or tuple(y.shape) != tuple(x.shape):
        raise ValueError("token_gate: x and y must be [B, E, L]")
    B, E, L = x.shape
    first, stride = _mod_rows(mod, E, B, row, "mod")
    if not 0 <= chunk < mod.shape[1] // E:
        raise ValueError("token_gate: chunk outside the table")
    if out is not None and out.data_ptr() == y.data_ptr():
        raise ValueError("token_gate: out must be [B, E, L] and may alias x only")
    out = _out(out, (B, E, L), x, "token_gate: out must be [B, E, L] and may alias x only")
    N.check(N.lib().ds_token_gate(_p(out, "out"), _p(x, "x"), _p(y, "y"), mod.data_ptr() + 4 * (first + chunk * E), stride, B, E, L,
                                  _stream()), "ds_token_gate")
    return out


def silu_amax(x, out=None, out_amax=None):
    """SiLU(x) for x [B, ...] (out may be x), the per-sample max |out| merged into out_amax (int32 [B]) when given."""
    require_device(x, "x")
    B = x.shape[0]
    out = _out(out, x.shape, x, "silu_amax: out must have x's shape")
    N.check(N.lib().ds_silu_amax(_p(out, "out"), _p(x, "x"), B, x.numel() // max(B, 1), _pi(out_amax, B, "out_amax"), _stream()),
            "ds_silu_amax")
    return out


def _patch_dims(shape, patch, what):
    if len(shape) != 4:
        raise ValueError(f"{what}: the image must be [B, C, H, W]")
    B, C, H, W = shape
    patch = int(patch)
    if patch < 1 or H % patch or W % patch:
        raise ValueError(f"{what}: a {H}x{W} image does not divide into {patch}x{patch} patches")
    return B, C, H, W, patch, (H // patch) * (W // patch)


def patch_embed(x, w, bias, patch, out=None):
    """x [B, C, H, W] -> tokens [B, E, L]: Linear(C*patch^2, E) of the patches flattened in (c p1 p2) order, token h*(W/patch) + w."""
    require_device(x, "x")
    B, C, H, W, patch, L = _patch_dims(x.shape, patch, "patch_embed")
    E = w.shape[0]
    if tuple(w.shape) != (E, C * patch * patch) or (bias is not None and bias.numel() != E):
        raise ValueError(f"patch_embed: weight must be [E, {C * patch * patch}] and bias [E]; got {tuple(w.shape)}")
    out = _out(out, (B, E, L), x, "patch_embed: out must be {1}")
    N.check(N.lib().ds_patch_embed(_p(out, "out"), _p(x, "x"), _p(w, "weight"), _p(bias, "bias"), B, C, H, W, patch, E, _stream()),
            "ds_patch_embed")
    return out


def patch_unembed(x, w, bias, patch, shape, out=None):
    """tokens x [B, E, L] -> image `shape` = (B, C, H, W): Linear(E, C*patch^2), then the inverse patch map."""
    require_device(x, "x")
    B, C, H, W, patch, L = _patch_dims(tuple(shape), patch, "patch_unembed")
    if x.dim() != 3 or x.shape[0] != B or x.shape[2] != L:
        raise ValueError(f"patch_unembed: x must be [{B}, E, {L}]; got {tuple(x.shape)}")
    E = x.shape[1]
    K = C * patch * patch
    if tuple(w.shape) != (K, E) or (bias is not None and bias.numel() != K):
        raise ValueError(f"patch_unembed: weight must be [{K}, {E}] and bias [{K}]; got {tuple(w.shape)}")
    out = _out(out, (B, C, H, W), x, "patch_unembed: out must be {1}")
    N.check(N.lib().ds_patch_unembed(_p(out, "out"), _p(x, "x"), _p(w, "weight"), _p(bias, "bias"), B, C, H, W, patch, E, _stream()),
            "ds_patch_unembed")
    return out


# ---------------------------------------------------------------- streaming layers of ConVit (ds_convit.hip)
RMS_EPS = float(torch.finfo(torch.float32).eps)      # ChannelRMSNorm's eps (convit.py:237)
RMS_FUSED_POOLS = (1, 2, 4)                           # pooling factors ds_channel_rmsnorm applies itself
# Each wrapper below builds its argument tuple first and touches the library last, so every pointer and extent is checked
# before N.lib() is called at all.


def channel_rmsnorm(x, w, mod=None, row=None, pool=1, out=None, out_amax=None, eps=RMS_EPS, scratch=None):
    """ChannelRMSNorm of x [B, E, H, W] plus an embedding row: out = x / sqrt(mean_c(x^2) + eps) * w [+ mod row], with mod
    [rows, E]: 1 or B rows, or the single row `row` for the whole batch (the captured sampler's table).  pool=f writes
    AvgPool2d(f) of that result, [B, E, H // f, W // f]; f in RMS_FUSED_POOLS is pooled inside the kernel, any other factor is the
    unpooled result (in `scratch` [B, E, H, W] when given: captured code must not allocate) followed by avgpool_f.
    out_amax: int32 [B] slots (zeroed) that receive the per-sample max |out| for an fp16x3 consumer.  out may not alias x."""
    require_device(x, "x")
    if x.dim() != 4:
        raise ValueError(f"channel_rmsnorm: x must be [B, E, H, W]; got {tuple(x.shape)}")
    B, E, H, W = x.shape
    _entries(w, E, "channel_rmsnorm: weight must have E={} entries", E)
    f = _factor(pool)
    if f > min(H, W):
        raise ValueError(f"channel_rmsnorm: pool={f} exceeds the field {H}x{W}")
    if _overlap(out, x):
        raise ValueError("channel_rmsnorm: out must be a tensor other than x")
    out = _out(out, (B, E, H // f, W // f), x, "channel_rmsnorm: out has shape {}, expected {}")
    pmod, stride = None, 0
    if mod is not None:
        first, stride = _mod_rows(mod, E, B, row, "mod")
        if mod.shape[1] != E:
            raise ValueError(f"channel_rmsnorm: mod must be [rows, {E}]; got {tuple(mod.shape)}")
        pmod = mod.data_ptr() + 4 * first
    fused = f in RMS_FUSED_POOLS
    dst = out
    if not fused:
        if _overlap(scratch, x) or _overlap(scratch, out):
            raise ValueError("channel_rmsnorm: scratch must be a tensor other than x and out")
        dst = _out(scratch, (B, E, H, W), x, "channel_rmsnorm: scratch has shape {}, expected {}")
    args = (_p(dst, "out" if fused else "scratch"), _p(x, "x"), _p(w, "weight"), pmod, stride, B, E, H, W, f if fused else 1, float(eps),
            _pi(out_amax, B, "out_amax") if fused else None, _stream(), 0)
    N.check(N.lib().ds_channel_rmsnorm(*args), "ds_channel_rmsnorm")
    if not fused:
        avgpool_f(dst, f, out=out)
        if out_amax is not None:
            absmax_rows(out, B, out=out_amax)
    return out


def rope2d(qkv, E, heads, cos_sin, out_amax=None):
    """LearnedRoPE in place on the q and k thirds of qkv [B, 3E, L]: with d = E / heads, rows (h*d + 2i, h*d + 2i + 1) become
    (a cos - b sin, a sin + b cos) with cos, sin = cos_sin[l, i] (cos_sin [L, d/2, 2]); the v third is left untouched.
    out_amax: int32 [2, B] slots (zeroed) that receive max |q, k| after the rotation and max |v|: attention(in_amax=)."""
    require_device(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[1] != 3 * E:
        raise ValueError(f"rope2d: qkv must be [B, 3E, L] with E={E}; got {tuple(qkv.shape)}")
    B, _, L = qkv.shape
    heads = _check_heads(E, heads)
    d = E // heads
    if d % 2:
        raise ValueError(f"rope2d: the head width E / heads = {d} must be even")
    require_device(cos_sin, "cos_sin")
    if tuple(cos_sin.shape) != (L, d // 2, 2):
        raise ValueError(f"rope2d: cos_sin must be {(L, d // 2, 2)}; got {tuple(cos_sin.shape)}")
    args = (_p(qkv, "qkv"), _p(cos_sin, "cos_sin"), B, E, heads, L, _pi(out_amax, 2 * B, "out_amax"), _stream(), 0)
    N.check(N.lib().ds_rope2d(*args), "ds_rope2d")
    return qkv


def upsample_bilinear(x, factor, out=None):
    """F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=False) of a field [B, C, H, W], any integer
    factor >= 1."""
    f = _factor(factor)
    require_device(x, "x")
    if x.dim() != 4:
        raise ValueError(f"upsample_bilinear: x must be [B, C, H, W]; got {tuple(x.shape)}")
    B, C, H, W = x.shape
    if _overlap(out, x):
        raise ValueError("upsample_bilinear: out must be a tensor other than x")
    out = _out(out, (B, C, f * H, f * W), x, "upsample_bilinear: out has shape {}, expected {}")
    args = (_p(out, "out"), _p(x, "x"), B * C, H, W, f, _stream(), 0)
    N.check(N.lib().ds_upsample_bilinear(*args), "ds_upsample_bilinear")
    return out


DEPTHWISE_MAX_KERNEL = 7


def depthwise_conv_silu(x, w, b, out=None, out_amax=None):
    """SiLU(depthwise k x k 'same' zero-padded convolution + bias) of x [B, E, H, W]: w [E, 1, k, k] (k odd, at most
    DEPTHWISE_MAX_KERNEL), b [E] or None.  out_amax: as channel_rmsnorm.  out may not alias x."""
    require_device(x, "x")
    if x.dim() != 4:
        raise ValueError(f"depthwise_conv_silu: x must be [B, E, H, W]; got {tuple(x.shape)}")
    B, E, H, W = x.shape
    if w.dim() != 4 or w.shape[0] != E or w.shape[1] != 1 or w.shape[2] != w.shape[3]:
        raise ValueError(f"depthwise_conv_silu: weight must be [{E}, 1, k, k]; got {tuple(w.shape)}")
    k = w.shape[2]
    if k % 2 == 0 or k > DEPTHWISE_MAX_KERNEL:
        raise NotImplementedError(f"depthwise_conv_silu: kernel size {k}: odd sizes up to {DEPTHWISE_MAX_KERNEL} are implemented")
    _entries(b, E, "depthwise_conv_silu: bias must have E={} entries", E)
    if _overlap(out, x):
        raise ValueError("depthwise_conv_silu: out must be a tensor other than x")
    out = _out(out, (B, E, H, W), x, "depthwise_conv_silu: out has shape {}, expected {}")
    args = (_p(out, "out"), _p(x, "x"), _p(w, "weight"), _p(b, "bias"), B, E, H, W, k,
            _pi(out_amax, B, "out_amax"), _stream(), 0)
    N.check(N.lib().ds_depthwise_conv_silu(*args), "ds_depthwise_conv_silu")
    return out


def swiglu(ag, out=None, out_amax=None):
    """ag [B, 2C, ...] -> SiLU(ag[:, :C]) * ag[:, C:], [B, C, ...].  out_amax: as channel_rmsnorm.  out may not overlap ag."""
    require_device(ag, "ag")
    if ag.dim() < 2 or ag.shape[1] % 2:
        raise ValueError(f"swiglu: ag must be [B, 2C, ...]; got {tuple(ag.shape)}")
    B, C = ag.shape[0], ag.shape[1] // 2
    if _overlap(out, ag):
        raise ValueError("swiglu: out must not overlap ag")
    out = _out(out, (B, C) + tuple(ag.shape[2:]), ag, "swiglu: out has shape {}, expected {}")
    args = (_p(out, "out"), _p(ag, "ag"), B, out.numel() // max(B, 1), _pi(out_amax, B, "out_amax"), _stream(), 0)
    N.check(N.lib().ds_swiglu(*args), "ds_swiglu")
    return out


def convit_blend(u, xc, x0, s, out=None):
    """((1 - s) * u + s * xc) + x0, with s a one-element device tensor (read by the kernel: no host read, so the call can be
    captured).  out may be x0 (in place), not u or xc."""
    require_device(u, "u")
    if tuple(xc.shape) != tuple(u.shape) or tuple(x0.shape) != tuple(u.shape):
        raise ValueError(f"convit_blend: u, xc and x0 must have one shape; got {tuple(u.shape)}, {tuple(xc.shape)}, {tuple(x0.shape)}")
    require_device(s, "s")
    if s.numel() != 1:
        raise ValueError(f"convit_blend: s must hold one element; got {tuple(s.shape)}")
    if _overlap(out, u) or _overlap(out, xc) or (_overlap(out, x0) and out.data_ptr() != x0.data_ptr()):
        raise ValueError("convit_blend: out may alias x0 only")
    out = _out(out, tuple(u.shape), u, "convit_blend: out has shape {}, expected {}")
    args = (_p(out, "out"), _p(u, "u"), _p(xc, "xc"), _p(x0, "x0"), _p(s, "s"), u.numel(), _stream(), 0)
    N.check(N.lib().ds_convit_blend(*args), "ds_convit_blend")
    return out


def fourier_channels(x, W, out=None):
    """ConvolutionalFourierProjection: x [B, C, *spatial], W [C, D] -> [B, 2D, *spatial] = cat[sin, cos](x . 2*pi*W)."""
    require_device(x, "x")
    B, C = x.shape[0], x.shape[1]
    if W.dim() != 2 or W.shape[0] != C:
        raise ValueError(f"fourier_channels: W must be [{C}, D]; got {tuple(W.shape)}")
    D = W.shape[1]
    HW = x.numel() // max(B * C, 1)
    out = _out(out, (B, 2 * D) + tuple(x.shape[2:]), x)
    N.check(N.lib().ds_fourier_channels(_p(out, "out"), _p(x, "x"), _p(W, "W"), B, C, D, HW, _stream()), "ds_fourier_channels")
    return out


class Graph:
    """A captured launch sequence (hipGraph) on torch's current stream."""

    def __init__(self):
        self._h = ctypes.c_void_p()
        self.nodes = 0

    @staticmethod
    def _allocations():
        return torch.cuda.memory_stats().get("allocation.all.allocated", 0)

    def __enter__(self):
        self._stream = _stream()
        # No finaliser may run inside the captured region: a module that has captured plans is cyclic garbage once dropped
        # (module -> plans -> loop -> source -> module), and the collector frees its graphs and tensors -- HIP calls on the
        # capturing thread -- whenever its counters say so.  Collect now, and keep the collector off until the capture ends
        # (torch.cuda.graph collects before it captures for the same reason).
        self._gc = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            self._alloc0 = self._allocations()
            N.check(N.lib().ds_graph_begin_capture(self._stream), "ds_graph_begin_capture")
        except BaseException:
            if self._gc:
                gc.enable()
            raise
        return self

    def __exit__(self, et, ev, tb):
        n = ctypes.c_int(0)
        rc = N.lib().ds_graph_end_capture(self._stream, ctypes.byref(self._h), ctypes.byref(n))
        if self._gc:
            gc.enable()
        if et is None:
            N.check(rc, "ds_graph_end_capture")
            # The graph bakes device addresses.  A tensor allocated inside the captured region belongs to torch's
            # caching allocator, which hands its block to someone else once the Python object dies -- while every
            # replay keeps writing there.  Captured code must take its buffers from a pre-filled workspace.
            made = self._allocations() - self._alloc0
            if made:
                raise RuntimeError(f"{made} device allocation(s) happened inside a captured region; the graph would "
                                   "write to memory it does not own on replay")
        self.nodes = n.value
        return False

    def launch(self):
        N.check(N.lib().ds_graph_launch(self._h, _stream()), "ds_graph_launch")

    def __del__(self):
        try:
            if self._h:
                N.lib().ds_graph_destroy(self._h)
        except Exception:
            pass
