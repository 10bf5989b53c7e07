"""The error model of the normalisation kernels, and the data families that stress it (plain numpy / torch, no GPU).

Every reference is fp64 computed FROM THE fp32 INPUT VALUES, so input quantisation is not an error.  u = 2^-24.

Statistics bound -- kernels that expose (mean, rstd) or table rows (M, A):
    |mean - mean64| <= dm = k_m u mean64(|x|)
    |rstd / rstd64 - 1| <= rho = 4e-7 + dm^2 / (2 (var64 + eps)) + c64
  4e-7: (float)var, + eps, sqrtf and the reciprocal are one rounding each when correctly rounded (u each, the first two count
  half through the square root: 3u), plus two ulp (2 * 2u) of slack for the device's sqrtf and division: 7u = 4.2e-7.
  dm^2 / (2 (var + eps)): a second moment centred on a mean that is off by dm is too large by dm^2.
  c64 = 2^-51 mean64(x^2) / (var64 + eps) for kernels that form q/n - mean^2 in fp64 (the roundings of q/n and mean^2, one
  fp64 ulp of mean(x^2) each, survive the subtraction at full size), 0 for the others.
  k_m = 2 for kernels that accumulate in fp64 and round once (ds_gnorm.hip, ds_groupnorm.hip, ds_normtab.hip, k_slice_tables);
  k_m = ceil(log2 n) + 2 for the fp32 two-pass tree reductions of ds_norm.hip -- the a-priori bound of pairwise summation,
  which any correct fp32 tree meets and a sequential or one-pass sum does not.

Element bound -- fused kernels that return only SiLU(norm(x)); arg64 = (x - mean64) rstd64 w + b, want = SiLU(arg64):
    |got - want| <= 1.1 |w| rstd64 (dm + rho |x - mean64|) + 4u (|want| + |arg64| + |b|)
  1.1 is SiLU's Lipschitz constant; FiLM multiplies w by t1 and maps b to b t1 + t2 (the caller passes those).

The RMS kinds have no subtraction: the project's rel_l2 < 5e-7 stays their bound.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
RHO0 = 4e-7
REL = 5e-7            # the project's rel-L2 bound of the fp32 norm kernels against fp64

FAMILIES = ("A", "B30", "B1e3", "B-1e3", "B1e4", "C", "D", "E40", "E1e-7", "F")


def k_tree(n):
    """k_m of an fp32 tree reduction over n elements."""
    return math.ceil(math.log2(n)) + 2 if n > 1 else 2


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def family(name, shape, seed=0):
    """A seeded fp32 tensor of one data family.  D takes shape [B, C, *spatial]: sample 0 is exactly zero, so are planes
    (b, c) with b + c odd of the other samples; plane (1, 0) is exactly 3.0 where the plane size is a power of two (the mean
    is then exact); the rest is family A."""
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(name) + seed)
    r = torch.randn(shape, generator=g, dtype=torch.float32)
    if name == "A":
        return 3.0 * r + 0.7
    if name.startswith("B"):
        return r + float(name[1:])
    if name == "C":
        return 1000.0 + 1e-3 * r
    if name == "E40":
        return 2.0 ** -40 * r
    if name == "E1e-7":
        return 1e-7 * r
    if name == "F":
        return 2.0 ** 40 * r
    assert name == "D" and len(shape) >= 3
    x = 3.0 * r + 0.7
    x[0] = 0.0
    for b in range(1, shape[0]):
        for c in range(shape[1]):
            if (b + c) % 2:
                x[b, c] = 0.0
    if shape[0] > 1 and is_pow2(int(np.prod(shape[2:]))):
        x[1, 0] = 3.0
    return x


class Stats:
    """fp64 statistics of groups x [..., n] (an fp32 or fp64 tensor; the last axis is reduced) and the bounds they imply."""

    def __init__(self, x, eps, k_m, fp64_onepass):
        x = x.double()
        self.eps, self.k_m = float(eps), k_m
        self.mean = x.mean(-1)
        self.var = ((x - self.mean[..., None]) ** 2).mean(-1)
        self.ms = (x * x).mean(-1)
        self.rstd = 1.0 / torch.sqrt(self.var + self.eps)
        self.rms_den = torch.sqrt(self.ms + self.eps)
        self.dm = k_m * U * x.abs().mean(-1)
        c64 = 2.0 ** -51 * self.ms / (self.var + self.eps) if fp64_onepass else 0.0
        self.rho = RHO0 + self.dm ** 2 / (2.0 * (self.var + self.eps)) + c64

    def mean_ratio(self, mean):
        """max over groups of |mean - mean64| / dm (0 where both vanish)."""
        err = (mean.double() - self.mean).abs()
        return float(torch.where(err == 0, torch.zeros_like(err), err / self.dm.clamp_min(1e-300)).max())

    def rstd_ratio(self, rstd):
        return float(((rstd.double() / self.rstd - 1.0).abs() / self.rho).max())

    def rms_ratio(self, den):
        """Kind 1 (no subtraction, no mean): the RMS denominator against RHO0."""
        return float(((den.double() / self.rms_den - 1.0).abs() / RHO0).max())


def silu64(v):
    return v / (1.0 + torch.exp(-v))


def element_ratio(got, x, st, w, b, slack_rel=0.0, slack_abs=0.0):
    """max |got - want| / bound of the element bound.  x [..., n] as given to Stats (st); w, b broadcast against x (fp64;
    with FiLM: w t1 and b t1 + t2).  slack_rel |want| + slack_abs is added to the bound: the storage format of a result that
    is not read back as fp32.  -> (ratio, max |got - want|)."""
    x = x.double()
    d = (x - st.mean[..., None]).abs()
    arg = (x - st.mean[..., None]) * st.rstd[..., None] * w + b
    want = silu64(arg)
    bound = 1.1 * abs(w) * st.rstd[..., None] * (st.dm[..., None] + st.rho[..., None] * d) \
        + 4.0 * U * (want.abs() + arg.abs() + abs(b)) + slack_rel * want.abs() + slack_abs
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max()), float(err.max())


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
