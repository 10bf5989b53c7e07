"""The error model of the transformer-side norm kernels -- k_token_ln (ds_tokens.hip), k_channel_rms (ds_convit.hip) and
k_token_l2norm (ds_small.hip) -- and the token-wise data families that stress it (plain torch, no GPU).  The vocabulary of
tests/norm_bounds.py: every reference is fp64 computed FROM THE fp32 INPUT VALUES, u = 2^-24, k_tree(E) = ceil(log2 E) + 2.
Tensors are channel-major [B, E, L]; the reduced axis is E, so the references work on the transpose [B, L, E].

Token LayerNorm with modulation: n = (x - mean) rstd w + b, y = n (1 + sc) + sh.
    |got - want| <= |w (1 + sc)| rstd64 (dm + rho |x - mean64|) + 4u (|want| + |n64 (1 + sc)| + |b (1 + sc)| + |sh|)
    dm = k_tree(E) u mean_e |x - mean64|,   rho = RHO0 + dm^2 / (2 (var64 + eps))
  dm is DEVIATION-based, not magnitude-based as in norm_bounds: the kernel's comment claims that the mean is never rounded to the
  magnitude of x, i.e. that the centred values x - mean carry the error of a tree sum of the deviations only.  An unshifted
  two-pass kernel rounds its mean to ulp(|mean|) and misses this bound by |mean| / std on families B and C.  rho as in
  norm_bounds (RHO0 = 7u for (float)var, + eps, sqrtf and the reciprocal; dm^2 / (2 (var + eps)) for a second moment centred
  dm off).  The 4u terms: the roundings of the subtraction, the products with rstd, w, (1 + sc) (itself rounded) and the two sums,
  each relative to the intermediate it rounds.

Channel RMSNorm: want = x / sqrt(ms64 + eps) w + mod, then the mean over f x f pixels when pool = f > 1.
    unpooled:  |got - want| <= (k_tree(E) / 2 + 6) u |x / den64 w| + 2u |mod|
  the sum of squares is a tree of ceil(log2 E) additions of terms that carry one rounding each (the square), divided by E: a
  relative error of k_tree(E) u, all terms being positive, which the square root halves.  + eps counts half through the root, sqrtf,
  the division x / den, the product with w and the sum with mod are one rounding each (4.5 u), and 1.5 u of slack is left for the
  device's sqrtf and division.  The sum with mod also rounds relative to |mod|: u |mod|, and another u |mod| of slack.
    pooled:    the mean of the f^2 pixel bounds + (2 log2 f + 2) u mean(|terms|)
  the butterfly adds f^2 terms in log2(f^2) = 2 log2 f levels, each a rounding relative to at most the sum of |terms|; the product
  with 1 / f^2 is exact (a power of two) and counts once with one u of slack.

Token L2 normalise: want = x / (||x||_2 + eps) gain, the sum of squares taken sequentially over C.
    |got - want| <= ((C + 1) / 2 + 6) u |want|
  the a-priori bound of recursive summation: C - 1 additions and one rounding per square give (C + 1) u on the sum of positive
  terms (first order, counting the first term's C - 1 additions for all), halved by the root; sqrtf, + eps, the division and the
  product with gain are one rounding each, and two u of slack for the device's sqrtf and division.
"""
import math

import torch

from tests import norm_bounds as nb
from tests.norm_bounds import U, RHO0, k_tree

L2_EPS = 1e-8                  # the project's eps of token_l2_normalize
TOKEN_FAMILIES = ("A", "B1e4", "B-1e3", "C", "E40", "E1e-7", "F", "P0", "P0neg", "Pmid", "Z")
_OWN = ("P0", "P0neg", "Pmid", "Z")


def token_family(name, shape, seed=0):
    """A seeded fp32 tensor [B, E, L] of one token-wise family.  norm_bounds.family for its names; P0: family A with channel 0 of
    every token = 1e6 (1 + 0.1 rand); P0neg: channel 0 = -3e4; Pmid: the P0 outlier in channel 5 (the control: the pivot is an
    ordinary value); Z: sample 0 is family A, in sample 1 token 0 is all zeros, token 1 the constant 7.0, the rest family A."""
    if name not in _OWN:
        return nb.family(name, shape, seed)
    B, E, L = shape
    x = nb.family("A", shape, seed)
    g = torch.Generator().manual_seed(7000 + 100 * _OWN.index(name) + seed)
    if name in ("P0", "Pmid"):
        c = 0 if name == "P0" else 5
        assert E > c
        x[:, c, :] = 1e6 * (1.0 + 0.1 * torch.rand(B, L, generator=g))
    elif name == "P0neg":
        x[:, 0, :] = -3e4
    else:
        assert B >= 2 and L >= 2
        x[1, :, 0] = 0.0
        x[1, :, 1] = 7.0
    return x


class TokenStats(nb.Stats):
    """norm_bounds.Stats of tokens [..., E] with the deviation-based dm (and the rho it implies) of the module docstring."""

    def __init__(self, x, eps):
        E = x.shape[-1]
        super().__init__(x, eps, k_tree(E), False)
        self.dm = self.k_m * U * (x.double() - self.mean[..., None]).abs().mean(-1)
        self.rho = RHO0 + self.dm ** 2 / (2.0 * (self.var + self.eps))


def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return ratio, err


def ln_reference(x, w, b, sc, sh, eps):
    """x [B, E, L] fp32; w, b [E]; sc, sh [B, E] or None -> (want, bound), fp64 [B, E, L]."""
    B, E, L = x.shape
    t = x.double().transpose(1, 2)                                   # [B, L, E]
    st = TokenStats(x.transpose(1, 2), eps)
    w, b = w.double().view(1, 1, E), b.double().view(1, 1, E)
    one_sc = 1.0 + (sc.double().reshape(B, 1, E) if sc is not None else torch.zeros(1, 1, E, dtype=torch.float64))
    sh = sh.double().reshape(B, 1, E) if sh is not None else torch.zeros(1, 1, E, dtype=torch.float64)
    dev = t - st.mean[..., None]
    n = dev * st.rstd[..., None] * w + b
    want = n * one_sc + sh
    bound = (w * one_sc).abs() * st.rstd[..., None] * (st.dm[..., None] + st.rho[..., None] * dev.abs()) \
        + 4.0 * U * (want.abs() + (n * one_sc).abs() + (b * one_sc).abs() + sh.abs())
    return want.transpose(1, 2), bound.transpose(1, 2)


def ln_ratio(got, x, w, b, sc, sh, eps):
    """-> (error / bound [B, E, L], max |got - want|)."""
    want, bound = ln_reference(x, w, b, sc, sh, eps)
    ratio, err = _ratio(got, want, bound)
    return ratio, float(err.max())


def rms_reference(x, w, mod, pool, eps):
    """x [B, E, H, W] fp32; w [E]; mod [B, E] or None; pool a power of two -> (want, bound), fp64 [B, E, H // pool, W // pool]."""
    B, E, H, W = x.shape
    t = x.double()
    den = torch.sqrt((t * t).mean(1, keepdim=True) + eps)
    nw = t / den * w.double().view(1, E, 1, 1)
    m = mod.double().reshape(B, E, 1, 1) if mod is not None else torch.zeros(1, E, 1, 1, dtype=torch.float64)
    want = nw + m
    bound = (k_tree(E) / 2.0 + 6.0) * U * nw.abs() + 2.0 * U * m.abs()
    if pool > 1:
        f = pool
        OH, OW = H // f, W // f

        def pooled(v):
            return v[:, :, :OH * f, :OW * f].reshape(B, E, OH, f, OW, f).mean(dim=(3, 5))

        bound = pooled(bound.expand_as(want)) + (2.0 * math.log2(f) + 2.0) * U * pooled(want.abs())
        want = pooled(want)
    return want, bound


def rms_ratio(got, x, w, mod, pool, eps):
    want, bound = rms_reference(x, w, mod, pool, eps)
    ratio, err = _ratio(got, want, bound.expand_as(want))
    return ratio, float(err.max())


def l2_reference(x, eps, gain):
    """x [B, C, L] fp32 (the normalised slice) -> (want, bound) fp64."""
    t = x.double()
    want = t / (torch.linalg.vector_norm(t, dim=1, keepdim=True) + eps) * gain
    return want, ((x.shape[1] + 1) / 2.0 + 6.0) * U * want.abs()


def l2_ratio(got, x, eps, gain):
    want, bound = l2_reference(x, eps, gain)
    ratio, err = _ratio(got, want, bound)
    return ratio, float(err.max())
