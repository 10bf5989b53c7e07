"""The error model of tests/token_norm_bounds.py rejects what it should and admits what it should (CPU only).

Three fp32 emulations of a token LayerNorm, numpy with a pairwise tree over E and one rounding per operation:
  unshifted   mean = sum(x) / E, c = x - mean, var = sum(c^2) / E: the textbook two-pass.  Its mean is rounded to ulp(|mean|), so
              it misses the deviation-based bound on the mean-dominated families (C, B1e4) by orders of magnitude.
  pivot       d = x - K with K the token's first channel, dm = sum(d) / E, c = d - dm, var = sum(c^2) / E: k_token_ln as it was.
              Exact on B and C (x - K is exact by Sterbenz), but an outlier in channel 0 rounds every other channel to ulp(K):
              it misses the bound on P0 and P0neg -- and on those alone.
  recentred   m1 = fl(K + sum(x - K) / E), d = x - m1, dm = sum(d) / E, c = d - dm, var = sum(c^2) / E: k_token_ln as it is.  At
              most half the bound on every family and width.
The RMS and L2 bounds get the same two-sided check: an fp32 emulation of the kernel's order stays below half the bound; a sum
of squares rounded to fp16, or taken over half the channels, fails."""
import numpy as np
import pytest
import torch

from tests import token_norm_bounds as tb

WIDTHS = (8, 9, 48, 64, 200, 256, 1024)
TOKENS = 37
EPS = 1e-5
RMS_EPS = float(torch.finfo(torch.float32).eps)
f32 = np.float32


def tree(a):
    """Pairwise fp32 sum over the last axis (zero-padded to a power of two)."""
    n = a.shape[-1]
    p = 1 << max(n - 1, 0).bit_length()
    v = np.zeros(a.shape[:-1] + (p,), f32)
    v[..., :n] = a
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(f32)
    return v[..., 0]


def ln_emulation(order, x, w, b, sc, sh, eps=EPS):
    """x [B, E, L] torch fp32 -> the fp32 LayerNorm + modulation of one of the three orders, [B, E, L] torch fp32."""
    t = x.transpose(1, 2).contiguous().numpy().astype(f32)             # [B, L, E]
    B, L, E = t.shape
    inv = f32(1.0) / f32(E)
    if order == "unshifted":
        mean = (tree(t) * inv).astype(f32)
        c = (t - mean[..., None]).astype(f32)
    else:
        K = t[..., :1]
        d = (t - K).astype(f32)
        if order == "recentred":
            m1 = (K + (tree(d) * inv).astype(f32)[..., None]).astype(f32)
            d = (t - m1).astype(f32)
        else:
            assert order == "pivot"
        dm = (tree(d) * inv).astype(f32)
        c = (d - dm[..., None]).astype(f32)
    var = (tree((c * c).astype(f32)) * inv).astype(f32)
    rstd = (f32(1.0) / np.sqrt((var + f32(eps)).astype(f32)).astype(f32)).astype(f32)
    w, b = w.numpy().astype(f32).reshape(1, 1, E), b.numpy().astype(f32).reshape(1, 1, E)
    n = (((c * rstd[..., None]).astype(f32) * w).astype(f32) + b).astype(f32)
    one_sc = (f32(1.0) + sc.numpy().astype(f32).reshape(B, 1, E)).astype(f32)
    y = ((n * one_sc).astype(f32) + sh.numpy().astype(f32).reshape(B, 1, E)).astype(f32)
    return torch.from_numpy(y).transpose(1, 2)


def ln_inputs(fam, E):
    x = tb.token_family(fam, (2, E, TOKENS), seed=E)
    g = torch.Generator().manual_seed(E)
    w, b = 1 + 0.25 * torch.randn(E, generator=g), 0.25 * torch.randn(E, generator=g)
    sc, sh = torch.randn(2, E, generator=g), torch.randn(2, E, generator=g)
    return x, w, b, sc, sh


def ln_worst(order, fam, E):
    x, w, b, sc, sh = ln_inputs(fam, E)
    got = ln_emulation(order, x, w, b, sc, sh)
    assert torch.isfinite(got).all()
    return float(tb.ln_ratio(got, x, w, b, sc, sh, EPS)[0].max())


@pytest.mark.parametrize("fam", tb.TOKEN_FAMILIES)
def test_the_layernorm_bound_admits_the_recentred_order(fam):
    worst = {E: ln_worst("recentred", fam, E) for E in WIDTHS}
    print(f"re-centred LayerNorm, family {fam:6s}: error / bound = " + ", ".join(f"E={E}: {r:.3f}" for E, r in worst.items()))
    assert max(worst.values()) <= 0.5, (fam, worst)


@pytest.mark.parametrize("fam", ["C", "B1e4"])
def test_the_layernorm_bound_rejects_an_unshifted_mean(fam):
    worst = {E: ln_worst("unshifted", fam, E) for E in WIDTHS}
    print(f"unshifted LayerNorm, family {fam}: error / bound = " + ", ".join(f"E={E}: {r:.3g}" for E, r in worst.items()))
    assert min(worst.values()) > 3.0, (fam, worst)


@pytest.mark.parametrize("fam", ["P0", "P0neg"])
def test_the_layernorm_bound_rejects_the_first_channel_shift(fam):
    """Every width from 48 on misses the bound, the wide ones by far: the bound's dm term falls with the outlier's share of the
    token, 1 / E, and what ulp(K) costs does not (at E = 8 and 9 the pivot order still passes, at 0.4 - 0.9 of the bound)."""
    worst = {E: ln_worst("pivot", fam, E) for E in WIDTHS if E >= 48}
    print(f"first-channel shift, family {fam}: error / bound = " + ", ".join(f"E={E}: {r:.3g}" for E, r in worst.items()))
    assert min(worst.values()) > 1.0 and max(worst.values()) > 10.0, (fam, worst)


@pytest.mark.parametrize("fam", [f for f in tb.TOKEN_FAMILIES if f not in ("P0", "P0neg")])
def test_the_first_channel_shift_fails_on_nothing_else(fam):
    """The pivot order is a correct kernel wherever channel 0 is an ordinary value, Pmid (the same outlier elsewhere) included:
    the model singles out the pivot, not the outlier."""
    worst = max(ln_worst("pivot", fam, E) for E in WIDTHS)
    print(f"first-channel shift, family {fam:6s}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (fam, worst)


# ------------------------------------------------------------------------------------------------------------------------ RMS
RMS_FAMILIES = ("A", "E40", "F", "P0", "Pmid", "Z")


def rms_emulation(kind, x, w, mod, pool, eps=RMS_EPS):
    """x [B, E, H, W]: k_channel_rms's arithmetic in fp32 (tree sum of squares, sqrtf(tot / E + eps), x / norm * w + mod, the
    butterfly over the f^2 pixels, * 1 / f^2); kind 'fp16': the sum of squares rounded to fp16; 'half': taken over E / 2 channels."""
    B, E, H, W = x.shape
    t = x.permute(0, 2, 3, 1).contiguous().numpy().astype(f32)         # [B, H, W, E]
    sq = (t * t).astype(f32)
    if kind == "half":
        sq = sq[..., :E // 2]
    tot = tree(sq)
    if kind == "fp16":
        with np.errstate(over="ignore"):
            tot = tot.astype(np.float16).astype(f32)
    norm = np.sqrt(((tot / f32(E)).astype(f32) + f32(eps)).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore"):
        y = ((t / norm[..., None]).astype(f32) * w.numpy().astype(f32)).astype(f32)
    y = (y + mod.numpy().astype(f32).reshape(B, 1, 1, E)).astype(f32)
    if pool > 1:
        f = pool
        OH, OW = H // f, W // f
        y = y[:, :OH * f, :OW * f].reshape(B, OH, f, OW, f, E).transpose(0, 1, 3, 5, 2, 4).reshape(B, OH, OW, E, f * f)
        y = (tree(y) * f32(1.0 / (f * f))).astype(f32)
    return torch.from_numpy(np.ascontiguousarray(y)).permute(0, 3, 1, 2)


def rms_inputs(fam, E, H, W):
    x = tb.token_family(fam, (2, E, H * W), seed=E + H).view(2, E, H, W).clone()
    g = torch.Generator().manual_seed(E + 1)
    return x, 1 + 0.25 * torch.randn(E, generator=g), torch.randn(2, E, generator=g)


@pytest.mark.parametrize("pool,H,W", [(1, 3, 5), (2, 6, 10), (4, 8, 12), (2, 9, 7)])
@pytest.mark.parametrize("fam", RMS_FAMILIES)
def test_the_rms_bound_admits_the_fp32_tree(fam, pool, H, W):
    worst = {}
    for E in WIDTHS:
        x, w, mod = rms_inputs(fam, E, H, W)
        got = rms_emulation("fp32", x, w, mod, pool)
        assert torch.isfinite(got).all()
        worst[E] = float(tb.rms_ratio(got, x, w, mod, pool, RMS_EPS)[0].max())
    print(f"fp32 RMSNorm, family {fam:5s} pool {pool} {H}x{W}: error / bound = " + ", ".join(f"E={E}: {r:.3f}" for E, r in worst.items()))
    assert max(worst.values()) <= 0.5, (fam, worst)


@pytest.mark.parametrize("kind", ["fp16", "half"])
@pytest.mark.parametrize("pool", [1, 2])
def test_the_rms_bound_rejects_a_wrong_sum_of_squares(kind, pool):
    worst = {}
    for E in WIDTHS:
        x, w, mod = rms_inputs("A", E, 6, 10)
        worst[E] = float(tb.rms_ratio(rms_emulation(kind, x, w, mod, pool), x, w, mod, pool, RMS_EPS)[0].max())
    print(f"RMSNorm, sum of squares {kind}, pool {pool}: error / bound = " + ", ".join(f"E={E}: {r:.3g}" for E, r in worst.items()))
    assert min(worst.values()) > 3.0, (kind, worst)


# ------------------------------------------------------------------------------------------------------------------------- L2
L2_FAMILIES = ("A", "E40", "F", "P0")


def l2_emulation(kind, x, eps, gain):
    """x [B, C, L]: k_token_l2norm's arithmetic in fp32 (squares summed in channel order, sqrtf(ss) + eps, x / den * gain)."""
    t = x.numpy().astype(f32)
    C = t.shape[1] // 2 if kind == "half" else t.shape[1]
    ss = np.zeros((t.shape[0], t.shape[2]), f32)
    for c in range(C):
        ss = (ss + (t[:, c] * t[:, c]).astype(f32)).astype(f32)
    if kind == "fp16":
        with np.errstate(over="ignore"):
            ss = ss.astype(np.float16).astype(f32)
    den = (np.sqrt(ss).astype(f32) + f32(eps)).astype(f32)
    with np.errstate(invalid="ignore"):
        return torch.from_numpy(((t / den[:, None]).astype(f32) * f32(gain)).astype(f32))


@pytest.mark.parametrize("fam", L2_FAMILIES)
def test_the_l2_bound_admits_the_sequential_fp32_sum(fam):
    worst = {}
    for C in WIDTHS:
        x = tb.token_family(fam, (2, C, TOKENS), seed=C)
        got = l2_emulation("fp32", x, tb.L2_EPS, 4.0)
        assert torch.isfinite(got).all()
        worst[C] = float(tb.l2_ratio(got, x, tb.L2_EPS, 4.0)[0].max())
    print(f"fp32 L2 normalise, family {fam:4s}: error / bound = " + ", ".join(f"C={C}: {r:.3f}" for C, r in worst.items()))
    assert max(worst.values()) <= 0.5, (fam, worst)


@pytest.mark.parametrize("kind", ["fp16", "half"])
def test_the_l2_bound_rejects_a_wrong_sum_of_squares(kind):
    worst = {}
    for C in WIDTHS:
        x = tb.token_family("A", (2, C, TOKENS), seed=C)
        worst[C] = float(tb.l2_ratio(l2_emulation(kind, x, tb.L2_EPS, 4.0), x, tb.L2_EPS, 4.0)[0].max())
    print(f"L2 normalise, sum of squares {kind}: error / bound = " + ", ".join(f"C={C}: {r:.3g}" for C, r in worst.items()))
    assert min(worst.values()) > 3.0, (kind, worst)


def test_the_families():
    x = tb.token_family("Z", (2, 9, 5))
    assert not x[1, :, 0].any() and (x[1, :, 1] == 7.0).all() and x[0].std() > 1 and x[1, :, 2:].std() > 1
    p = tb.token_family("P0", (2, 9, 5))
    assert (p[:, 0] >= 1e6).all() and (p[:, 0] <= 1.1e6 * (1 + 1e-6)).all() and p[:, 1:].abs().max() < 50
    assert (tb.token_family("P0neg", (2, 9, 5))[:, 0] == -3e4).all()
    q = tb.token_family("Pmid", (2, 9, 5))
    assert (q[:, 5] >= 1e6).all() and q[:, :5].abs().max() < 50
