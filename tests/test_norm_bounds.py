"""The error model of tests/norm_bounds.py admits correct fp32 implementations and rejects a subtly wrong one (CPU only).

Admitted, on every data family and plane sizes 16 .. 65536, six draws each: a two-pass variance written with torch's fp32
reductions, an fp32 emulation of ds_norm.hip's two-pass register reductions (k_inorm_wave / k_inorm_block / k_inorm_generic: the
same grouping of the sums), and the fp64 one-pass statistics of ds_gnorm.hip (k_g1_partial / k_g1_final).  Rejected on the
mean-dominated families: a one-pass fp32 variance, sum(x^2)/n - mean^2, which is what a reduction that squares in fp32 amounts to.

torch's own fp32 group_norm is admitted on the families without a dominating mean only.  Its CPU kernel merges per-lane and
per-chunk (mean, m2) pairs, Welford's way, and every merge moves an fp32 running mean: on randn + r its variance is off by a
relative u r / std in the first order, which a two-pass reduction is not.  Measured with six draws per size: 1.2 times the
bound at r = 30 (n = 16), 21 and 23 times at r = +-1e3 (n = 64), 19 times at r = 1e4; its mean stays below 0.25 of the mean
bound everywhere.  The model is meant to tell a two-pass tree from anything weaker, and it does so here as well."""
import numpy as np
import pytest
import torch

from tests import norm_bounds as nb

SIZES = (16, 64, 175, 256, 864, 1024, 1089, 4096, 10000, 16384, 65536)
DRAWS = 6
EPS = 1e-5
f32 = np.float32


def _planes(fam, n):
    if fam == "D":
        x = nb.family("D", (2, 3, n), seed=n)
        return torch.cat([x.reshape(6, n)[:DRAWS]])
    return nb.family(fam, (DRAWS, n), seed=n)


def torch_two_pass(x):
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + EPS)


def torch_group_norm(x):
    P, n = x.shape
    _, mean, rstd = torch.native_group_norm(x.view(1, P, n), None, None, 1, P, n, P, EPS)
    return mean.view(P), rstd.view(P)


def _tree(per_thread):
    """Thread partials [P, T] (T a multiple of 64) -> the kernels' sum: an xor butterfly over each wave, then the waves in
    index order (block_sum), all in fp32."""
    P, T = per_thread.shape
    a = per_thread.reshape(P, T // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = (a + a[:, :, lane ^ o]).astype(f32)
    t = np.zeros(P, f32)
    for k in range(T // 64):
        t = (t + a[:, k, 0]).astype(f32)
    return t


def _layout(x, T, vec):
    """[P, n] -> values [P, VPT, T, vec] as thread t holds them (element idx = t + T i, vec floats each) and their mask."""
    P, n = x.shape
    nv = n // vec
    vpt = -(-nv // T)
    v = np.zeros((P, vpt * T * vec), f32)
    m = np.zeros((P, vpt * T * vec), bool)
    v[:, :n], m[:, :n] = x, True
    return v.reshape(P, vpt, T, vec), m.reshape(P, vpt, T, vec)


def _thread_sum(v):
    """Per-thread partial of [P, VPT, T, vec]: (x + y) + (z + w) per vector, the vectors added in order."""
    if v.shape[-1] == 4:
        g = ((v[..., 0] + v[..., 1]).astype(f32) + (v[..., 2] + v[..., 3]).astype(f32)).astype(f32)
    else:
        g = v[..., 0]
    s = np.zeros((v.shape[0], v.shape[2]), f32)
    for i in range(v.shape[1]):
        s = (s + g[:, i]).astype(f32)
    return s


def emulated_two_pass(x):
    """ds_norm.hip, kind 0: launch_inorm's choice of threads and vector width by plane size, two passes in fp32."""
    x = x.numpy().astype(f32)
    P, n = x.shape
    hw4 = n // 4
    if n % 4 == 0 and hw4 <= 16384:
        T, vec = (64 if hw4 <= 256 else 256 if hw4 <= 4096 else 1024), 4
    else:
        T, vec = 256, 1
    v, m = _layout(x, T, vec)
    inv = f32(1.0) / f32(n)
    mean = (_tree(_thread_sum(v)) * inv).astype(f32)
    a = np.where(m, (v - mean[:, None, None, None]).astype(f32), f32(0))
    var = (_tree(_thread_sum((a * a).astype(f32))) * inv).astype(f32)
    rstd = (f32(1.0) / np.sqrt((var + f32(EPS)).astype(f32))).astype(f32)
    return torch.from_numpy(mean), torch.from_numpy(rstd)


def fp64_one_pass(x):
    """ds_gnorm.hip: sums of x and x^2 in fp64, q/n - mean^2, rounded once."""
    d = x.double()
    n = x.shape[1]
    mean = d.sum(-1) / n
    var = ((d * d).sum(-1) / n - mean * mean).clamp_min(0.0)
    return mean.float(), 1.0 / torch.sqrt(var.float() + torch.tensor(EPS, dtype=torch.float32))


def fp32_one_pass(x):
    """The negative control: the three-line variance that cancels."""
    mean = x.sum(-1) / x.shape[1]
    var = ((x * x).sum(-1) / x.shape[1] - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + EPS)


def fp32_squares(x):
    """ds_gnorm.hip's 16-byte path as it was: (x0^2 + x1^2) + (x2^2 + x3^2) in fp32, then fp64 sums and q/n - mean^2."""
    P, n = x.shape
    v = x[:, :n // 4 * 4].view(P, n // 4, 4)
    fs = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
    fq = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + (v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3])
    t = x[:, n // 4 * 4:].double()
    mean = (fs.double().sum(-1) + t.sum(-1)) / n
    var = ((fq.double().sum(-1) + (t * t).sum(-1)) / n - mean * mean).clamp_min(0.0)
    return mean.float(), 1.0 / torch.sqrt(var.float() + torch.tensor(EPS, dtype=torch.float32))


def apply_fp32(x, mean, rstd, w, b):
    return torch.nn.functional.silu((x - mean[:, None]) * rstd[:, None] * w + b)


IMPLS = {"torch fp32 two-pass": (torch_two_pass, None, False), "two-pass fp32 emulation": (emulated_two_pass, None, False),
         "fp64 one-pass": (fp64_one_pass, 2, True)}


def _ratios(impl, k_m, onepass, fam, elements=True):
    worst = 0.0
    for n in SIZES:
        x = _planes(fam, n)
        st = nb.Stats(x, EPS, nb.k_tree(n) if k_m is None else k_m, onepass)
        mean, rstd = impl(x)
        assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        r = [st.mean_ratio(mean), st.rstd_ratio(rstd)]
        if elements:
            g = torch.Generator().manual_seed(n)
            w, b = torch.randn(x.shape[0], 1, generator=g), torch.randn(x.shape[0], 1, generator=g)
            got = apply_fp32(x, mean, rstd, w, b)
            assert torch.isfinite(got).all()
            r.append(nb.element_ratio(got, x, st, w.double(), b.double())[0])
        worst = max(worst, *r)
    return worst


@pytest.mark.parametrize("fam", nb.FAMILIES)
@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_the_bound_admits_correct_implementations(impl, fam):
    fn, k_m, onepass = IMPLS[impl]
    worst = _ratios(fn, k_m, onepass, fam, elements=fam != "B1e4")       # r = 1e4: the statistics checks only
    print(f"{impl:24s} family {fam:6s}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (impl, fam, worst)


@pytest.mark.parametrize("fam", nb.FAMILIES)
def test_torch_group_norm_against_the_bound(fam):
    """Mean: every family.  rstd and elements: the families without a dominating mean (module docstring); the others print."""
    pinned = not fam.startswith("B")
    worst_m = worst = 0.0
    for n in SIZES:
        x = _planes(fam, n)
        st = nb.Stats(x, EPS, nb.k_tree(n), False)
        mean, rstd = torch_group_norm(x)
        worst_m = max(worst_m, st.mean_ratio(mean))
        worst = max(worst, st.rstd_ratio(rstd), nb.element_ratio(apply_fp32(x, mean, rstd, 1.0, 0.0), x, st, 1.0, 0.0)[0])
    print(f"torch group_norm, family {fam:6s}: mean error / bound = {worst_m:.3f}, rstd and element error / bound = {worst:.3f}"
          + ("" if pinned else " (not asserted)"))
    assert worst_m <= 1.0 and (worst <= 1.0 or not pinned), (fam, worst_m, worst)


@pytest.mark.parametrize("fam", ["B1e3", "B-1e3", "B1e4", "C"])
def test_the_bound_rejects_a_one_pass_fp32_variance(fam):
    worst = 0.0
    for n in SIZES:
        x = _planes(fam, n)
        st = nb.Stats(x, EPS, nb.k_tree(n), False)
        worst = max(worst, st.rstd_ratio(fp32_one_pass(x)[1]))
    print(f"one-pass fp32 variance, family {fam}: worst rstd error / bound = {worst:.1f}")
    assert worst > 3.0, (fam, worst)


@pytest.mark.parametrize("fam", ["B1e3", "B-1e3", "B1e4", "C"])
def test_the_bound_rejects_fp32_squares_under_fp64_sums(fam):
    """What k_g1_partial's vector path did before it widened its elements: fp64 sums do not help once the squares are fp32."""
    worst = 0.0
    for n in SIZES:
        x = _planes(fam, n)
        st = nb.Stats(x, EPS, 2, True)
        worst = max(worst, st.rstd_ratio(fp32_squares(x)[1]))
    print(f"fp32 squares, fp64 sums, family {fam}: worst rstd error / bound = {worst:.1f}")
    assert worst > 3.0, (fam, worst)


def test_the_control_family_does_not_tell_them_apart():
    """On 3 randn + 0.7, the data every norm test used before, the one-pass fp32 variance passes: that data pins nothing."""
    worst = max(nb.Stats(_planes("A", n), EPS, nb.k_tree(n), False).rstd_ratio(fp32_one_pass(_planes("A", n))[1]) for n in SIZES)
    assert worst <= 1.0, worst


def test_family_d_planes():
    x = nb.family("D", (2, 3, 16, 16))
    assert not x[0].any() and not x[1, 2].any() and (x[1, 0] == 3.0).all() and x[1, 1].std() > 1
    assert not (nb.family("D", (2, 3, 5, 7))[1, 0] == 3.0).all()
