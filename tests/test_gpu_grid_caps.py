"""The streaming kernels past their grid caps, on a real MI355X.

Every memory-bound kernel of diffsci_amd/csrc caps its launch (about 2048 workgroups of 256 threads) and walks the rest of the
tensor in a grid-stride loop.  The other kernel tests stay below those caps, so the loop increments, the indices derived from a
second-trip index and the carried moduli of ds_inpaint.hip are first executed here: every case is sized just past the cap it is
named for and asserts that, from the constants below, in integer arithmetic before it launches.

No tolerance is new.  A comparison is bit equality where the kernel documents its reference's operation order or is a copy, a
maximum or a nearest pick; otherwise it is the rule of the named existing test for the same kernel, whose bound is torch-fp32's
own error against fp64 computed in the test.  The ops wrappers that had no direct test (lerp_stack, score, denoiser, tanh,
amax_merge, token_l2_normalize) get one at the end."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import adm_ref, philox_ref, punetg_ref  # noqa: E402
from oracle import karras_ref as K  # noqa: E402
from tests import vaenet_ref  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402
from tests.test_gpu_chunk_decode import SENTINEL, restated  # noqa: E402
from tests.test_gpu_dit import check_kernel  # noqa: E402
from tests.test_gpu_tiled_sampling import MODES, chain, chain64, referee, setitem_ref  # noqa: E402

# ---------------------------------------------------------------- 0. the caps, as data
# Each constant mirrors one line of a kernel source; CAP_SOURCES names the line by a pattern whose every group must still read the
# value (tests/test_host_logic.py::test_grid_caps_mirror_the_kernel_sources).  Who changes a cap is sent to the shapes below.
THREADS = 256            # ds_stepmath.h: constexpr int kThreads = 256;  the NT of ds_window / ds_resample / ds_gnorm / ds_groupnorm
GRID_FOR = 2048          # ds_stepmath.h grid_for: if (g > 2048) g = 2048;
WINDOW_BLOCKS = 2048     # ds_window.hip: constexpr unsigned MAX_BLOCKS = 2048;
WINDOW_PLANES = 1024     # ds_window.hip box_launch_shape: gy = planes < 1024u ? planes : 1024u;
RESAMPLE_BLOCKS = 2048   # ds_resample.hip: constexpr size_t MAX_BLOCKS = 2048;
POOLF_BLOCKS = 2048      # ds_gnorm.hip ds_gnorm1_apply_poolf: if (g > 2048) g = 2048;
GN_CHUNKS = 64           # ds_groupnorm.hip: constexpr int MAX_CHUNKS = 64;
FOURIER_BLOCKS = 8192    # ds_small.hip ds_fourier_channels: if (g > 8192) g = 8192;
FOURIER_THREADS = 256    # ds_small.hip ds_fourier_channels: dim3(256)
LINEAR_ROWS = 64         # ds_small.hip ds_linear: dim3 g((N + 3) / 4, M < 64 ? M : 64);
T = GRID_FOR * THREADS   # 524 288 threads: the most a capped one-dimensional launch has

CAP_SOURCES = [  # (name, value, source file, pattern)
    ("THREADS", THREADS, "ds_stepmath.h", r"constexpr int kThreads = (\d+);"),
    ("THREADS", THREADS, "ds_window.hip", r"constexpr int NT = (\d+);"),
    ("THREADS", THREADS, "ds_resample.hip", r"constexpr int NT = (\d+);"),
    ("THREADS", THREADS, "ds_gnorm.hip", r"constexpr int NT = (\d+);"),
    ("THREADS", THREADS, "ds_groupnorm.hip", r"constexpr int NT = (\d+);"),
    ("GRID_FOR", GRID_FOR, "ds_stepmath.h", r"if \(g > (\d+)\) g = (\d+);"),
    ("WINDOW_BLOCKS", WINDOW_BLOCKS, "ds_window.hip", r"constexpr unsigned MAX_BLOCKS = (\d+);"),
    ("WINDOW_PLANES", WINDOW_PLANES, "ds_window.hip", r"\(unsigned\)planes < (\d+)u \? \(unsigned\)planes : (\d+)u;"),
    ("RESAMPLE_BLOCKS", RESAMPLE_BLOCKS, "ds_resample.hip", r"constexpr size_t MAX_BLOCKS = (\d+);"),
    ("POOLF_BLOCKS", POOLF_BLOCKS, "ds_gnorm.hip", r"if \(g > (\d+)\) g = (\d+);"),
    ("GN_CHUNKS", GN_CHUNKS, "ds_groupnorm.hip", r"constexpr int MAX_CHUNKS = (\d+);"),
    ("FOURIER_BLOCKS", FOURIER_BLOCKS, "ds_small.hip", r"if \(g > (\d+)\) g = (\d+);"),
    ("FOURIER_THREADS", FOURIER_THREADS, "ds_small.hip", r"hipLaunchKernelGGL\(k_fourier_channels, dim3\(\(unsigned\)g\), dim3\((\d+)\)"),
    ("LINEAR_ROWS", LINEAR_ROWS, "ds_small.hip", r"dim3 g\(\(N \+ 3\) / 4, M < (\d+) \? M : (\d+)\);"),
]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffsci_amd", "csrc")


def trips(units, threads):
    """Loop trips of the busiest thread when `threads` threads stride over `units` units."""
    return -(-units // threads)


def capped(units, cap=GRID_FOR, threads=THREADS):
    """Threads of a one-dimensional launch sized by `units` and capped at `cap` workgroups (grid_for and its kin)."""
    return max(1, min(cap, -(-units // threads))) * threads


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


def aligned(t, dev):
    d = t.to(dev).contiguous()
    assert d.data_ptr() % 16 == 0
    return d


def shifted(t, dev):
    """The same values one float past a 16-byte boundary: torch.empty(n + 1)[1:], which every wrapper takes as contiguous."""
    v = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- 1. ds_step.hip: the second trip of the 16-byte loops
N_A = 4 * (T + 163840)       # 2 752 512: a whole number of 4-vectors, more of them than threads
N_B = N_A + 3                # the same vector body and a 3-element scalar tail that starts at 4 * n4


def assert_vector_loop_repeats(n, tail):
    n4 = n // 4
    assert capped(n4) == T and trips(n4, T) >= 2, (n, n4)                    # grid_elems(n4, n): at least one thread comes round again
    assert n - 4 * n4 == tail


def assert_scalar_loop_repeats(n):
    assert capped((n + 3) // 4) == T and trips(n, T) >= 2, n                # n4 = 0: grid_for(ceil(n / 4)) threads take everything


def _coef(**kw):
    from diffsci_amd._native import EvalCoef
    base = dict(c_out=1.0, c_skip=0.0, sigma_sq=1.0, neg_mult=-1.0, neg_lang=0.0, guidance=1.0, one_minus_guidance=0.0, input_kind=0,
                stochastic=0)
    base.update(kw)
    return EvalCoef(**base)


def _drift_cpu(xx, ff, fuu, r, g_):
    Fv = ff if fuu is None else (1 - g_) * fuu + g_ * ff
    D = r["c_out"] * Fv + r["c_skip"] * xx
    sc = (D - xx) / r["sigma_sq"]
    return r["neg_mult"] * sc


class StepCase:
    """The inputs of test_stepper_kernels_bit_exact (tests/test_gpu_kernels.py) at n elements and its reference expressions,
    torch-CPU fp32 in the kernels' operation order, evaluated once."""
    OPERANDS = ("x", "f1", "f2", "fu1", "fu2", "eps")
    GUIDE = (("plain", 1.0, False), ("guided", 2.0, True))

    def __init__(self, n):
        self.n = n
        g = torch.Generator().manual_seed(n)
        self.x, self.f1, self.f2, self.fu1, self.fu2, self.eps = (torch.randn(n, generator=g) * s for s in (80.0, 1.0, 1.0, 1.0, 1.0, 1.0))
        sig1, sig2 = torch.tensor(57.586), torch.tensor(40.786)
        self.dt = float(sig2 - sig1)
        self.rows = []
        for sg in (sig1, sig2):
            cs, co, ci, cn = K.edm_precond(sg)
            self.rows.append(dict(c_out=float(co), c_skip=float(cs), sigma_sq=float(sg ** 2), neg_mult=float(-(sg * (1 + 0 * sg)))))
        self.ci2 = float(K.edm_precond(sig2)[2])
        x, dt, want = self.x, self.dt, {}
        for tag, g_, guided in self.GUIDE:
            u1, u2 = (self.fu1, self.fu2) if guided else (None, None)
            d1 = _drift_cpu(x, self.f1, u1, self.rows[0], g_)
            xe = x + dt * d1
            d2 = _drift_cpu(xe, self.f2, u2, self.rows[1], g_)
            h = x + (0.5 * (d1 + d2)) * dt
            want[tag] = dict(euler=xe, euler_in=self.ci2 * xe, heun=h, heun_in=0.25 * h, drift=d1)
        self.want = want
        self.want_churn = x + 3.25 * self.eps
        self.want_scale, self.want_add = x * 80.0, x + self.f1

    def em(self, eps):
        """The Euler-Maruyama move of that test with the draw `eps`."""
        r = self.rows[0]
        sc = ((r["c_out"] * self.f1 + r["c_skip"] * self.x) - self.x) / r["sigma_sq"]
        d = r["neg_mult"] * sc
        d = d + (-0.7 * 57.586) * sc
        return self.x + d * self.dt + (1.3 * eps) * 0.9

    def coefs(self, g_, **kw):
        return tuple(_coef(guidance=g_, one_minus_guidance=1 - g_, **r, **kw) for r in self.rows)

    def em_coef(self):
        return _coef(stochastic=1, neg_lang=-0.7 * 57.586, **self.rows[0])


@pytest.fixture(scope="module")
def step_cases():
    made = {}

    def get(n):
        if n not in made:
            made.clear()                                              # one size at a time: a case holds about 200 MB of host memory
            made[n] = StepCase(n)
        return made[n]
    return get


def run_stepper(ops, dev, c, odd=None):
    """Every assertion of test_stepper_kernels_bit_exact on the case c; `odd` names the one operand (an input of OPERANDS, 'x_out'
    or 'xin_out') handed over one float off a 16-byte boundary."""
    n = c.n
    D = {k: (shifted if k == odd else aligned)(getattr(c, k), dev) for k in c.OPERANDS}

    def outs():
        mk = lambda k: (torch.empty(n + 1, device=dev)[1:] if k == odd else torch.empty(n, device=dev))         # noqa: E731
        return mk("x_out"), mk("xin_out")

    for tag, g_, guided in c.GUIDE:
        k1, k2 = c.coefs(g_)
        u1, u2 = (D["fu1"], D["fu2"]) if guided else (None, None)
        w = c.want[tag]
        xo, xi = outs()
        ops.euler(D["x"], D["f1"], k1, c.dt, fu=u1, x_out=xo, xin_out=xi, c_in_next=c.ci2)
        assert torch.equal(xo.cpu(), w["euler"]) and torch.equal(xi.cpu(), w["euler_in"]), (tag, odd)
        xo, xi = outs()
        ops.heun(D["x"], D["f1"], k1, D["f2"], k2, c.dt, f1u=u1, f2u=u2, x_out=xo, xin_out=xi, c_in_next=0.25)
        assert torch.equal(xo.cpu(), w["heun"]) and torch.equal(xi.cpu(), w["heun_in"]), (tag, odd)
        assert torch.equal(ops.drift(D["x"], D["f1"], k1, fu=u1).cpu(), w["drift"]), (tag, odd)
    xo, _ = outs()
    ops.euler(D["x"], D["f1"], c.em_coef(), c.dt, x_out=xo, eps=D["eps"], noise_coef=1.3, sqrt_abs_dt=0.9)
    assert torch.equal(xo.cpu(), c.em(c.eps)), odd
    xh, xi = outs()
    ops.churn(D["x"], D["eps"], 3.25, xhat_out=xh, xin_out=xi, c_in=0.125)
    assert torch.equal(xh.cpu(), c.want_churn) and torch.equal(xi.cpu(), 0.125 * c.want_churn), odd
    xo, _ = outs()
    assert torch.equal(ops.scale(D["x"], 80.0, out=xo).cpu(), c.want_scale), odd
    xo, _ = outs()
    assert torch.equal(ops.add(D["x"], D["f1"], out=xo).cpu(), c.want_add), odd
    return D


@pytest.mark.parametrize("n,tail", [(N_A, 0), (N_B, 3)], ids=["n_a", "n_b"])
def test_stepper_kernels_bit_exact_on_a_second_trip(ops, dev, step_cases, n, tail):
    """scale, add, euler (plain, injected eps, in-kernel Philox), heun (with and without the unconditional outputs), churn (injected,
    Philox): bit-equal to torch-CPU fp32 in the kernel's operation order where a thread's 16-byte loop runs twice."""
    assert_vector_loop_repeats(n, tail)
    c = step_cases(n)
    D = run_stepper(ops, dev, c)
    # in-kernel Philox: what the kernel computes from an injected copy of its own stream, which is the CPU expression on that copy
    st = torch.tensor([99, 1000], dtype=torch.int64, device=dev)
    eps = ops.philox_normal(st, 12, (n,))
    a = ops.euler(D["x"], D["f1"], c.em_coef(), c.dt, x_out=torch.empty(n, device=dev), eps=eps, noise_coef=1.3, sqrt_abs_dt=0.9)
    b = ops.euler(D["x"], D["f1"], c.em_coef(), c.dt, x_out=torch.empty(n, device=dev), philox=(st, 12), noise_coef=1.3, sqrt_abs_dt=0.9)
    assert torch.equal(a, b) and torch.equal(b.cpu(), c.em(eps.cpu()))
    a = ops.churn(D["x"], eps, 3.25, xhat_out=torch.empty(n, device=dev), xin_out=torch.empty(n, device=dev), c_in=0.125)
    xin = torch.empty(n, device=dev)
    b = ops.churn(D["x"], None, 3.25, xhat_out=torch.empty(n, device=dev), xin_out=xin, c_in=0.125, philox=(st, 12))
    assert torch.equal(a, b) and torch.equal(b.cpu(), c.x + 3.25 * eps.cpu()) and torch.equal(xin.cpu(), 0.125 * b.cpu())


def test_stepper_two_input_copies_on_a_second_trip(ops, dev, step_cases):
    """xin_copies = 2: both halves of the [2n] network input equal the single-copy result (the second copy starts n floats in)."""
    n = N_A
    assert_vector_loop_repeats(n, 0)
    c = step_cases(n)
    D = {k: aligned(getattr(c, k), dev) for k in c.OPERANDS}
    for tag, g_, guided in c.GUIDE:
        k1, k2 = c.coefs(g_, xin_copies=2)
        u1, u2 = (D["fu1"], D["fu2"]) if guided else (None, None)
        w = c.want[tag]
        xo, two = torch.empty(n, device=dev), torch.empty(2 * n, device=dev)
        ops.euler(D["x"], D["f1"], k1, c.dt, fu=u1, x_out=xo, xin_out=two, c_in_next=c.ci2)
        assert torch.equal(xo.cpu(), w["euler"]) and torch.equal(two[:n].cpu(), w["euler_in"]) and torch.equal(two[n:].cpu(), w["euler_in"])
        two = torch.empty(2 * n, device=dev)
        ops.heun(D["x"], D["f1"], k1, D["f2"], k2, c.dt, f1u=u1, f2u=u2, x_out=xo, xin_out=two, c_in_next=0.25)
        assert torch.equal(xo.cpu(), w["heun"]) and torch.equal(two[:n].cpu(), w["heun_in"]) and torch.equal(two[n:].cpu(), w["heun_in"])
    xh, two = torch.empty(n, device=dev), torch.empty(2 * n, device=dev)
    ops.churn(D["x"], D["eps"], 3.25, xhat_out=xh, xin_out=two, c_in=0.125, xin_copies=2)
    want = 0.125 * c.want_churn
    assert torch.equal(xh.cpu(), c.want_churn) and torch.equal(two[:n].cpu(), want) and torch.equal(two[n:].cpu(), want)


@pytest.mark.parametrize("odd", StepCase.OPERANDS + ("x_out", "xin_out"))
def test_stepper_misaligned_operand_takes_the_scalar_path(ops, dev, step_cases, odd):
    """One operand 4 bytes off: vec4_count gives 0 and the scalar loop covers all n elements, five trips and more per thread; the
    same bits."""
    assert_scalar_loop_repeats(N_A)
    run_stepper(ops, dev, step_cases(N_A), odd=odd)


def test_philox_stream_matches_oracle_on_a_second_trip(ops, dev):
    """The rule of test_philox_stream_matches_oracle (tests/test_gpu_round2.py) over all of n_b, at a non-zero base offset."""
    n, seed, base, off = N_B, 2**63 + 17, 2**40 + 3, 5
    assert_vector_loop_repeats(n, 3)
    i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v                 # noqa: E731
    st = torch.tensor([i64(seed), i64(base)], dtype=torch.int64, device=dev)
    got = ops.philox_normal(st, off, (n,)).cpu().double().numpy()
    want = philox_ref.normal(seed, base + off, n)
    assert np.abs(got - want).max() <= 4e-6 * (1.0 + np.abs(want).max())
    buf = torch.empty(n + 1, device=dev)
    assert_scalar_loop_repeats(n)
    shifted_out = ops.philox_normal(st, off, (n,), out=buf[1:]).cpu()     # 4-byte aligned only: the scalar path
    assert torch.equal(shifted_out, torch.from_numpy(got).float())


POSTERIOR_LARGE = [(3, 8, 56, 56, 56), (3, 2, 89, 89, 89)]               # n = 2 107 392, and 2 114 907 with n % 4 == 3


@pytest.mark.parametrize("shape", POSTERIOR_LARGE, ids=lambda s: "x".join(map(str, s)))
def test_posterior_on_a_second_trip(ops, dev, shape):
    """The rule of test_posterior_with_given_noise (tests/test_gpu_vaenet.py), with and without the clamp; then the Philox draw
    against the injected run on ops.philox_normal's draws at the documented counters (element e <- counter offset + e / 4)."""
    Z = shape[1] // 2
    n = shape[0] * Z * shape[2] * shape[3] * shape[4]
    n4 = (n + 3) // 4                                                      # k_posterior: a thread takes four consecutive elements
    assert capped(n4) == T and trips(n4, T) >= 2
    assert n % 4 == (0 if shape[1] == 8 else 3)
    torch.manual_seed(400)
    m = torch.randn(*shape)
    m[:, Z:] *= 4
    m[0, Z].flatten()[:3] = torch.tensor([-45.0, 31.0, 20.5])            # logvar outside (-30, 20)
    eps = torch.randn(shape[0], Z, *shape[2:])
    md, ed = m.to(dev), eps.to(dev)
    for clamp in (None, (-30.0, 20.0)):
        want = vaenet_ref.posterior(m.double(), eps.double(), clamp)
        got = ops.posterior_sample(md, ed, clamp=clamp)
        assert tuple(got.shape) == tuple(want.shape)
        err, own = rel_l2(got.cpu(), want), rel_l2(vaenet_ref.posterior(m, eps, clamp), want)
        print(f"posterior {shape} clamp={clamp}: {err:.2e} (torch fp32 {own:.2e})")
        assert err < 5e-7
        torch.manual_seed(5)
        off0 = torch.cuda.default_generators[dev.index].get_offset()
        a = ops.posterior_sample(md, clamp=clamp)
        state = torch.tensor([5, off0], dtype=torch.int64, device=dev)
        draws = ops.philox_normal(state, 0, a.shape)
        assert torch.equal(ops.posterior_sample(md, draws, clamp=clamp), a)
        assert torch.cuda.default_generators[dev.index].get_offset() >= off0 + n4


# ---------------------------------------------------------------- 2. ds_inpaint.hip: the carried position
SI_SHAPE = (3, 2, 76, 76, 76)     # the second trip lies inside the last sample: the carry advances and never wraps
SI_SHAPE_WRAP = (4, 2, 76, 76, 76)   # one sample more: second-trip threads on both sides of a sample's end, so the carry wraps for some


def si_geometry(shape):
    B, nps = shape[0], math.prod(shape[1:])
    assert nps % 4 == 0
    nps4, n4 = nps // 4, B * nps // 4
    return B, nps, nps4, n4, T % nps4


def assert_carry_is_live(shape, wraps):
    B, nps, nps4, n4, pstep = si_geometry(shape)
    assert capped(n4) == T and trips(n4, T) == 2 and pstep != 0          # k_si_inpaint: p = i % nps4, then p += stride % nps4
    i = np.arange(n4 - T, dtype=np.int64)                                  # the threads that come round again
    wrap = (i % nps4) + pstep >= nps4                                      # the conditional subtract of the carry
    assert bool((~wrap).any()) and bool(wrap.any()) == wraps, (shape, int(wrap.sum()))


def test_si_geometry_is_what_the_cases_assume():
    assert si_geometry(SI_SHAPE) == (3, 877952, 219488, 658464, 85312)
    assert_carry_is_live(SI_SHAPE, wraps=False)
    assert_carry_is_live(SI_SHAPE_WRAP, wraps=True)


class SICase:
    def __init__(self, shape, dev):
        import diffsci_amd.models as M
        from diffsci_amd._native import DS_IN_NETWORK
        from diffsci_amd.models.karras import siloop
        self.shape, self.dev, self.siloop = shape, dev, siloop
        g = torch.Generator().manual_seed(sum(shape))
        rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                           # noqa: E731
        one = (1,) + shape[1:]
        self.x, self.f, self.fu, self.x_orig = rnd(*shape), rnd(*shape), rnd(*shape), rnd(*one)
        self.eps = [rnd(*shape), rnd(*one), rnd(*shape), rnd(*one)]
        self.mask = torch.rand(*shape[1:], generator=g).to(dev)                          # a soft mask
        self.cfg = M.SIModuleConfig(scheduler="cosine", precondition_fn="edm")
        self.kind, self.guidance = DS_IN_NETWORK, 2.5
        self.tc, self.tn = torch.tensor(0.75), torch.tensor(0.5)
        self.made = {}

    def row(self, mode, **kw):
        r = self.siloop.si_row(self.cfg, self.tc, self.tn, False, blend=mode in ("blend", "renoise"), jump=mode == "renoise")
        nxt = self.cfg.preconditioner.eval_row(self.tc if mode == "renoise" else self.tn, False)
        return r, r.first.coef(self.kind, self.guidance, **kw), nxt.c_in

    def want(self, ops, mode):
        """(the eager chain's pair, the fp64 restatement's pair), computed once per mode."""
        if mode not in self.made:
            r, k, c_in = self.row(mode)
            a = chain(ops, self.x, self.f, self.fu, k, r, c_in, self.x_orig, self.mask, self.eps, mode)
            b = chain64(self.x, self.f, self.fu, k, r, c_in, self.x_orig, self.mask, self.eps, mode, True)
            self.made[mode] = (a, tuple(t.cpu() for t in b))
        return self.made[mode]


@pytest.fixture(scope="module")
def si_cases(dev):
    made = {}

    def get(shape):
        if shape not in made:
            made.clear()
            made[shape] = SICase(shape, dev)
        return made[shape]
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,wraps", [(SI_SHAPE, False), (SI_SHAPE_WRAP, True)], ids=["3x2x76x76x76", "4x2x76x76x76"])
def test_fused_step_equals_the_eager_chain_on_a_second_trip(ops, dev, si_cases, shape, wraps, mode):
    """edm, guidance 2.5 with fu, a soft mask: bit-equal to the eager op chain, and the fp64 restatement under the referee of
    tests/test_gpu_tiled_sampling.py, where the place in x_orig / mask / the per-position draws is a carried modulus."""
    assert_carry_is_live(shape, wraps)
    c = si_cases(shape)
    (want, want_in), (want64, want_in64) = c.want(ops, mode)
    r, k, c_in = c.row(mode)
    masked = mode != "no_mask"
    out, xin = torch.empty_like(c.x), torch.empty_like(c.x)
    for t in (c.x, c.f, c.fu, c.x_orig, c.mask, out, xin, *c.eps):
        assert t.data_ptr() % 16 == 0
    ops.si_inpaint_step(c.x, c.f, k, r.step(c_in), fu=c.fu, x_orig=c.x_orig if masked else None, mask=c.mask if masked else None,
                        blend=r.blend, renoise=r.jump, eps=c.eps, x_out=out, xin_out=xin)
    what = f"{shape} edm g=2.5 soft {mode}"
    referee(out.cpu(), want.cpu(), want64, what)
    referee(xin.cpu(), want_in.cpu(), want_in64, what + " xin")
    assert torch.equal(out, want) and torch.equal(xin, want_in), what
    k2 = c.row(mode, xin_copies=2)[1]
    B = shape[0]
    twice = torch.empty((2 * B,) + shape[1:], device=dev)
    ops.si_inpaint_step(c.x, c.f, k2, r.step(c_in), fu=c.fu, x_orig=c.x_orig if masked else None, mask=c.mask if masked else None,
                        blend=r.blend, renoise=r.jump, eps=c.eps, x_out=out, xin_out=twice)
    assert torch.equal(out, want) and torch.equal(twice[:B], want_in) and torch.equal(twice[B:], want_in), what


@pytest.mark.parametrize("shape,wraps", [(SI_SHAPE, False), (SI_SHAPE_WRAP, True)], ids=["3x2x76x76x76", "4x2x76x76x76"])
def test_philox_launch_equals_injected_launch_on_a_second_trip(ops, dev, si_cases, shape, wraps):
    """test_philox_launch_equals_injected_launch_at_the_documented_offsets, for blend and renoise: the per-position draws are read
    at the carried position as counters."""
    assert_carry_is_live(shape, wraps)
    c = si_cases(shape)
    B, n, one = shape[0], math.prod(shape[1:]), (1,) + shape[1:]
    state = torch.tensor([0x1234_5678_9ABC, 40], dtype=torch.int64, device=dev)
    base = 1000
    cB, c1 = ops.philox_counters(B * n), ops.philox_counters(n)
    eps = [ops.philox_normal(state, base + o, s) for o, s in ((0, shape), (cB, one), (cB + c1, shape), (2 * cB + c1, one))]
    for mode in ("blend", "renoise"):
        r, k, c_in = c.row(mode)
        a, a_in, b, b_in = (torch.empty_like(c.x) for _ in range(4))
        kw = dict(fu=c.fu, x_orig=c.x_orig, mask=c.mask, blend=r.blend, renoise=r.jump)
        ops.si_inpaint_step(c.x, c.f, k, r.step(c_in), eps=eps, x_out=a, xin_out=a_in, **kw)
        ops.si_inpaint_step(c.x, c.f, k, r.step(c_in), philox=(state, base), x_out=b, xin_out=b_in, **kw)
        assert torch.equal(a, b) and torch.equal(a_in, b_in), (shape, mode)
        want, want_in = chain(ops, c.x, c.f, c.fu, k, r, c_in, c.x_orig, c.mask, eps, mode)   # the draws' places, not only their counters
        assert torch.equal(b, want) and torch.equal(b_in, want_in), (shape, mode)
        assert ops.si_inpaint_counters(B, n, r.blend, r.jump) == (2 * (cB + c1) if r.jump else cB + c1)


SI_OPERANDS = ("x", "f", "fu", "x_orig", "mask", "eps0", "eps1", "eps2", "eps3", "x_out", "xin_out")


@pytest.mark.parametrize("odd", SI_OPERANDS)
def test_fused_step_misaligned_operand_takes_the_scalar_path(ops, dev, si_cases, odd):
    """Every operand in turn 4 bytes off, renoise (the mode that reads them all): the element-wise loop covers the whole state,
    its position carried with stride % nps, and gives the bits of the eager chain."""
    shape = SI_SHAPE
    B, nps, _, _, _ = si_geometry(shape)
    n = B * nps
    assert_scalar_loop_repeats(n)
    assert T % nps != 0 and trips(n, T) > 2                                # qstep != 0, and p passes a sample's end on the way
    c = si_cases(shape)
    (want, want_in), _ = c.want(ops, "renoise")
    r, k, c_in = c.row("renoise")
    t = dict(x=c.x, f=c.f, fu=c.fu, x_orig=c.x_orig, mask=c.mask, eps0=c.eps[0], eps1=c.eps[1], eps2=c.eps[2], eps3=c.eps[3])
    if odd in t:
        t[odd] = shifted(t[odd], dev)
    mk = lambda name: torch.empty(n + 1, device=dev)[1:].view(shape) if name == odd else torch.empty(shape, device=dev)   # noqa: E731
    out, xin = mk("x_out"), mk("xin_out")
    ops.si_inpaint_step(t["x"], t["f"], k, r.step(c_in), fu=t["fu"], x_orig=t["x_orig"], mask=t["mask"], blend=True, renoise=True,
                        eps=[t["eps0"], t["eps1"], t["eps2"], t["eps3"]], x_out=out, xin_out=xin)
    assert torch.equal(out, want) and torch.equal(xin, want_in), odd


# ---------------------------------------------------------------- 3. ds_window.hip: the row, plane and long-row loops
def box_launch_shape(planes, L):
    """box_launch_shape of ds_window.hip: (rows, quads, lanes per row, rows per block, grid.x, grid.y)."""
    rows, quads = L[0] * L[1], (L[2] + 3) // 4
    sh = 0
    while sh < 6 and (1 << sh) < quads:
        sh += 1
    rpb = THREADS >> sh
    gy = min(planes, WINDOW_PLANES)
    gx = min(-(-rows // rpb), max(WINDOW_BLOCKS // gy, 1))
    return rows, quads, 1 << sh, rpb, gx, gy


def check_box(ops, dev, planes, S, start, L, seed):
    """box_copy3d against `restated` and box_scatter3d against `setitem_ref` with the periodic tensor [planes, *S], the box L at
    `start` of it; the dense side holds the box at an offset with the inner start's alignment.  After the scatter, the gather
    returns the box."""
    g = torch.Generator().manual_seed(seed)
    at = (1, 2, start[2] % 4)                                              # the dense side's start: aligned when the periodic one is
    Dn = (L[0] + 2, L[1] + 3, (L[2] + at[2] + 7) // 4 * 4)
    per = torch.randn(planes, *S, generator=g)
    # the gather
    dst = torch.full((planes,) + Dn, SENTINEL, device=dev)
    want = torch.full((planes,) + Dn, SENTINEL)
    want[..., at[0]:at[0] + L[0], at[1]:at[1] + L[1], at[2]:at[2] + L[2]] = restated(per, start, L)
    assert ops.box_copy3d(per.to(dev), start, dst, at, L) is dst
    assert torch.equal(dst.cpu(), want)
    assert int((dst == SENTINEL).sum()) == dst.numel() - planes * L[0] * L[1] * L[2]
    # the scatter
    src = torch.randn((planes,) + Dn, generator=g)
    box = src[:, at[0]:at[0] + L[0], at[1]:at[1] + L[1], at[2]:at[2] + L[2]]
    want = setitem_ref(per, box, start)
    got = per.clone().to(dev)
    assert ops.box_scatter3d(src.to(dev), at, got, start, L) is got
    assert torch.equal(got.cpu(), want)
    back = ops.box_copy3d(got, start, torch.empty(planes, *L, device=dev), (0, 0, 0), L)
    assert torch.equal(back.cpu(), box)


@pytest.mark.parametrize("start", [(30, 20, 101), (30, 20, 100)], ids=["odd_start", "aligned_start"])
def test_box_rows_past_the_cap_and_rows_longer_than_64_quads(ops, dev, start):
    """8 planes, box (33, 32, 260) of a periodic (40, 37, 300): 1056 rows at 4 per block on a grid capped at 256 blocks of rows, so
    rows 1024 and above are a second trip, and 65 quads on 64 lanes, so the quad loop runs twice.  The start wraps all three axes;
    with the inner start a multiple of 4 the 16-byte path is the one that loops."""
    planes, S, L = 8, (40, 37, 300), (33, 32, 260)
    rows, quads, lpr, rpb, gx, gy = box_launch_shape(planes, L)
    assert (rows, quads, lpr, rpb, gx, gy) == (1056, 65, 64, 4, WINDOW_BLOCKS // 8, 8)
    assert rows > gx * rpb and quads > lpr and gy == planes
    assert all(s + n > m for s, n, m in zip(start, L, S))                  # a wrap on every axis
    if start[2] % 4 == 0:
        assert S[2] % 4 == 0 and L[2] % 4 == 0                             # every quad whole and aligned on both sides of the wrap
    check_box(ops, dev, planes, S, start, L, 31)


@pytest.mark.parametrize("S,L", [((6, 7, 9), (3, 4, 5)), ((24, 23, 9), (20, 20, 5))], ids=["3x4x5", "20x20x5"])
def test_box_planes_past_1024(ops, dev, S, L):
    """1030 planes on a grid.y of 1024: planes 1024 .. 1029 are a second trip of the plane loop.  The larger box also caps the row
    blocks at 2048 / 1024 = 2, so its rows 256 and above are a second trip inside every plane."""
    planes, start = 1030, (S[0] - 2, S[1] - 1, S[2] - 3)
    rows, quads, lpr, rpb, gx, gy = box_launch_shape(planes, L)
    assert gy == WINDOW_PLANES < planes and gx <= WINDOW_BLOCKS // WINDOW_PLANES
    if L == (20, 20, 5):
        assert gx == 2 and rows > gx * rpb
    check_box(ops, dev, planes, S, start, L, 32)


# ---------------------------------------------------------------- 4. ds_resample.hip, ds_gnorm.hip: one unit per thread
@pytest.mark.parametrize("f,out_shape", [(2, (1, 1, 81, 81, 81)), (4, (1, 1, 728, 728))], ids=["3d_f2", "2d_f4"])
def test_avgpool_vs_fp64_past_the_cap(ops, dev, f, out_shape):
    """The rule of test_pooling_vs_fp64 (tests/test_gpu_adm_resample.py); one output per thread, more outputs than threads.  The
    field at factor 4 takes the 16-byte window loads."""
    units = math.prod(out_shape)
    cap = RESAMPLE_BLOCKS if len(out_shape) == 5 else POOLF_BLOCKS         # volumes: ds_avgpool3d_f; fields: ds_gnorm1_apply_poolf, kind 2
    assert capped(units, cap) == T and trips(units, T) >= 2
    g = torch.Generator().manual_seed(10 + f)
    x = torch.randn(out_shape[:2] + tuple(f * v for v in out_shape[2:]), generator=g) * 2 + 0.3
    assert f % 4 or x.shape[-1] % 4 == 0
    pool = F.avg_pool2d if x.dim() == 4 else F.avg_pool3d
    want = pool(x.double(), f)
    xd = aligned(x, dev)
    ref = pool(xd, f).cpu()
    got = ops.avgpool_f(xd, f).cpu()
    assert got.shape == want.shape == out_shape
    ref_err, err = rel_l2(ref, want), rel_l2(got, want)
    print(f"avgpool_f {tuple(x.shape)} f={f}: {err:.2e} (torch {ref_err:.2e})")
    assert err <= max(2 * ref_err, 1e-12), (f, err, ref_err)


def _same(a, b):
    """The comparison of tests/test_gpu_punetg_resample.py: NaN where the other has NaN, the same bits everywhere else."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num().view(torch.int32), b.nan_to_num().view(torch.int32))


@pytest.mark.parametrize("f,side,vec", [(2, 1456, 4), (3, 727, 1)], ids=["f2_four_per_thread", "f3_one_per_thread"])
def test_maxpool_is_torch_bit_for_bit_past_the_cap(ops, dev, f, side, vec):
    """Bit-equal to F.max_pool2d, with a NaN window and an all -inf window among the outputs only a second trip writes."""
    assert (side % 4 == 0) == (vec == 4)
    units = side * side // vec
    assert capped(units, RESAMPLE_BLOCKS) == T and trips(units, T) >= 2
    g = torch.Generator().manual_seed(40 + f)
    x = torch.randn(1, 1, f * side, f * side, generator=g) * 3
    x[..., ::5] = 0.0
    x[..., 1::7] = -0.0
    for j, (o, val) in enumerate(((vec * T + 5, float("nan")), (vec * T + 1000, float("-inf")))):
        assert vec * T <= o < side * side                                  # a flat output index of a unit past the first T
        oy, ox = divmod(o, side)
        if j == 0:
            x[0, 0, oy * f + f - 1, ox * f] = val                          # one NaN, in the window's last row
        else:
            x[0, 0, oy * f:oy * f + f, ox * f:ox * f + f] = val
    want = F.max_pool2d(x, f)
    got = ops.maxpool_f(aligned(x, dev), f).cpu()
    assert _same(got, want)
    assert bool(got.flatten()[vec * T + 5].isnan()) and float(got.flatten()[vec * T + 1000]) == float("-inf")
    assert int(got.isnan().sum()) == 1


@pytest.mark.parametrize("f,out_sides", [(1, (33, 32, 64)), (2, (17, 32, 31))], ids=["f1_16_byte_loads", "f2_scalar_stores"])
def test_cornerpool_is_torch_bit_for_bit_past_the_cap(ops, dev, f, out_sides):
    """The bit-exact rule of test_cornerpool_is_torch_bit_for_bit (tests/test_gpu_punetg_field3d.py) at B = 16: a sample gets
    2048 / 16 = 128 workgroups, fewer threads than it has units.  out_amax equals the result's per-sample abs().amax()."""
    B, C = 16, 2
    vec = 4 if out_sides[2] % 4 == 0 else 1
    per = C * math.prod(out_sides) // vec
    assert (f, vec) in ((1, 4), (2, 1))
    assert per > THREADS * (RESAMPLE_BLOCKS // B) and trips(per, THREADS * (RESAMPLE_BLOCKS // B)) >= 2
    g = torch.Generator().manual_seed(10 + f)
    x = (torch.randn((B, C) + tuple(v * f for v in out_sides), generator=g) * 3).to(dev)
    x.view(-1)[::7] = -0.0
    te = torch.randn(B, C, generator=g).to(dev)
    want = x[(Ellipsis,) + (slice(None, None, f),) * 3] + te.view(B, C, 1, 1, 1)
    amax = torch.zeros(B, dtype=torch.int32, device=dev)
    got = ops.cornerpool_f(x, f, te=te, out_amax=amax)
    assert bits(got, want)
    assert torch.equal(amax.view(torch.float32), got.reshape(B, -1).abs().amax(1))
    assert bits(ops.cornerpool_f(x, f), x[(Ellipsis,) + (slice(None, None, f),) * 3])    # the pure copy keeps -0.0


@pytest.mark.parametrize("f,side", [(2, 368), (4, 736)], ids=["f2", "f4"])
def test_norm_silu_pool_vs_fp64_past_the_cap(ops, dev, f, side):
    """The rule and bound of test_norm_silu_pool_vs_fp64 (tests/test_gpu_adm_resample.py): kinds 0 and 1, with and without FiLM."""
    B, C = 2, 8
    units = B * C * (side // f) ** 2
    assert capped(units, POOLF_BLOCKS) == T and trips(units, T) >= 2
    g = torch.Generator().manual_seed(20 + f)
    x = torch.randn(B, C, side, side, generator=g) * 3 + 0.7
    w, b, film = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, 2 * C, generator=g)
    xd = aligned(x, dev)
    for kind in (0, 1):
        st = ops.gnorm1_stats(xd, kind)
        n = (F.group_norm(x.double(), 1, w.double(), b.double(), 1e-5) if kind == 0
             else adm_ref.group1_rms_norm(x.double(), w.double(), b.double()))
        for fl in (None, film):
            v = n if fl is None else n * fl[:, :C, None, None].double() + fl[:, C:, None, None].double()
            want = F.avg_pool2d(F.silu(v), f)
            got = ops.gnorm1_apply_poolf(xd, st, w.to(dev), b.to(dev), kind, f, film=None if fl is None else fl.to(dev)).cpu()
            assert got.shape == want.shape
            err = rel_l2(got, want)
            print(f"gnorm1_apply_poolf {side}x{side} f={f} kind={kind} film={fl is not None}: {err:.2e}")
            assert err < 5e-7, (f, kind, fl is None)


# ---------------------------------------------------------------- 5. ds_groupnorm.hip, ds_small.hip
@pytest.mark.parametrize("shape,G,vec", [((1, 32, 258, 256), 8, 4), ((1, 8, 129, 129), 4, 1)], ids=["16_byte", "scalar"])
def test_groupnorm_apply_against_fp64_past_the_cap(ops, dev, shape, G, vec):
    """The rule of test_groupnorm_kernels_against_fp64 (tests/test_gpu_ldm_decoder.py): a channel row gets 64 workgroups, fewer
    threads than it has units of `vec` positions.  The amax slot equals the output's own maximum, bit for bit."""
    B, C = shape[:2]
    N = shape[2] * shape[3]
    assert (N % 4 == 0) == (vec == 4)
    assert N // vec > GN_CHUNKS * THREADS and trips(N // vec, GN_CHUNKS * THREADS) >= 2
    torch.manual_seed(100 + G)
    x = torch.randn(*shape) * 3 + 0.7
    w, b = torch.randn(C), torch.randn(C)
    xd = aligned(x, dev)
    st = ops.groupnorm_stats(xd, G, eps=1e-6)
    for act in (0, 1):
        want = F.group_norm(x.double(), G, w.double(), b.double(), 1e-6)
        want = F.silu(want) if act else want
        am = ops.amax_new(B, dev)
        got = ops.groupnorm_apply(xd, st, w.to(dev), b.to(dev), G, act=bool(act), out_amax=am)
        assert bool(torch.isfinite(got).all())
        err = rel_l2(got.cpu(), want)
        print(f"groupnorm {shape} G={G} act={act}: rel-L2 {err:.2e}")
        assert err < 5e-7
        assert torch.equal(am.view(torch.float32), got.reshape(B, -1).abs().amax(1))
        assert torch.equal(ops.groupnorm_apply(xd, st, w.to(dev), b.to(dev), G, act=bool(act)), got)


def test_fourier_channels_past_the_cap(ops, dev):
    """check_kernel of tests/test_gpu_dit.py.  W is scaled so that the arguments 2 pi x.W stay within a few radians: beyond that
    the fp32 rounding of the argument itself dominates both fp32 results and the comparison says nothing about the kernel."""
    shape, D = (1, 2, 252, 253), 33
    units = shape[0] * D * shape[2] * shape[3]
    assert units == 2103948 and capped(units, FOURIER_BLOCKS, FOURIER_THREADS) == FOURIER_BLOCKS * FOURIER_THREADS < units
    g = torch.Generator().manual_seed(51)
    x, W = torch.randn(shape, generator=g), torch.randn(shape[1], D, generator=g) * 0.04
    assert float((2 * math.pi * torch.einsum('bc...,cd->bd...', x.double(), W.double())).abs().max()) < 6.0
    got = ops.fourier_channels(x.to(dev), W.to(dev))
    assert got.shape == (1, 2 * D) + shape[2:]
    check_kernel("fourier_channels 252x253 D=33", got, punetg_ref.fourier_input({"convin.W": W}, x),
                 punetg_ref.fourier_input({"convin.W": W.double()}, x.double()))


def test_linear_rows_past_grid_y(ops, dev):
    """check_kernel of tests/test_gpu_dit.py: 70 rows on a grid.y of 64, so rows 64 .. 69 are a second trip of the row loop."""
    M_, K_, N_ = 70, 65, 5
    assert M_ > LINEAR_ROWS and trips(M_, LINEAR_ROWS) == 2
    g = torch.Generator().manual_seed(52)
    x, w, b = torch.randn(M_, K_, generator=g), torch.randn(N_, K_, generator=g), torch.randn(N_, generator=g)
    for act, fn in ((0, lambda t: t), (1, F.silu), (2, F.relu)):
        got = ops.linear(x.to(dev), w.to(dev), b.to(dev), act=act)
        check_kernel(f"linear 70x65x5 act={act}", got, fn(F.linear(x, w, b)), fn(F.linear(x.double(), w.double(), b.double())))
    got = ops.linear(x.to(dev), w.to(dev))
    check_kernel("linear 70x65x5 no bias", got, F.linear(x, w), F.linear(x.double(), w.double()))


# ---------------------------------------------------------------- 6. wrappers that had no direct test
FLAT_SIZES = [1, 5, 4099, N_B]         # one element, not a multiple of 4, several blocks, and past the cap with a tail


def _placed(t, dev, odd):
    return shifted(t, dev) if odd else aligned(t, dev)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("size", FLAT_SIZES)
@pytest.mark.parametrize("n", [2, 5])
def test_lerp_stack_bit_exact(ops, dev, n, size, odd):
    """k_lerp_stack's header: out[i] = x1 + ((x2 - x1) * i) / (n - 1), in torch fp32."""
    g = torch.Generator().manual_seed(60 + n + size)
    x1, x2 = torch.randn(size, generator=g) * 3, torch.randn(size, generator=g) * 3
    want = torch.stack([x1 + ((x2 - x1) * i) / (n - 1) for i in range(n)])
    got = ops.lerp_stack(_placed(x1, dev, odd), _placed(x2, dev, odd), n)
    assert got.shape == (n, size) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("size", FLAT_SIZES)
def test_score_bit_exact(ops, dev, size, odd):
    """ds_step.hip's header: D = c_out*F + c_skip*x, score = (D - x)/sigma^2, F = (1 - g)*Fu + g*F under guidance."""
    g = torch.Generator().manual_seed(70 + size)
    x, f, fu = torch.randn(size, generator=g) * 80, torch.randn(size, generator=g), torch.randn(size, generator=g)
    cs, co, _, _ = K.edm_precond(torch.tensor(57.586))
    r = dict(c_out=float(co), c_skip=float(cs), sigma_sq=float(torch.tensor(57.586) ** 2))
    xd, fd, ud = (_placed(t, dev, odd) for t in (x, f, fu))
    for g_, u, uu in ((1.0, None, None), (2.5, fu, ud)):
        Fv = f if u is None else (1 - g_) * u + g_ * f
        want = ((r["c_out"] * Fv + r["c_skip"] * x) - x) / r["sigma_sq"]
        got = ops.score(xd, fd, _coef(guidance=g_, one_minus_guidance=1 - g_, **r), fu=uu)
        assert torch.equal(got.cpu(), want), (size, g_)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("per", [1, 5, 4099, N_B // 3])
def test_denoiser_bit_exact(ops, dev, per, odd):
    """k_denoiser: out = c_out[b]*F + c_skip[b]*x with F = (1 - g)*Fu + g*F, per-sample c_out / c_skip at B = 3."""
    B = 3
    if per == N_B // 3:
        assert capped((B * per + 3) // 4) == T and trips(B * per, T) >= 2
    g = torch.Generator().manual_seed(80 + per)
    x, f, fu = (torch.randn(B, per, generator=g) * s for s in (80.0, 1.0, 1.0))
    c_out, c_skip = torch.rand(B, generator=g) + 0.1, torch.rand(B, generator=g)
    xd, fd, ud = (_placed(t, dev, odd) for t in (x, f, fu))
    for g_, u, uu in ((1.0, None, None), (2.5, fu, ud)):
        Fv = f if u is None else (1 - g_) * u + g_ * f
        want = c_out[:, None] * Fv + c_skip[:, None] * x
        got = ops.denoiser(xd, fd, c_out.to(dev), c_skip.to(dev), fu=uu, guidance=g_)
        assert torch.equal(got.cpu(), want), (per, g_)


@pytest.mark.parametrize("n", [1, 257])
def test_amax_merge_is_the_maximum_of_the_bit_patterns(ops, dev, n):
    g = torch.Generator().manual_seed(90 + n)
    out, a, b = (torch.rand(n, generator=g).mul(1e3).view(torch.int32).clone() for _ in range(3))
    a[0], b[-1] = 0, int(torch.tensor(3.0e38).view(torch.int32))         # an empty slot and the largest finite magnitude
    for second in (None, b):
        od = out.clone().to(dev)
        want = torch.maximum(out, a) if second is None else torch.maximum(torch.maximum(out, a), second)
        assert ops.amax_merge(od, a.to(dev), None if second is None else second.to(dev)) is od      # in place
        assert torch.equal(od.cpu(), want)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("size", FLAT_SIZES)
def test_tanh_against_fp64(ops, dev, size, odd):
    g = torch.Generator().manual_seed(95 + size)
    x = torch.randn(size, generator=g) * 3
    got = ops.tanh(_placed(x, dev, odd))
    check_kernel(f"tanh n={size}", got, torch.tanh(x), torch.tanh(x.double()))


@pytest.mark.parametrize("L", [35, 300])
@pytest.mark.parametrize("E", [32, 48])
@pytest.mark.parametrize("c0_is_E", [False, True], ids=["c0=0", "c0=E"])
def test_token_l2_normalize_against_fp64(ops, dev, c0_is_E, E, L):
    """x / (norm + eps) * gain over channels [c0, c0 + E) of every token, in place; the other channels untouched; an all-zero
    token stays finite (eps)."""
    B, c0, eps, gain = 2, (E if c0_is_E else 0), 1e-8, 4.0
    g = torch.Generator().manual_seed(97 + E + L)
    x = torch.randn(B, 3 * E, L, generator=g) * 2
    x[1, c0:c0 + E, L // 2] = 0.0
    xd = x.clone().to(dev)
    assert ops.token_l2_normalize(xd, c0, E, eps=eps, gain=gain) is xd
    got = xd.cpu()
    keep = torch.ones(3 * E, dtype=torch.bool)
    keep[c0:c0 + E] = False
    assert torch.equal(got[:, keep], x[:, keep])

    def ref(t):
        part = t[:, c0:c0 + E]
        return part / (torch.linalg.vector_norm(part, dim=1, keepdim=True) + eps) * gain

    assert bool(torch.isfinite(got).all()) and bool((got[1, c0:c0 + E, L // 2] == 0).all())
    check_kernel(f"token_l2_normalize E={E} L={L} c0={c0}", got[:, c0:c0 + E], ref(x), ref(x.double()))
