"""The transformer-side norm kernels -- k_token_ln (ops.token_layernorm), k_channel_rms (ops.channel_rmsnorm), k_token_l2norm
(ops.token_l2_normalize) -- under the analytic fp64 error model of tests/token_norm_bounds.py (checked on the CPU by
tests/test_token_norm_bounds.py), on the token-wise data families: means that dominate the deviation, variances below eps,
tiny and huge magnitudes, an outlier in the channel the LayerNorm pivots on (P0, P0neg) and elsewhere (Pmid), zero and constant
tokens (Z).  Every case prints its error / bound ratio and its max-abs error (pytest -s), and every register-count
instantiation of launch_ln and launch_rms is reached on both lane widths.  Each output is a view into a sentinel-filled buffer
with guard rows on both sides, inside one allocation: a stray write would land in memory the test owns, and is seen.

Register counts, NR = the first of {2, 4, 8, 16, 32 (, 64, 128: scalar lanes)} >= ceil(E / TY):
  16-byte lanes (TY = 32):  E = 64 -> 2,  100 -> 4,  256 -> 8,  500 -> 16,  1024 -> 32
  scalar lanes  (TY = 8):   E = 9 -> 2,  32 -> 4,  48, 64 -> 8,  128 -> 16,  200 -> 32,  512 -> 64,  520, 1000, 1024 -> 128
"""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import dit_ref  # noqa: E402
from tests import token_norm_bounds as tb  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

B = 2
LN_EPS = 1e-5
ULP = 2.0 ** -23
SENTINEL = -1.2345e30
MODES = ("shared", "per_sample", "row", "none")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


def mod_table(mode, E, chunks, gen):
    """(table [rows, chunks * E], row) in the forms the kernels take, and the [B, chunks * E] rows they mean (None: no table)."""
    if mode == "none":
        return None, None, None
    if mode == "shared":                                  # one row for the batch: stride 0
        tab = torch.randn(1, chunks * E, generator=gen)
        return tab, None, tab.expand(B, -1)
    if mode == "per_sample":
        tab = torch.randn(B, chunks * E, generator=gen)
        return tab, None, tab
    tab = torch.randn(5, chunks * E, generator=gen)       # the sampler's table of all evaluations: a non-zero row
    return tab, 3, tab[3:4].expand(B, -1)


class Guarded:
    """An output of `shape` as a view into a larger buffer filled with a sentinel: `guard` floats (whole rows of the output, a
    multiple of four so that the view keeps the buffer's 16-byte alignment) before and after it."""

    def __init__(self, shape, row, dev):
        self.n = int(torch.Size(shape).numel())
        self.guard = 4 * row
        self.buf = torch.full((self.n + 2 * self.guard,), SENTINEL, device=dev)
        self.out = self.buf[self.guard:self.guard + self.n].view(shape)
        assert self.out.is_contiguous() and self.buf.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def intact(self):
        s = torch.full((self.guard,), SENTINEL)
        return torch.equal(self.buf[:self.guard].cpu(), s) and torch.equal(self.buf[self.guard + self.n:].cpu(), s)


def amax_checks(call, out, dev):
    """out_amax holds the bits of the output's per-sample maximum, and is merged into the slot, not overwritten."""
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    again = call(slots)
    assert torch.equal(again, out)                                         # the same bits from run to run
    assert torch.equal(slots.view(torch.float32), out.abs().amax(dim=tuple(range(1, out.dim()))))
    big = torch.full((B,), 3.0e38, device=dev).view(torch.int32).clone()
    call(big)
    assert torch.equal(big.view(torch.float32), torch.full((B,), 3.0e38, device=dev))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- token LayerNorm
# L = 36, aligned: 16-byte lanes, the second workgroup has four live tokens; L = 37: scalar lanes, five live tokens
LN_SHAPES = [(36, E) for E in (64, 100, 256, 500, 1024)] + [(37, E) for E in (9, 32, 64, 128, 200, 512, 1000)]
LN_CASES = [(fam, L, E, MODES[(i + j) % 4]) for i, fam in enumerate(tb.TOKEN_FAMILIES) for j, (L, E) in enumerate(LN_SHAPES)]


@pytest.mark.parametrize("fam,L,E,mode", LN_CASES)
def test_token_layernorm(ops, dev, fam, L, E, mode):
    gen = torch.Generator().manual_seed(100 * E + L)
    x = tb.token_family(fam, (B, E, L), seed=E + L)
    w, b = 1 + 0.25 * torch.randn(E, generator=gen), 0.25 * torch.randn(E, generator=gen)
    tab, row, rows = mod_table(mode, E, 6, gen)
    sh, sc = (None, None) if rows is None else (rows[:, 3 * E:4 * E], rows[:, 4 * E:5 * E])       # the MLP pair of chunks
    xd, wd, bd, tabd = x.to(dev), w.to(dev), b.to(dev), None if tab is None else tab.to(dev)
    assert xd.data_ptr() % 16 == 0
    g = Guarded((B, E, L), L, dev)

    def call(slots):
        return ops.token_layernorm(xd, wd, bd, tabd, 3, 4, row, eps=LN_EPS, out=g.out, out_amax=slots)

    out = call(None).clone()
    assert g.intact(), "a write outside the live region"
    got = out.cpu()
    assert torch.isfinite(got).all()
    ratio, err = tb.ln_ratio(got, x, w, b, sc, sh, LN_EPS)
    worst = float(ratio.max())
    print(f"token_layernorm {fam:6s} E={E:4d} L={L} {mode:10s}: error / bound = {worst:.3f}, max-abs error {err:.2e}")
    amax_checks(call, out, dev)
    assert g.intact()
    if fam == "Z":
        one_sc = 1.0 + sc[1] if sc is not None else torch.ones(E)          # fp32, one rounding per operation, as the kernel
        const = b * one_sc + (sh[1] if sh is not None else torch.zeros(E))
        assert same_bits(got[1, :, 1], const), "the constant token is not b (1 + sc) + sh"
        assert float(ratio[1, :, 0].max()) <= 1.0                          # the zero token (finite: checked above)
    assert worst <= 1.0, (fam, E, L, mode, worst)


# ------------------------------------------------------------------------------------------------------- channel RMSNorm
RMS_FAMILIES = ("A", "E40", "F", "P0", "Pmid", "Z")
# (H, W, pool, E): 4x8 = 32 pixels on 16-byte lanes; 3x5 on scalar lanes; pooled (scalar lanes), the last with an odd side
RMS_SHAPES = [(4, 8, 1, E) for E in (64, 100, 256, 500, 1024)] + [(3, 5, 1, E) for E in (9, 32, 64, 128, 200, 512, 520, 1024)] \
    + [(H, W, p, E) for (H, W, p) in ((6, 10, 2), (8, 12, 4), (9, 7, 2)) for E in (48, 200)]
RMS_CASES = [(fam, H, W, p, E, MODES[(i + j) % 4]) for i, fam in enumerate(RMS_FAMILIES) for j, (H, W, p, E) in enumerate(RMS_SHAPES)]


@pytest.mark.parametrize("fam,H,W,pool,E,mode", RMS_CASES)
def test_channel_rmsnorm(ops, dev, fam, H, W, pool, E, mode):
    gen = torch.Generator().manual_seed(100 * E + H * W + pool)
    x = tb.token_family(fam, (B, E, H * W), seed=E + H * W).view(B, E, H, W).clone()      # Z: pixel 0 of sample 1 is zero
    w = 1 + 0.25 * torch.randn(E, generator=gen)
    tab, row, rows = mod_table(mode, E, 1, gen)
    xd, wd, tabd = x.to(dev), w.to(dev), None if tab is None else tab.to(dev)
    OH, OW = H // pool, W // pool
    g = Guarded((B, E, OH, OW), OH * OW, dev)
    assert xd.data_ptr() % 16 == 0                                         # with g.out's alignment: 4x8 takes the 16-byte lanes

    def call(slots):
        return ops.channel_rmsnorm(xd, wd, tabd, row, pool=pool, out=g.out, out_amax=slots)

    out = call(None).clone()
    assert out.shape == (B, E, OH, OW)                                     # the floor of the pooled size
    assert g.intact(), "a write outside the live region"
    got = out.cpu()
    assert torch.isfinite(got).all()
    ratio, err = tb.rms_ratio(got, x, w, rows, pool, ops.RMS_EPS)
    worst = float(ratio.max())
    print(f"channel_rmsnorm {fam:5s} E={E:4d} {H}x{W} pool={pool} {mode:10s}: error / bound = {worst:.3f}, max-abs error {err:.2e}")
    amax_checks(call, out, dev)
    assert g.intact()
    if fam == "Z" and pool == 1:                                           # the zero pixel is the embedding row, bit for bit
        assert same_bits(got[1, :, 0, 0], rows[1]) if rows is not None else not got[1, :, 0, 0].any()
    assert worst <= 1.0, (fam, E, H, W, pool, mode, worst)


# ------------------------------------------------------------------------------------------------------ token L2 normalise
def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def check_kernel(what, got, t32, ref64):
    """The bound of the existing op tests: 4 x torch's own fp32 error, in rel-L2 and in max-abs."""
    e_rel, t_rel = rel_l2(got, ref64), rel_l2(t32, ref64)
    e_abs, t_abs = max_abs(got, ref64), max_abs(t32, ref64)
    print(f"{what}: rel-L2 {e_rel:.2e} (torch fp32 {t_rel:.2e}); max-abs {e_abs:.2e} (torch fp32 {t_abs:.2e})")
    assert e_rel <= max(4 * t_rel, 1e-7)
    assert e_abs <= max(4 * t_abs, ULP * float(ref64.abs().max()))


@pytest.mark.parametrize("c0_is_C", [False, True], ids=["c0=0", "c0=C"])
@pytest.mark.parametrize("L", [36, 37])
@pytest.mark.parametrize("C", [32, 200, 512])
@pytest.mark.parametrize("fam", ["A", "E40", "F", "P0"])
def test_token_l2_normalize(ops, dev, fam, C, L, c0_is_C):
    c0, gain = (C if c0_is_C else 0), 4.0
    x = tb.token_family("A", (B, 3 * C, L), seed=C + L)
    x[:, c0:c0 + C] = tb.token_family(fam, (B, C, L), seed=C + L + 1)      # E40: eps-dominated at eps = 1e-8
    x[1, c0:c0 + C, L // 2] = 0.0
    xd = x.clone().to(dev)
    assert ops.token_l2_normalize(xd, c0, C, eps=tb.L2_EPS, gain=gain) is xd
    got = xd.cpu()
    keep = torch.ones(3 * C, dtype=torch.bool)
    keep[c0:c0 + C] = False
    assert same_bits(got[:, keep], x[:, keep]), "a channel outside the slice changed"
    part, xs = got[:, c0:c0 + C], x[:, c0:c0 + C]
    assert torch.isfinite(part).all() and not part[1, :, L // 2].any()    # an all-zero token stays zero
    ratio, err = tb.l2_ratio(part, xs, tb.L2_EPS, gain)
    worst = float(ratio.max())
    print(f"token_l2_normalize {fam:4s} C={C:3d} L={L} c0={c0:3d}: error / bound = {worst:.3f}, max-abs error {err:.2e}")

    def ref(t):
        return t / (torch.linalg.vector_norm(t, dim=1, keepdim=True) + tb.L2_EPS) * gain

    check_kernel("  against torch fp32", part, ref(xs), ref(xs.double()))
    assert worst <= 1.0, (fam, C, L, c0, worst)


# ------------------------------------------------------------------------------------------------------------ the network
def check_network(what, got, f32, f64):
    """The network bound of tests/test_gpu_dit.py; prints the three distances."""
    got = got.cpu()
    ref_rel, ref_abs = rel_l2(f32, f64), max_abs(f32, f64)
    e_rel, e_abs = rel_l2(got, f64), max_abs(got, f64)
    print(f"{what}: HIP vs fp32 {rel_l2(got, f32):.2e}; HIP vs fp64 {e_rel:.2e}; reference fp32 vs fp64 {ref_rel:.2e}; "
          f"max-abs HIP {e_abs:.2e}, reference fp32 {ref_abs:.2e}")
    assert torch.isfinite(got).all()
    assert e_rel <= max(1e-5, 4 * ref_rel)
    assert e_abs <= max(1e-4 * float(f64.abs().max()), 4 * ref_abs)


def test_dit_with_a_massive_first_channel(M, dev):
    """The smallest golden DiT (one block, 64 channels) with row 0 of the patch embedding scaled by 1e4: channel 0 of every token,
    the LayerNorm's pivot, is about 1e4 times the others.  Whether the op-level finding reaches an output; the network bound is
    the existing one."""
    v, sd, kw = dit_ref.load_golden("c")
    sd = {n: w.clone() for n, w in sd.items()}
    sd["embed.weight"][0] *= 1e4
    sd["embed.bias"][0] *= 1e4
    nheads, patch = kw.get("nheads", 4), kw.get("patch_size", 4)
    with torch.inference_mode():
        f32 = dit_ref.dit_forward(sd, v["x"], v["t"], nheads, patch)
        f64 = dit_ref.dit_forward({n: w.double() for n, w in sd.items()}, v["x"], v["t"], nheads, patch)
    net = M.DiffusionTransformer(**kw)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = net(v["x"].to(dev), v["t"].to(dev))
    check_network("dit_c, embed row 0 x 1e4", out, f32, f64)
