"""DiffusionTransformer on a real MI355X: the token kernels (ds_tokens.hip) against fp64 torch compositions, the network against
the reference's goldens (tests/golden/dit_*.npz) and against tests/dit_ref.py where no golden exists, and the captured sampler.

Bounds, all against fp64 (the network's Fourier time embedding, scale 30, amplifies last-bit differences, so two fp32 forms of
it are not comparable with each other below a few 1e-6):
  kernels   rel-L2 and max-abs error at most 4 x the error torch's fp32 CPU result has on the same inputs, computed
            here, with floors of 1e-7 rel-L2 and one fp32 ulp of the largest value for the cases where torch happens to be exact;
            the gated residual is bit-exact against torch-CPU fp32;
  network   rel-L2 <= max(1e-5, 4 x the reference's own fp32-vs-fp64 distance), max-abs <= max(1e-4 x max |out|, 4 x the
            reference fp32 output's own max-abs error)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import dit_ref  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def check_kernel(what, got, t32, ref64):
    """4 x torch's own fp32 error, in rel-L2 and in max-abs."""
    got = got.cpu()
    e_rel, t_rel = rel_l2(got, ref64), rel_l2(t32, ref64)
    e_abs, t_abs = max_abs(got, ref64), max_abs(t32, ref64)
    print(f"{what}: rel-L2 {e_rel:.2e} (torch fp32 {t_rel:.2e}); max-abs {e_abs:.2e} (torch fp32 {t_abs:.2e})")
    assert e_rel <= max(4 * t_rel, 1e-7)
    assert e_abs <= max(4 * t_abs, ULP * float(ref64.abs().max()))


def check_network(what, got, f32, f64, scale=None):
    """The stated network bound; prints the three distances."""
    got = got.cpu()
    ref_rel, ref_abs = rel_l2(f32, f64), max_abs(f32, f64)
    e_rel, e_abs = rel_l2(got, f64), max_abs(got, f64)
    print(f"{what}: HIP vs fp32 {rel_l2(got, f32):.2e}; HIP vs fp64 {e_rel:.2e}; reference fp32 vs fp64 {ref_rel:.2e}; "
          f"max-abs HIP {e_abs:.2e}, reference fp32 {ref_abs:.2e}")
    assert torch.isfinite(got).all()
    assert e_rel <= max(1e-5, 4 * ref_rel)
    assert e_abs <= max(1e-4 * (float(f64.abs().max()) if scale is None else scale), 4 * ref_abs)


def mod_table(mode, B, E, gen):
    """(table, row) in the three forms the kernels take, and the [B, 6E] rows they mean."""
    if mode == "shared":                                  # one row for the batch: stride 0
        tab, row = torch.randn(1, 6 * E, generator=gen), None
        return tab, row, tab.expand(B, -1)
    if mode == "per_sample":                              # stride 6E
        tab = torch.randn(B, 6 * E, generator=gen)
        return tab, None, tab
    tab = torch.randn(5, 6 * E, generator=gen)            # the sampler's table of all evaluations: a non-zero row
    return tab, 3, tab[3:4].expand(B, -1)


LN_CASES = [(1, 48, 60, "shared", 0.0), (3, 64, 64, "per_sample", 0.0), (3, 128, 1000, "row", 0.0), (1, 384, 1024, "per_sample", 0.0),
            (3, 48, 1024, "row", 0.0), (3, 384, 60, "shared", 0.0), (1, 64, 1000, "shared", 0.0), (3, 128, 64, "per_sample", 0.0),
            (3, 64, 1000, "per_sample", 1e4),             # a large common offset: E[x^2] - mean^2 would cancel
            (2, 64, 63, "row", 0.0), (1, 128, 1001, "per_sample", 0.0), (2, 1024, 36, "shared", 0.0)]   # L % 4 != 0; the widest E


@pytest.mark.parametrize("B,E,L,mode,offset", LN_CASES)
def test_token_layernorm(ops, dev, B, E, L, mode, offset):
    gen = torch.Generator().manual_seed(1000 + B * 7 + E + L)
    x = offset + torch.randn(B, E, L, generator=gen) * (1.0 + torch.rand(B, 1, L, generator=gen))
    w, b = 1 + 0.25 * torch.randn(E, generator=gen), 0.25 * torch.randn(E, generator=gen)
    tab, row, rows = mod_table(mode, B, E, gen)
    shift, scale = rows[:, 3 * E:4 * E], rows[:, 4 * E:5 * E]          # the MLP pair of chunks

    def ref(dt):
        n = F.layer_norm(x.to(dt).transpose(1, 2), (E,), w.to(dt), b.to(dt), 1e-5)
        return (n * (1 + scale.to(dt)[:, None, :]) + shift.to(dt)[:, None, :]).transpose(1, 2)

    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    out = ops.token_layernorm(x.to(dev), w.to(dev), b.to(dev), tab.to(dev), 3, 4, row, out_amax=slots)
    check_kernel(f"layernorm B={B} E={E} L={L} {mode} offset={offset:g}", out, ref(torch.float32), ref(torch.float64))
    assert torch.equal(slots.view(torch.float32), out.abs().amax(dim=(1, 2)))
    # merged into, not overwritten; and the plain LayerNorm without a table
    big = torch.full((B,), 3.0e38, device=dev).view(torch.int32).clone()
    ops.token_layernorm(x.to(dev), w.to(dev), b.to(dev), tab.to(dev), 3, 4, row, out_amax=big)
    assert torch.equal(big.view(torch.float32), torch.full((B,), 3.0e38, device=dev))
    plain = ops.token_layernorm(x.to(dev), w.to(dev), b.to(dev))
    n64 = F.layer_norm(x.double().transpose(1, 2), (E,), w.double(), b.double(), 1e-5).transpose(1, 2)
    n32 = F.layer_norm(x.transpose(1, 2), (E,), w, b, 1e-5).transpose(1, 2)
    check_kernel("  plain", plain, n32, n64)


@pytest.mark.parametrize("B,E,L,mode", [(1, 48, 60, "shared"), (3, 64, 64, "per_sample"), (3, 128, 1000, "row"), (1, 384, 1024, "per_sample"),
                                        (3, 384, 1024, "row"), (3, 48, 1000, "shared"), (2, 64, 63, "per_sample"), (1, 128, 1001, "row")])
def test_token_gate_is_bit_exact(ops, dev, B, E, L, mode):
    gen = torch.Generator().manual_seed(2000 + B + E + L)
    x, y = torch.randn(B, E, L, generator=gen), torch.randn(B, E, L, generator=gen)
    tab, row, rows = mod_table(mode, B, E, gen)
    want = x + rows[:, 2 * E:3 * E, None] * y              # a rounded product, then a rounded sum
    got = ops.token_gate(x.to(dev), y.to(dev), tab.to(dev), 2, row)
    assert torch.equal(got.cpu(), want)
    xd = x.to(dev)
    assert ops.token_gate(xd, y.to(dev), tab.to(dev), 2, row, out=xd) is xd and torch.equal(xd.cpu(), want)       # in place


@pytest.mark.parametrize("B,n", [(1, 4096), (3, 1000 * 48), (2, 1001)])
def test_silu_amax(ops, dev, B, n):
    gen = torch.Generator().manual_seed(n)
    x = 3 * torch.randn(B, n, generator=gen)
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    out = ops.silu_amax(x.to(dev), out_amax=slots)
    check_kernel(f"silu B={B} n={n}", out, F.silu(x), F.silu(x.double()))
    assert torch.equal(slots.view(torch.float32), out.abs().amax(dim=1))


PATCH_CASES = [(3, 1, 4, 32, 32, 64), (1, 3, 2, 40, 100, 48), (3, 3, 4, 24, 40, 128), (1, 1, 4, 128, 128, 384), (3, 1, 2, 16, 16, 128),
               (1, 3, 4, 128, 128, 64)]          # L = 64, 1000, 60, 1024, 64, 1024


@pytest.mark.parametrize("B,C,p,H,W,E", PATCH_CASES)
def test_patch_embed(ops, dev, B, C, p, H, W, E):
    gen = torch.Generator().manual_seed(3000 + E + H)
    K = C * p * p
    x, w, b = torch.randn(B, C, H, W, generator=gen), torch.randn(E, K, generator=gen) / K ** 0.5, torch.randn(E, generator=gen)
    got = ops.patch_embed(x.to(dev), w.to(dev), b.to(dev), p)
    assert got.shape == (B, E, (H // p) * (W // p))
    patches = dit_ref.patchify(x, p)
    check_kernel(f"patch_embed B={B} C={C} p={p} {H}x{W} E={E}", got, F.linear(patches, w, b).transpose(1, 2),
                 F.linear(patches.double(), w.double(), b.double()).transpose(1, 2))


@pytest.mark.parametrize("B,C,p,H,W,E", PATCH_CASES)
def test_patch_unembed(ops, dev, B, C, p, H, W, E):
    gen = torch.Generator().manual_seed(4000 + E + H)
    K, L = C * p * p, (H // p) * (W // p)
    x, w, b = torch.randn(B, E, L, generator=gen), torch.randn(K, E, generator=gen) / E ** 0.5, torch.randn(K, generator=gen)
    got = ops.patch_unembed(x.to(dev), w.to(dev), b.to(dev), p, (B, C, H, W))
    tok = x.transpose(1, 2)
    check_kernel(f"patch_unembed B={B} C={C} p={p} {H}x{W} E={E}", got, dit_ref.unpatchify(F.linear(tok, w, b), p, C, H, W),
                 dit_ref.unpatchify(F.linear(tok.double(), w.double(), b.double()), p, C, H, W))


# ------------------------------------------------------------------------------------------------------------------ the network
def golden_net(M, tag, dev, precision="fp16x3"):
    v, sd, kw = dit_ref.load_golden(tag)
    net = M.DiffusionTransformer(**kw)
    net.load_state_dict(sd, strict=True)
    net.conv_precision = precision
    return v, sd, kw, net.to(dev).eval()


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_forward_vs_reference(M, dev, tag, precision):
    v, _, _, net = golden_net(M, tag, dev, precision)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = net(v["x"].to(dev), v["t"].to(dev))
    assert net.conv_precision == precision
    check_network(f"dit_{tag} {precision}", out, v["out_f32"], v["out_f64"])


def test_heun_history_planned_and_captured(M, dev):
    from diffsci_amd.models.karras.engine import ModuleSource
    v, _, _, net = golden_net(M, "a", dev)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).to(dev)
    sch = module.config.noisescheduler
    orig = sch.create_steps
    sch.create_steps = lambda n: v["steps_4"].clone() if n == 5 else orig(n)      # the reference's own sigma grid
    wn = v["white_noise"].to(dev)
    assert ModuleSource(module, None, 1.0, wn.shape[0], wn).planned
    module.use_graph = False
    eager = module.propagate_white_noise(wn, nsteps=4, record_history=True)
    module.use_graph = True
    g1 = module.propagate_white_noise(wn, nsteps=4, record_history=True)
    assert len(module._plans.plans) == 1                                         # captured, not stepped
    g2 = module.propagate_white_noise(wn, nsteps=4, record_history=True)
    assert len(module._plans.plans) == 1
    assert torch.equal(eager, g1) and torch.equal(g1, g2)
    h32, h64 = v["hist_heun_N4_f32"], v["hist_heun_N4_f64"]
    assert eager.shape == h32.shape
    assert torch.equal(eager[0].cpu(), h32[0])                                   # x * sigma_max is exact
    for i in range(1, h32.shape[0]):
        check_network(f"heun state {i}", eager[i], h32[i], h64[i], scale=80.0)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_samples_are_independent(M, dev, tag):
    _, _, kw, net = golden_net(M, tag, dev)
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(3, kw.get("nchannels", 1), 32, 32, generator=gen) * torch.tensor([1.0, 30.0, 0.02])[:, None, None, None]
    t = torch.tensor([0.3, -1.1, 0.9])
    x, t = x.to(dev), t.to(dev)
    out = net(x, t)
    perm = torch.tensor([2, 0, 1], device=dev)
    assert torch.equal(net(x[perm].contiguous(), t[perm].contiguous()), out[perm])
    for i in range(3):
        assert torch.equal(net(x[i:i + 1].contiguous(), t[i:i + 1].contiguous()), out[i:i + 1])


@pytest.mark.parametrize("k", [-20, -8, 8, 20])
def test_magnitudes(M, dev, k):
    v, sd, kw, net = golden_net(M, "a", dev)
    x = v["x"] * 2.0 ** k
    with torch.inference_mode():
        f32 = dit_ref.dit_forward(sd, x, v["t"], kw.get("nheads", 4), kw.get("patch_size", 4))
        f64 = dit_ref.dit_forward({n: w.double() for n, w in sd.items()}, x, v["t"], kw.get("nheads", 4), kw.get("patch_size", 4))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # no escalation
        out = net(x.to(dev), v["t"].to(dev))
    assert net.conv_precision == "fp16x3"
    check_network(f"dit_a x 2^{k}", out, f32, f64)


def test_mid_size_against_dit_ref(M, dev):
    """nembed=256, nheads=4 (head width 64: the fp16x3 head-axis attention kernel), L = 1024; no golden at this size."""
    torch.manual_seed(390)
    net = M.DiffusionTransformer(nembed=256, nheads=4, nblocks=2, patch_size=4)
    with torch.no_grad():
        for name, w in net.state_dict().items():
            if ".norm" in name or name.endswith("bias"):
                w.add_(0.25 * torch.randn_like(w))
    sd = {n: w.clone() for n, w in net.state_dict().items()}
    x, t = torch.randn(2, 1, 128, 128), torch.tensor([0.3, -1.1])
    with torch.inference_mode():
        f32 = dit_ref.dit_forward(sd, x, t, 4, 4)
        f64 = dit_ref.dit_forward({n: w.double() for n, w in sd.items()}, x, t, 4, 4)
    net = net.to(dev).eval()
    for precision in ("fp16x3", "fp32"):
        net.conv_precision = precision
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            out = net(x.to(dev), t.to(dev))
        check_network(f"mid-size {precision}", out, f32, f64)
