"""ConVit on a real MI355X: the streaming kernels (ds_convit.hip) against fp64 torch compositions, the network against the
reference's goldens (tests/golden/convit_*.npz) and against tests/convit_ref.py where no golden exists, and the captured sampler.

Bounds, all against fp64:
  kernels   rel-L2 and max-abs error at most 4 x the error torch's fp32 CPU result has on the same inputs, computed
            here, with floors of 1e-7 rel-L2 and one fp32 ulp of the largest value for the cases where torch happens to be exact;
  network   rel-L2 <= max(1e-5, 4 x the reference's own fp32-vs-fp64 distance), max-abs <= max(1e-4 x max |out|, 4 x the
            reference fp32 output's own max-abs error)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import convit_ref  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

ULP = 2.0 ** -23
EPS = float(torch.finfo(torch.float32).eps)


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


def slots_of(t):
    """Per-sample max |t| as the amax slots hold it."""
    return t.abs().amax(dim=tuple(range(1, t.dim())))


def mod_table(mode, B, E, gen):
    """(table, row) in the forms the kernel takes, and the [B, E] rows they mean (None: no embedding row)."""
    if mode == "none":
        return None, None, None
    if mode == "shared":                                  # one row for the batch: stride 0
        tab = torch.randn(1, E, generator=gen)
        return tab, None, tab.expand(B, -1)
    if mode == "per_sample":                              # stride E
        tab = torch.randn(B, E, generator=gen)
        return tab, None, tab
    tab = torch.randn(5, E, generator=gen)                # the sampler's table of all evaluations: a non-zero row
    return tab, 3, tab[3:4].expand(B, -1)


def rms_ref(x, w, rows, pool, dt):
    x = x.to(dt)
    n = x / torch.sqrt(torch.mean(x ** 2, dim=1, keepdim=True) + EPS) * w.to(dt).view(1, -1, 1, 1)
    if rows is not None:
        n = n + rows.to(dt)[:, :, None, None]
    return F.avg_pool2d(n, pool) if pool > 1 else n


RMS_CASES = [(1, 48, 6, 10, "shared", 1, 1.0), (3, 64, 8, 8, "per_sample", 2, 1.0), (3, 128, 5, 7, "row", 1, 1.0),
             (1, 384, 32, 32, "per_sample", 4, 1.0), (2, 64, 12, 20, "none", 2, 1.0),
             (3, 64, 8, 8, "per_sample", 2, 1e4),          # x * 1e4
             (2, 64, 10, 6, "row", 2, 1.0), (1, 48, 9, 7, "shared", 2, 1.0),       # odd sides: the floor of the pooled size
             (1, 200, 8, 12, "per_sample", 4, 1.0), (2, 48, 6, 12, "shared", 6, 1.0),     # a ragged channel count; an unfused factor
             # the widest E the entry point accepts: 16-byte lanes with 32 channels per thread, 4-byte lanes with 128 (unpooled and
             # pooled), and a width between the last two register counts
             (1, 1024, 4, 8, "shared", 1, 1.0), (2, 1024, 3, 5, "row", 1, 1.0), (1, 1024, 4, 8, "per_sample", 2, 1.0),
             (1, 520, 4, 4, "per_sample", 1, 1.0)]


@pytest.mark.parametrize("B,E,H,W,mode,pool,mag", RMS_CASES)
def test_channel_rmsnorm(ops, dev, B, E, H, W, mode, pool, mag):
    gen = torch.Generator().manual_seed(1000 + B * 7 + E + H * W + pool)
    x = mag * torch.randn(B, E, H, W, generator=gen) * (1.0 + torch.rand(B, 1, H, W, generator=gen))
    w = 1 + 0.25 * torch.randn(E, generator=gen)
    tab, row, rows = mod_table(mode, B, E, gen)
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    tabd = None if tab is None else tab.to(dev)
    out = ops.channel_rmsnorm(x.to(dev), w.to(dev), tabd, row, pool=pool, out_amax=slots)
    assert out.shape == (B, E, H // pool, W // pool)
    check_kernel(f"rmsnorm B={B} E={E} {H}x{W} {mode} pool={pool} x{mag:g}", out, rms_ref(x, w, rows, pool, torch.float32),
                 rms_ref(x, w, rows, pool, torch.float64))
    assert torch.equal(slots.view(torch.float32), slots_of(out))
    big = torch.full((B,), 3.0e38, device=dev).view(torch.int32).clone()          # merged into, not overwritten
    ops.channel_rmsnorm(x.to(dev), w.to(dev), tabd, row, pool=pool, out_amax=big)
    assert torch.equal(big.view(torch.float32), torch.full((B,), 3.0e38, device=dev))


@pytest.mark.parametrize("pool", [1, 2])
def test_channel_rmsnorm_of_a_zero_pixel_is_zero(ops, dev, pool):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 64, 8, 8, generator=gen)
    x[1, :, 2:4, 4:6] = 0.0
    w = 1 + 0.25 * torch.randn(64, generator=gen)
    out = ops.channel_rmsnorm(x.to(dev), w.to(dev), pool=pool)
    assert torch.isfinite(out).all()
    zero = out[1, :, 1, 2] if pool == 2 else out[1, :, 2:4, 4:6]
    assert torch.equal(zero, torch.zeros_like(zero))
    check_kernel(f"rmsnorm zero pixel pool={pool}", out, rms_ref(x, w, None, pool, torch.float32), rms_ref(x, w, None, pool, torch.float64))


def rope_ref(qkv, E, heads, angles, grid, relative, dt):
    """convit.py:369-388 on the q and k thirds of qkv [B, 3E, L]."""
    B, _, L = qkv.shape
    d = E // heads
    out = qkv.to(dt).clone()
    for third in (0, 1):
        t = out[:, third * E:(third + 1) * E].reshape(B, heads, d, *grid).permute(0, 1, 3, 4, 2).reshape(B * heads, *grid, d)
        t = convit_ref.rope(t, angles.to(dt), relative)
        out[:, third * E:(third + 1) * E] = t.reshape(B, heads, *grid, d).permute(0, 1, 4, 2, 3).reshape(B, E, L)
    return out


@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("B,E,heads,grid", [(2, 64, 8, (8, 8)), (1, 128, 4, (16, 16)), (3, 64, 2, (6, 10)), (1, 64, 1, (1, 1)), (2, 48, 4, (5, 7))])
def test_rope2d(ops, dev, B, E, heads, grid, relative):
    from diffsci_amd.models.nets.convit import LearnedRoPE
    torch.manual_seed(2000 + E + heads + grid[0])
    L = grid[0] * grid[1]
    layer = LearnedRoPE(embed_dim=E // heads, num_pos_dims=2, base_freq=1.0, relative_positioning=relative)
    qkv = torch.randn(B, 3 * E, L) * torch.tensor([1.0, 3.0, 0.5])[:B, None, None]
    qd = qkv.to(dev)
    slots = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    got = ops.rope2d(qd, E, heads, layer.to(dev).cos_sin(grid), out_amax=slots)
    assert got is qd
    angles = layer.angles.detach().cpu()
    check_kernel(f"rope B={B} E={E} heads={heads} grid={grid} relative={relative}", got, rope_ref(qkv, E, heads, angles, grid, relative, torch.float32),
                 rope_ref(qkv, E, heads, angles, grid, relative, torch.float64))
    assert torch.equal(got[:, 2 * E:].cpu(), qkv[:, 2 * E:])                      # v: bit-identical
    pair = slots.view(torch.float32).view(2, B)
    assert torch.equal(pair[0], slots_of(got[:, :2 * E])) and torch.equal(pair[1], slots_of(got[:, 2 * E:]))


@pytest.mark.parametrize("C", [3, 48])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8), (12, 20)])
@pytest.mark.parametrize("f", [1, 2, 4, 3])
def test_upsample_bilinear(ops, dev, f, H, W, C):
    gen = torch.Generator().manual_seed(3000 + f + H + C)
    x = torch.randn(2, C, H, W, generator=gen)
    got = ops.upsample_bilinear(x.to(dev), f)
    assert got.shape == (2, C, H * f, W * f)
    check_kernel(f"bilinear x{f} {H}x{W} C={C}", got, F.interpolate(x, scale_factor=f, mode="bilinear", align_corners=False),
                 F.interpolate(x.double(), scale_factor=f, mode="bilinear", align_corners=False))


@pytest.mark.parametrize("E", [48, 128])
@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (32, 32), (9, 40)])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_depthwise_conv_silu(ops, dev, k, H, W, E):
    gen = torch.Generator().manual_seed(4000 + k + H + E)
    B = 2
    x = torch.randn(B, E, H, W, generator=gen) * torch.tensor([1.0, 20.0])[:, None, None, None]
    w, b = torch.randn(E, 1, k, k, generator=gen) / k, 0.25 * torch.randn(E, generator=gen)
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    got = ops.depthwise_conv_silu(x.to(dev), w.to(dev), b.to(dev), out_amax=slots)
    check_kernel(f"depthwise k={k} {H}x{W} E={E}", got, F.silu(F.conv2d(x, w, b, padding="same", groups=E)),
                 F.silu(F.conv2d(x.double(), w.double(), b.double(), padding="same", groups=E)))
    assert torch.equal(slots.view(torch.float32), slots_of(got))


GATE_SIZES = [(1, 48, 5, 7), (3, 128, 32, 32)]


@pytest.mark.parametrize("B,C,H,W", GATE_SIZES)
def test_swiglu(ops, dev, B, C, H, W):
    gen = torch.Generator().manual_seed(5000 + C)
    ag = 3 * torch.randn(B, 2 * C, H, W, generator=gen)
    slots = torch.zeros(B, dtype=torch.int32, device=dev)
    got = ops.swiglu(ag.to(dev), out_amax=slots)
    assert got.shape == (B, C, H, W)
    check_kernel(f"swiglu {B}x{2 * C}x{H}x{W}", got, F.silu(ag[:, :C]) * ag[:, C:], F.silu(ag[:, :C].double()) * ag[:, C:].double())
    assert torch.equal(slots.view(torch.float32), slots_of(got))


@pytest.mark.parametrize("B,C,H,W", GATE_SIZES)
def test_convit_blend(ops, dev, B, C, H, W):
    gen = torch.Generator().manual_seed(6000 + C)
    u, xc, x0 = (torch.randn(B, C, H, W, generator=gen) for _ in range(3))
    s = torch.sigmoid(torch.tensor([0.37]))

    def ref(dt):
        sd = s.to(dt)
        return (1 - sd) * u.to(dt) + sd * xc.to(dt) + x0.to(dt)

    got = ops.convit_blend(u.to(dev), xc.to(dev), x0.to(dev), s.to(dev))
    check_kernel(f"blend {B}x{C}x{H}x{W}", got, ref(torch.float32), ref(torch.float64))
    x0d = x0.to(dev)
    assert ops.convit_blend(u.to(dev), xc.to(dev), x0d, s.to(dev), out=x0d) is x0d and torch.equal(x0d, got)       # in place on x0


# ------------------------------------------------------------------------------------------------------------------ the network
def build(M, kw, sd=None):
    net = M.nets.ConVit(M.nets.ConVitConfig(**kw), conditional_embedding=torch.nn.Linear(1, kw.get("embed_dim", 64)))
    if sd is not None:
        net.load_state_dict(sd, strict=True)
    return net


def golden_net(M, tag, dev, precision="fp16x3"):
    v, sd, kw = convit_ref.load_golden(tag)
    net = build(M, kw, sd)
    net.conv_precision = precision
    return v, sd, kw, net.to(dev).eval()


def ref_kwargs(kw):
    return dict(attn_compression_factor=kw.get("attn_compression_factor", 2), relative_positioning=kw.get("relative_positioning", False))


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_forward_vs_reference(M, dev, tag, precision):
    v, _, _, net = golden_net(M, tag, dev, precision)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = net(v["x"].to(dev), v["t"].to(dev), v["y"].to(dev))
        out_nocond = net(v["x"].to(dev), v["t"].to(dev))
    assert net.conv_precision == precision
    check_network(f"convit_{tag} {precision}", out, v["out_f32"], v["out_f64"])
    check_network(f"convit_{tag} {precision} y=None", out_nocond, v["out_nocond_f32"], v["out_nocond_f64"])


def test_no_t_and_no_y_means_no_embedding_row(M, dev):
    v, sd, kw, net = golden_net(M, "c", dev)
    with torch.inference_mode():
        f32 = convit_ref.convit_forward(sd, v["x"], None, None, **ref_kwargs(kw))
        f64 = convit_ref.convit_forward({n: w.double() for n, w in sd.items()}, v["x"], None, None, **ref_kwargs(kw))
    check_network("convit_c without t and y", net(v["x"].to(dev)), f32, f64)
    with torch.inference_mode():                                             # y alone: ye is the whole embedding
        f32 = convit_ref.convit_forward(sd, v["x"], None, v["y"], **ref_kwargs(kw))
        f64 = convit_ref.convit_forward({n: w.double() for n, w in sd.items()}, v["x"], None, v["y"], **ref_kwargs(kw))
    check_network("convit_c with y alone", net(v["x"].to(dev), None, v["y"].to(dev)), f32, f64)


@pytest.mark.parametrize("name,guidance", [("heun", 1.0), ("cfg2", 2.0)])
def test_history_planned_and_captured(M, dev, name, guidance):
    from diffsci_amd.models.karras.engine import ModuleSource
    v, _, _, net = golden_net(M, "a", dev)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), conditional=True).to(dev).eval()
    sch = module.config.noisescheduler
    orig = sch.create_steps
    sch.create_steps = lambda n: v["steps_4"].clone() if n == 5 else orig(n)      # the reference's own sigma grid
    wn, y = v["white_noise"].to(dev), v["y_hist"].to(dev)
    src = ModuleSource(module, y.unsqueeze(0), guidance, wn.shape[0], wn)
    assert src.planned and src.batched_cfg == (guidance != 1.0)
    kw = dict(y=y, guidance=guidance, nsteps=4, record_history=True)
    module.use_graph = False
    eager = module.propagate_white_noise(wn, **kw)
    module.use_graph = True
    g1 = module.propagate_white_noise(wn, **kw)
    assert len(module._plans.plans) == 1                                         # captured, not stepped
    g2 = module.propagate_white_noise(wn, **kw)
    assert len(module._plans.plans) == 1
    assert torch.equal(eager, g1) and torch.equal(g1, g2)
    h32, h64 = v[f"hist_{name}_N4_f32"], v[f"hist_{name}_N4_f64"]
    assert eager.shape == h32.shape
    assert torch.equal(eager[0].cpu(), h32[0])                                   # x * sigma_max is exact
    for i in range(1, h32.shape[0]):
        check_network(f"{name} state {i}", eager[i], h32[i], h64[i], scale=80.0)


def test_per_sample_conditions_take_the_per_sample_tables(M, dev):
    """An embedded condition with one row per sample: [n_evals, B, E] tables in the planned sampler; every sample equals its own
    run with the one condition."""
    v, _, _, net = golden_net(M, "a", dev)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), conditional=True).to(dev).eval()
    wn, y = v["white_noise"].to(dev), v["y"].to(dev)                            # y [B, 1] -> ye [B, E]
    both = module.propagate_white_noise(wn, y=y, nsteps=2)
    for i in range(wn.shape[0]):
        one = module.propagate_white_noise(wn[i:i + 1].contiguous(), y=y[i], nsteps=2)
        assert torch.equal(one, both[i:i + 1])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_samples_are_independent(M, dev, tag):
    _, _, kw, net = golden_net(M, tag, dev)
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(3, kw.get("in_channels", 1), 32, 32, generator=gen) * torch.tensor([1.0, 30.0, 0.02])[:, None, None, None]
    t, y = torch.tensor([0.3, -1.1, 0.9]), torch.tensor([[0.7], [-0.4], [0.1]])
    x, t, y = x.to(dev), t.to(dev), y.to(dev)
    out = net(x, t, y)
    perm = torch.tensor([2, 0, 1], device=dev)
    assert torch.equal(net(x[perm].contiguous(), t[perm].contiguous(), y[perm].contiguous()), out[perm])
    for i in range(3):
        assert torch.equal(net(x[i:i + 1].contiguous(), t[i:i + 1].contiguous(), y[i:i + 1].contiguous()), out[i:i + 1])


@pytest.mark.parametrize("k", [-20, -8, 8, 20])
def test_magnitudes(M, dev, k):
    v, sd, kw, net = golden_net(M, "a", dev)
    x = v["x"] * 2.0 ** k
    with torch.inference_mode():
        f32 = convit_ref.convit_forward(sd, x, v["t"], v["y"], **ref_kwargs(kw))
        f64 = convit_ref.convit_forward({n: w.double() for n, w in sd.items()}, x, v["t"], v["y"], **ref_kwargs(kw))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # no escalation
        out = net(x.to(dev), v["t"].to(dev), v["y"].to(dev))
    assert net.conv_precision == "fp16x3"
    check_network(f"convit_a x 2^{k}", out, f32, f64)


def test_mid_size_against_convit_ref(M, dev):
    """embed_dim=256, 4 heads (head width 64: the fp16x3 head-axis attention kernel), L = 1024; no golden at this size."""
    torch.manual_seed(490)
    kw = dict(embed_dim=256, num_heads=4, num_layers=1, has_time_embedding=True, has_conditional_embedding=True)
    net = build(M, kw)
    with torch.no_grad():
        for name, w in net.state_dict().items():
            if "norm" in name or ".rms." in name or name.endswith("bias") or name.endswith("fusion_weight"):
                w.add_(0.25 * torch.randn_like(w))
    sd = {n: w.clone() for n, w in net.state_dict().items()}
    x, t, y = torch.randn(2, 1, 64, 64), torch.tensor([0.3, -1.1]), torch.tensor([[0.7], [-0.4]])
    with torch.inference_mode():
        f32 = convit_ref.convit_forward(sd, x, t, y)
        f64 = convit_ref.convit_forward({n: w.double() for n, w in sd.items()}, x, t, y)
    net = net.to(dev).eval()
    for precision in ("fp16x3", "fp32"):
        net.conv_precision = precision
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            out = net(x.to(dev), t.to(dev), y.to(dev))
        check_network(f"mid-size {precision}", out, f32, f64)
