"""Field-valued conditional embeddings on volumes (dimension=3 PUNetG / PUNetGCond) on a real MI355X: the corner-pool kernel
against torch bit for bit, the network against a golden made by the reference (tools/make_field3d_golden.py) and against an fp64
torch composition, eager and captured sampling, and the 2-D route unchanged next to it.

Bounds are those of the other volume tests: rel-L2 < 1e-5 against the reference's fp32 output and
< max(4 x reference-fp32-vs-fp64, 2e-6) against fp64."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import punetg_ref as R  # noqa: E402
from tests.golden_util import GOLDEN_DIR, load, rel_l2  # noqa: E402

REL = 1e-5
NAME = "punetg8_3d_spatial_cond"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


@pytest.fixture(scope="module")
def gold3d():
    """The fixture and its state_dict (spread over weight files to keep every committed file small)."""
    v, sd = load(NAME)
    i = 1
    while os.path.exists(os.path.join(GOLDEN_DIR, f"{NAME}_w{i}.npz")):
        sd.update(load(f"{NAME}_w{i}")[1])
        i += 1
    return v, sd


def _pin_grid(module):
    grids, _ = load("schedule")
    sch = module.config.noisescheduler
    orig = sch.create_steps
    sch.create_steps = lambda n: grids[f"steps_{n - 1}"].clone() if f"steps_{n - 1}" in grids else orig(n)


def _golden_net(M, gold3d, dev):
    v, sd = gold3d
    net = M.PUNetG(M.PUNetGConfig(model_channels=8, dimension=3), conditional_embedding=torch.nn.Conv3d(2, 8, kernel_size=1))
    r = net.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return net.to(dev).eval()


# ---------------------------------------------------------------- the kernel
def _want(x, f, te):
    sl = (Ellipsis,) + (slice(None, None, f),) * (x.dim() - 2)
    w = x[sl]
    if te is not None:
        w = w + te.view(te.shape + (1,) * (x.dim() - 2))
    return w


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


OUT_SIDES = [(3, 5), (4, 8), (1, 1), (6, 12), (2, 3, 5), (4, 4, 8), (1, 2, 1), (3, 2, 16)]


@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_cornerpool_is_torch_bit_for_bit(dev, f):
    from diffsci_amd import ops
    g = torch.Generator().manual_seed(10 + f)
    B, C = 2, 3
    for out_sides in OUT_SIDES:
        sides = tuple(v * f for v in out_sides)
        for xb in (1, B):
            x = (torch.randn((xb, C) + sides, generator=g) * 3).to(dev)
            x.view(-1)[::7] = -0.0
            for tb in (None, 1, B):
                te = None if tb is None else torch.randn(tb, C, generator=g).to(dev)
                want = _want(x, f, te)                               # batch max(xb, tb) by broadcasting
                amax = torch.zeros(want.shape[0], dtype=torch.int32, device=dev)
                got = ops.cornerpool_f(x, f, te=te, out_amax=amax)
                assert _bits(got, want), (f, sides, xb, tb)
                assert torch.equal(amax, ops.absmax_rows(got)), (f, sides, xb, tb)
                # out= sets the batch (x and te may both be shared); this one is not 16-byte aligned
                buf = torch.empty(B * want[0].numel() + 1, device=dev)
                o = buf[1:].view((B,) + tuple(want.shape[1:]))
                ops.cornerpool_f(x, f, te=te, out=o)
                assert _bits(o, want.expand_as(o)), (f, sides, xb, tb, "unaligned out")
                xs = torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape)
                xs.copy_(x)
                assert _bits(ops.cornerpool_f(xs, f, te=te), got), (f, sides, xb, tb, "unaligned x")


def test_cornerpool_merges_into_the_amax_row(dev):
    """The merge rule of absmax_rows: out[r] = max(out[r], bits of max |row|) -- a slot that already holds more keeps it."""
    from diffsci_amd import ops
    x = torch.randn(2, 4, 8, 8, 8, device=dev)
    big = torch.full((2,), 1e6, device=dev).view(torch.int32).clone()
    keep = big.clone()
    ops.cornerpool_f(x, 2, out_amax=big)
    assert torch.equal(big, keep)
    nan = x.clone()
    nan[1, 0, 0, 0, 0] = float("nan")                                  # NaNs are dropped, as ds_absmax_rows drops them
    a = torch.zeros(2, dtype=torch.int32, device=dev)
    got = ops.cornerpool_f(nan, 2, out_amax=a)
    assert torch.equal(a, ops.absmax_rows(got))


def test_cornerpool_large_output(dev):
    """128 MiB of output from one shared 512 MiB volume, and a 64 MiB field case with per-sample x."""
    from diffsci_amd import ops
    x = torch.randn(1, 8, 256, 256, 256, device=dev)
    te = torch.randn(2, 8, device=dev)
    a = torch.zeros(2, dtype=torch.int32, device=dev)
    got = ops.cornerpool_f(x, 2, te=te, out_amax=a)
    assert got.numel() * 4 >= 64 << 20
    assert torch.equal(got, _want(x, 2, te)) and torch.equal(a, ops.absmax_rows(got))
    del x, got
    x = torch.randn(2, 8, 3072, 3072, device=dev)
    got = ops.cornerpool_f(x, 3, te=te[:1])
    assert got.numel() * 4 >= 64 << 20 and torch.equal(got, _want(x, 3, te[:1]))


# ---------------------------------------------------------------- the network against the reference's golden
def _set(net, prec):
    net.conv_precision, net.auto_precision = prec, False


@pytest.mark.parametrize("prec", ["fp16x3", "bf16x6", "fp32"])
def test_network_matches_the_reference(M, gold3d, dev, prec):
    """Measured on an MI355X, rel-L2 against the reference's fp32 output (bound 1e-5) / fp64 output (bound 4.86e-6):
    fp16x3 1.44e-6 / 8.69e-7, bf16x6 and fp32 1.63e-6 / 1.32e-6; the unconditional call 1.41e-6 (fp16x3), 1.66e-6 (the others)."""
    v, _ = gold3d
    net = _golden_net(M, gold3d, dev)
    _set(net, prec)
    x, t, y = v["x"].to(dev), v["t"].to(dev), v["y"].to(dev)
    assert net.condition_is_field(y) and not net.condition_is_field(None)
    out = net(x, t, y).cpu()
    bound = max(4 * rel_l2(v["out_f32"], v["out_f64"]), 2e-6)
    e32, e64 = rel_l2(out, v["out_f32"]), rel_l2(out, v["out_f64"])
    print(f"[golden {prec}] vs reference fp32 {e32:.2e} (bound {REL:.0e}), vs fp64 {e64:.2e} (bound {bound:.2e})")
    assert out.shape == (2, 1, 16, 16, 16) and e32 < REL and e64 < bound
    eu = rel_l2(net(x, t).cpu(), v["out_uncond_f32"])
    print(f"[golden {prec}] unconditional vs reference fp32 {eu:.2e}")
    assert eu < REL
    # the samples of a batch are independent: sample 0 alone gives the same bits
    alone = net(x[:1], t[:1], y[:1]).cpu()
    assert torch.equal(alone[0], out[0])
    # a field shared by the batch ([1, ...]) is the same as its copies
    y1 = y[:1]
    assert torch.equal(net(x, t, y1).cpu(), net(x, t, y1.expand(2, -1, -1, -1, -1).contiguous()).cpu())


def test_one_block_with_a_pooled_field(M, gold3d, dev):
    """One level-1 block: the per-voxel shift of a 16^3 field, corner-pooled to 8^3, added through conv1's res1 (measured:
    1.34e-7 against the reference's block output)."""
    from diffsci_amd import ops
    from diffsci_amd.models.nets.punetg import _FieldShifts
    v, _ = gold3d
    net = _golden_net(M, gold3d, dev)
    blk, pk, ws = net.downward_blocks[1][0], net.packed_weights(), net._ws
    h, te = v["resblock_in"].to(dev), v["resblock_te"].to(dev)
    fs = _FieldShifts(te, ws, True, batch=2)
    yt = net._field_shift(blk, fs, 8, 8, 8)
    assert yt.shape == (2, 16, 64, 8)
    sd = {k: w.detach().double().cpu() for k, w in blk.state_dict().items()}
    want_yt = R.time_shift(sd, "timeblock.", v["resblock_te"].double(), ndim=3)[..., ::2, ::2, ::2]
    assert rel_l2(yt.view(2, 16, 8, 8, 8).cpu(), want_yt) < 2e-6
    k1, k2 = net.norm_kinds
    a = ops.inorm_silu(h, blk.gnorm1.weight, blk.gnorm1.bias, kind=k1)
    y = ops.conv3d_mfma(a, pk[(id(blk.conv1), "3d")], bias=blk.conv1.bias, res1=yt.view(2, 16, 8, 8, 8))
    a = ops.inorm_silu(y, blk.gnorm2.weight, blk.gnorm2.bias, kind=k2)
    got = ops.conv3d_mfma(a, pk[(id(blk.conv2), "3d")], bias=blk.conv2.bias, res1=h)
    ws.give(yt)
    fs.release()
    err = rel_l2(got.cpu(), v["resblock_l1"])
    print(f"[level-1 block, 16^3 field pooled to 8^3] vs reference fp32 {err:.2e}")
    assert err < REL


def test_captured_sampling(M, gold3d, dev):
    """Eager, capture and replay give equal bits and one plan per guidance mode; a second condition reuses the plan.  Measured:
    Heun N = 4 histories 9.22e-8 (guidance 1) and 1.64e-7 (guidance 2) against the reference's, bound 1e-5."""
    from diffsci_amd.models.karras import engine
    v, _ = gold3d
    net = _golden_net(M, gold3d, dev)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), conditional=True).to(dev)
    _pin_grid(module)
    x, y, wn = v["x"].to(dev), v["y"].to(dev), v["white_noise"].to(dev)
    src = engine.ModuleSource(module, y[:1], 1.0, 2, x)
    assert src.planned and src.field and not src.batched_cfg
    last = None
    for g in (1.0, 2.0):
        runs = []
        for use_graph in (False, True, True):
            module.use_graph = use_graph
            h = module.propagate_white_noise(wn, y=y[0], guidance=g, nsteps=4, record_history=True).cpu()
            err = rel_l2(h, v[f"hist_heun_N4_g{int(g)}_f32"])
            print(f"[Heun N=4 guidance {g} graph={use_graph}] history vs reference fp32 {err:.2e}")
            assert err < REL
            runs.append(h)
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2])          # eager, capture + replay, replay
        last = runs[-1]
    assert len(module._plans.plans) == 2
    y2 = y[0] * 0.5 + 0.25
    a = module.propagate_white_noise(wn, y=y2, guidance=2.0, nsteps=4, record_history=True)
    module.use_graph = False
    b = module.propagate_white_noise(wn, y=y2, guidance=2.0, nsteps=4, record_history=True)
    assert len(module._plans.plans) == 2 and torch.equal(a, b) and not torch.equal(a.cpu(), last)


# ---------------------------------------------------------------- against an fp64 composition (torch ops only)
def _compose(sd, cfg, x, t, ye, f):
    """PUNetG.forward with MaxPool3d(f) / nearest Upsample(f) transitions and a field-valued te: the building blocks of
    oracle/punetg_ref.py (resnet_block evaluates the time MLP per voxel and corner-pools it to the block, as rescale_yt does)."""
    circ = cfg.get("convolution_type", "default") == "circular"
    norms = (cfg.get("first_resblock_norm", "GroupLN"), cfg.get("second_resblock_norm", "GroupRMS"))
    nlev = len(cfg["channel_expansion"])
    x = R.conv3x3(sd, "convin", x, circ)
    te = R.fourier_features(t, sd["time_projection.W"]).reshape(t.numel(), -1, 1, 1, 1) + ye
    skips = []
    for lv in range(nlev):
        for r in range(cfg["number_resnet_downward_block"]):
            x = R.resnet_block(sd, f"downward_blocks.{lv}.{r}.", x, te, circ, norms)
        skips.append(x)
        x = R.conv3x3(sd, f"downsamplers.{lv}.conv", F.max_pool3d(x, f), circ)
    for r in range(cfg["number_resnet_before_attn_block"]):
        x = R.resnet_block(sd, f"before_block.{r}.", x, te, circ, norms)
    xa, nattn = x, cfg["number_resnet_attn_block"]
    for r in range(nattn):
        xa = R.resnet_block(sd, f"attn_resnet_block.{r}.", xa, te, circ, norms)
        if r < nattn - 1:
            xa = R.attention_2d(sd, f"attn_block.{r}.", xa, cfg["attn_residual"])
    x = x + xa
    for r in range(cfg["number_resnet_after_attn_block"]):
        x = R.resnet_block(sd, f"after_block.{r}.", x, te, circ, norms)
    for lv in range(nlev):
        x = R.conv3x3(sd, f"upsamplers.{lv}.conv", F.interpolate(x, scale_factor=f, mode="nearest"), circ) + skips.pop()
        for r in range(cfg["number_resnet_upward_block"]):
            x = R.resnet_block(sd, f"upward_blocks.{lv}.{r}.", x, te, circ, norms)
    return R.conv3x3(sd, "convout", x, circ)


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, w in m.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                w.add_(0.1 * torch.randn(w.shape, generator=g))
    return m


def _oracle(net, x, t, ye, f, skip=("conditional_embedding.",)):
    cfg = R.default_config(model_channels=net.config.model_channels)
    d = net.config.export_description()
    cfg.update({k: v for k, v in d.items() if k in cfg or k == "convolution_type"})
    sd = {k: w.detach().cpu().clone() for k, w in net.state_dict().items() if not k.startswith(skip)}
    want = _compose({k: w.double() for k, w in sd.items()}, cfg, x.double(), t.double(), ye.double(), f)
    want32 = _compose(sd, cfg, x, t, ye, f)
    return want, max(4 * rel_l2(want32, want), 2e-6)


def test_the_composition_restates_the_reference(gold3d):
    """The fp64 composition on the golden case against the reference's own fp64 network (CPU arithmetic only; 2.0e-15 and
    3.6e-15 on the two hosts it has run on)."""
    v, sd = gold3d
    sd64 = {k: w.double() for k, w in sd.items()}
    ye = F.conv3d(v["y"].double(), sd64["conditional_embedding.weight"], sd64["conditional_embedding.bias"])
    want = _compose(sd64, R.default_config(model_channels=8), v["x"].double(), v["t"].double(), ye, 2)
    err = rel_l2(want, v["out_f64"])
    print(f"[composition vs the reference's fp64 network] {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("prec", ["fp16x3", "bf16x6", "fp32"])
def test_finer_field_periodic_factor_four(M, dev, prec):
    """A 32^3 field on a 16^3 network (level 0 already pools, by 2; the bottom by 8), periodic padding, one transition by 4.
    Measured against fp64 (bound 9.77e-6 = 4 x torch-fp32-vs-fp64): fp16x3 2.00e-6, bf16x6 and fp32 2.53e-6."""
    torch.manual_seed(200)
    cfg = M.PUNetGConfig(model_channels=8, dimension=3, channel_expansion=[2], transition_scale_factor=4, convolution_type="circular")
    net = _perturb(M.PUNetG(cfg, conditional_embedding=torch.nn.Identity()), 201)
    g = torch.Generator().manual_seed(202)
    x, t = torch.randn(2, 1, 16, 16, 16, generator=g), torch.rand(2, generator=g)
    ye = torch.randn(2, 8, 32, 32, 32, generator=g) * 0.5
    want, bound = _oracle(net, x, t, ye, 4)
    net = net.to(dev).eval()
    _set(net, prec)
    got = net(x.to(dev), t.to(dev), ye.to(dev)).cpu()
    err = rel_l2(got, want)
    print(f"[32^3 field, 16^3 periodic network, factor 4, {prec}] vs fp64 {err:.2e}, bound {bound:.2e}")
    assert got.shape == x.shape and err < bound
    moved = rel_l2(got, net(x.to(dev), t.to(dev)).cpu())
    assert moved > 1e-3                                                # the condition matters


class _FieldOfRest(torch.nn.Module):
    """conditional_embedding of a PUNetGCond: a 1x1x1 convolution of the item the channel concatenation left over."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv3d(2, 8, kernel_size=1)

    def forward(self, y):
        return self.conv(y["f"])


def test_conditional_network_with_a_field_embedding(M, dev):
    """PUNetGCond(dimension=3): one channel-concatenated item, a field embedding of the rest; eager and captured.
    Measured against fp64: 1.18e-6 (bound 5.65e-6)."""
    torch.manual_seed(210)
    cfg = M.PUNetGConfig(model_channels=8, dimension=3, input_channels=2)
    net = _perturb(M.nets.PUNetGCond(cfg, conditional_embedding=_FieldOfRest(), channel_conditional_items=["c"]), 211)
    g = torch.Generator().manual_seed(212)
    x, t = torch.randn(2, 1, 16, 16, 16, generator=g), torch.rand(2, generator=g)
    c, fld = torch.randn(2, 1, 16, 16, 16, generator=g), torch.randn(2, 2, 16, 16, 16, generator=g)
    with torch.no_grad():
        ye = net.conditional_embedding.double()({"f": fld.double()}).float()
        net.conditional_embedding.float()
    want, bound = _oracle(net, torch.cat([x, c], dim=1), t, ye, 2)
    net = net.to(dev).eval()
    y = {"c": c.to(dev), "f": fld.to(dev)}
    got = net(x.to(dev), t.to(dev), y).cpu()
    err = rel_l2(got, want)
    print(f"[PUNetGCond 3-D, channel item + field embedding] vs fp64 {err:.2e}, bound {bound:.2e}")
    assert got.shape == x.shape and err < bound
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), conditional=True).to(dev)
    wn = torch.randn(2, 1, 16, 16, 16, generator=g).to(dev)
    y0 = {"c": c[0].to(dev), "f": fld[0].to(dev)}
    runs = []
    for use_graph in (False, True, True):
        module.use_graph = use_graph
        runs.append(module.propagate_white_noise(wn, y=y0, nsteps=3))
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1]) and torch.equal(runs[1], runs[2])
    assert len(module._plans.plans) == 1


def test_2d_route_is_unchanged_next_to_a_volume_network(M, gold3d, dev):
    v2, sd2 = load("punetg8_spatial_cond")
    net2 = M.PUNetG(M.PUNetGConfig(model_channels=8), conditional_embedding=torch.nn.Conv2d(2, 8, kernel_size=1))
    net2.load_state_dict(sd2, strict=True)
    net2 = net2.to(dev).eval()
    x2, t2, y2 = v2["x"].to(dev), v2["t"].to(dev), v2["y"].to(dev)
    before = net2(x2, t2, y2).clone()
    assert rel_l2(before.cpu(), v2["out_f32"]) < REL
    v, _ = gold3d
    net3 = _golden_net(M, gold3d, dev)
    assert rel_l2(net3(v["x"].to(dev), v["t"].to(dev), v["y"].to(dev)).cpu(), v["out_f32"]) < REL
    assert torch.equal(net2(x2, t2, y2), before)


def test_refusals(M, gold3d, dev):
    v, _ = gold3d
    net = _golden_net(M, gold3d, dev)
    x, t = v["x"].to(dev), v["t"].to(dev)
    net.set_conditional_embedding(torch.nn.Identity())
    with pytest.raises(ValueError, match="rank 5"):
        net(x, t, torch.zeros(1, 8, 16, 16, device=dev))
    with pytest.raises(ValueError, match="model_channels channels"):
        net(x, t, torch.zeros(1, 4, 16, 16, 16, device=dev))
    with pytest.raises(ValueError, match=r"yt_dims \(24, 24, 24\) and y_dims \(16, 16, 16\)"):
        net(x, t, torch.zeros(1, 8, 24, 24, 24, device=dev))
    with pytest.raises(ValueError, match="not compatible"):
        net(x, t, torch.zeros(1, 8, 32, 32, 16, device=dev))
    with pytest.raises(NotImplementedError, match="coarser"):
        net(x, t, torch.zeros(1, 8, 8, 8, 8, device=dev))
    with pytest.raises(ValueError, match="batch"):
        net(x, t, torch.zeros(3, 8, 16, 16, 16, device=dev))
    # ... and the network still runs after them
    assert net(x, t, torch.zeros(1, 8, 16, 16, 16, device=dev)).shape == x.shape
