"""PUNetG with transition_scale_factor other than 2 on a real MI355X: the max-pool kernel against torch, whole networks (2-D and
3-D, every convolution precision and route) against an fp64 torch composition with the factor, the public stage methods,
eager vs captured sampling, and factor 2 unchanged next to another factor.

Bounds: max pooling is exact, so ds_maxpool_f is bit-identical to F.max_pool{2,3}d; networks stay within
max(4 x torch-fp32-vs-fp64, 2e-6) rel-L2, as the other parity tests."""
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import punetg_ref as R  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


# ---------------------------------------------------------------- the kernel
POOL_SHAPES = [(2, 3, 12, 12), (2, 3, 13, 14), (1, 5, 25, 31), (2, 2, 64, 64), (1, 1, 7, 7), (3, 2, 8, 36),
               (2, 3, 12, 12, 12), (1, 2, 13, 9, 14), (1, 2, 8, 16, 20), (1, 1, 7, 7, 7), (2, 1, 7, 8, 28)]


def _torch_pool(x, f):
    return (F.max_pool3d if x.dim() == 5 else F.max_pool2d)(x, f)


def _same(a, b):
    """Equal shapes, NaN where the other has NaN, and the same bits everywhere else (signed zeros included)."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num().view(torch.int32), b.nan_to_num().view(torch.int32))


@pytest.mark.parametrize("f", [1, 3, 4, 5, 7])
def test_maxpool_is_torch_bit_for_bit(dev, f):
    from diffsci_amd import ops
    g = torch.Generator().manual_seed(f)
    for shape in POOL_SHAPES:
        if f > min(shape[2:]):
            continue
        x = torch.randn(shape, generator=g) * 3
        x[..., ::5] = 0.0
        x[..., 1::7] = -0.0                                       # signed zeros: the first of equal values wins, as in torch
        got = ops.maxpool_f(x.to(dev), f).cpu()
        assert _same(got, _torch_pool(x, f)), (shape, f)
        assert _same(got, _torch_pool(x.to(dev), f).cpu()), (shape, f)
        # the wrapper's out= and a sub-view that is not 16-byte aligned (the scalar-store route)
        buf = torch.empty(got.numel() + 1, device=dev)
        o = buf[1:].view(got.shape)
        ops.maxpool_f(x.to(dev), f, out=o)
        assert _same(o.cpu(), got)
        xs = torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape)
        xs.copy_(x.to(dev))
        assert _same(ops.maxpool_f(xs, f).cpu(), got)               # x not 16-byte aligned: no float4 loads


@pytest.mark.parametrize("f", [1, 3, 4, 5, 7])
def test_maxpool_nan_and_infinite_windows(dev, f):
    from diffsci_amd import ops
    g = torch.Generator().manual_seed(100 + f)
    for shape in ((2, 2, 4 * f, 4 * f + 1), (1, 2, 2 * f, 3 * f, 4 * f)):
        x = torch.randn(shape, generator=g)
        x.view(-1)[::11] = float("nan")
        x.view(-1)[3::17] = float("inf")
        if x.dim() == 4:
            x[:, :, :f, :f] = float("-inf")                        # an all -inf window
            x[:, :, f:2 * f, :f] = float("-inf")
            x[:, :, f, 0] = float("nan")                           # NaN after -inf
        else:
            x[:, :, :f, :f, :f] = float("-inf")
        want = _torch_pool(x, f)
        got = ops.maxpool_f(x.to(dev), f).cpu()
        assert _same(got, want), (shape, f)
        assert _same(got, _torch_pool(x.to(dev), f).cpu()), (shape, f)
        assert got.isnan().any() and (got == float("-inf")).any()


def test_maxpool_large_output(dev):
    from diffsci_amd import ops
    for f, shape in ((3, (4, 4, 2106, 2106)), (4, (2, 4, 4096, 4096))):        # 30.1 MiB and 32 MiB outputs
        x = torch.randn(shape, device=dev)
        got = ops.maxpool_f(x, f)
        assert got.numel() * 4 >= 30 << 20
        assert torch.equal(got, _torch_pool(x, f)), (f, shape)


def test_maxpool_refusals(dev):
    from diffsci_amd import ops
    with pytest.raises(ValueError, match="exceeds"):
        ops.maxpool_f(torch.zeros(1, 1, 4, 8, device=dev), 5)
    with pytest.raises(ValueError, match="exceeds"):
        ops.maxpool_f(torch.zeros(1, 1, 3, 8, 8, device=dev), 4)
    with pytest.raises(ValueError, match="out has shape"):
        ops.maxpool_f(torch.zeros(1, 1, 9, 9, device=dev), 3, out=torch.empty(1, 1, 3, 4, device=dev))


# ---------------------------------------------------------------- fp64 composition with the factor
def _punetg(sd, cfg, x, t, f, ye=None):
    """PUNetG.forward (punetg.py:389-416) with transition_scale_factor f: oracle.punetg_ref.punetg_forward with MaxPool(f) and
    nearest Upsample(f) in the Down / UpSamplers (commonlayers.py:25-165)."""
    nlev = len(cfg["channel_expansion"])
    ctype = cfg.get("convolution_type", "default")
    circ = "mp" if ctype == "mp" else ctype == "circular"
    norms = (cfg.get("first_resblock_norm", "GroupLN"), cfg.get("second_resblock_norm", "GroupRMS"))
    x = R.conv3x3(sd, "convin", x, circ)
    te = R.fourier_features(t, sd["time_projection.W"])
    if ye is not None:
        if ye.dim() > te.dim():
            te = te.reshape(list(te.shape) + [1] * (ye.dim() - te.dim()))
        te = te + ye
    skips = []
    for lv in range(nlev):
        for r in range(cfg["number_resnet_downward_block"]):
            x = R.resnet_block(sd, f"downward_blocks.{lv}.{r}.", x, te, circ, norms)
        skips.append(x)
        x = R.conv3x3(sd, f"downsamplers.{lv}.conv", _torch_pool(x, f), circ)
    for r in range(cfg["number_resnet_before_attn_block"]):
        x = R.resnet_block(sd, f"before_block.{r}.", x, te, circ, norms)
    xa = x
    nattn = cfg["number_resnet_attn_block"]
    for r in range(nattn):
        xa = R.resnet_block(sd, f"attn_resnet_block.{r}.", xa, te, circ, norms)
        if r < nattn - 1:
            if ctype == "mp":
                xa = R.mp_attention_2d(sd, f"attn_block.{r}.", xa, cfg["attn_residual"], True, False)
            else:
                xa = R.attention_2d(sd, f"attn_block.{r}.", xa, cfg["attn_residual"])
    x = x + xa
    for r in range(cfg["number_resnet_after_attn_block"]):
        x = R.resnet_block(sd, f"after_block.{r}.", x, te, circ, norms)
    for lv in range(nlev):
        x = F.interpolate(x, scale_factor=f, mode="nearest")
        x = R.conv3x3(sd, f"upsamplers.{lv}.conv", x, circ)
        x = x + skips.pop()
        for r in range(cfg["number_resnet_upward_block"]):
            x = R.resnet_block(sd, f"upward_blocks.{lv}.{r}.", x, te, circ, norms)
    return R.conv3x3(sd, "convout", x, circ)


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                            # non-trivial norm affines and biases
        for k, w in m.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                w.add_(0.1 * torch.randn(w.shape, generator=g))
    return m


def _net(M, f, seed, dim=2, mc=16, cls=None, **over):
    torch.manual_seed(seed)
    kw = dict(model_channels=mc, dimension=dim, transition_scale_factor=f)
    kw.update(over)
    cfg = M.PUNetGConfig(**kw)
    net = _perturb((cls or M.PUNetG)(cfg), seed + 1)
    d = R.default_config(model_channels=mc)
    d.update({k: v for k, v in cfg.export_description().items() if k in d or k in ("convolution_type", "transition_kernel_size")})
    return net, d


def _oracle(net, cfg, x, t, f, ye=None):
    sd = {k: w.detach().cpu().clone() for k, w in net.state_dict().items()}
    cast = (lambda v, dt: None if v is None else v.to(dt))
    want = _punetg({k: v.double() for k, v in sd.items()}, cfg, x.double(), t.double(), f, cast(ye, torch.float64))
    want32 = _punetg(sd, cfg, x.float(), t.float(), f, cast(ye, torch.float32))
    return want, max(4 * rel_l2(want32, want), 2e-6)


NET_CASES = {
    # tag: (f, (H, W), config overrides, precisions)
    "f3_54": (3, (54, 54), {}, ("fp16x3", "fp16x3-unfused", "bf16x6", "fp32")),
    "f3_54x81": (3, (54, 81), {}, ("fp16x3", "fp16x3-unfused", "bf16x6", "fp32")),
    "f4_64": (4, (64, 64), {}, ("fp16x3", "fp16x3-unfused", "bf16x6", "fp32")),
    "f1_16": (1, (16, 20), {}, ("fp16x3", "fp16x3-unfused", "bf16x6", "fp32")),
    "f3_circular": (3, (27, 36), dict(convolution_type="circular"), ("fp16x3", "fp16x3-unfused")),
    "f3_mp": (3, (27, 27), dict(convolution_type="mp"), ("fp16x3", "fp16x3-unfused", "fp32")),
    "f3_tks5": (3, (27, 27), dict(transition_kernel_size=5), ("fp16x3", "fp16x3-unfused")),
    "f4_tks7_circular": (4, (64, 64), dict(transition_kernel_size=7, convolution_type="circular"), ("fp16x3",)),
}


def _run(net, prec, x, t, y=None):
    net.conv_precision = "fp16x3" if prec.startswith("fp16x3") else prec
    net.fuse_norm = prec != "fp16x3-unfused"
    net.auto_precision = False
    return (net(x, t) if y is None else net(x, t, y)).cpu()


@pytest.mark.parametrize("tag", sorted(NET_CASES))
def test_network_2d_vs_fp64(M, dev, tag):
    f, (H, W), over, precs = NET_CASES[tag]
    net, cfg = _net(M, f, 30 + f, **over)
    g = torch.Generator().manual_seed(40 + f)
    x, t = torch.randn(2, 1, H, W, generator=g), torch.rand(2, generator=g)
    want, bound = _oracle(net, cfg, x, t, f)
    net = net.to(dev).eval()
    for prec in precs:
        got = _run(net, prec, x.to(dev), t.to(dev))
        err = rel_l2(got, want)
        print(f"[{tag} {prec}] HIP vs fp64 {err:.2e}, bound {bound:.2e}")
        assert got.shape == x.shape and err < bound, (tag, prec, err, bound)


def test_larger_kernels_keep_their_precision_refusals(M, dev):
    net, _ = _net(M, 3, 5, transition_kernel_size=5)
    net = net.to(dev).eval()
    net.conv_precision = "bf16x6"
    with pytest.raises(NotImplementedError, match="5x5 kernels are implemented on the fp16x3 convolution only"):
        net(torch.randn(1, 1, 27, 27, device=dev), torch.rand(1, device=dev))


@pytest.mark.parametrize("prec", ["fp16x3", "fp32"])
def test_network_3d_vs_fp64(M, dev, prec):
    f = 3
    net, cfg = _net(M, f, 60, dim=3, mc=8)
    g = torch.Generator().manual_seed(61)
    x, t = torch.randn(2, 1, 18, 18, 18, generator=g), torch.rand(2, generator=g)
    want, bound = _oracle(net, cfg, x, t, f)
    net = net.to(dev).eval()
    for p in ((prec, "fp16x3-unfused") if prec == "fp16x3" else (prec,)):
        got = _run(net, p, x.to(dev), t.to(dev))
        err = rel_l2(got, want)
        print(f"[3-D f={f} 18^3 {p}] HIP vs fp64 {err:.2e}, bound {bound:.2e}")
        assert got.shape == x.shape and err < bound


def test_field_condition_at_factor_three(M, dev):
    """A field-valued conditional embedding: every block corner-pools it to its own level (f^lv), as rescale_yt does."""
    f, H = 3, 27
    net, cfg = _net(M, f, 70)
    g = torch.Generator().manual_seed(71)
    x, t = torch.randn(2, 1, H, H, generator=g), torch.rand(2, generator=g)
    ye = torch.randn(2, 16, H, H, generator=g) * 0.5
    want, bound = _oracle(net, cfg, x, t, f, ye=ye)
    net = net.to(dev).eval()
    net.set_conditional_embedding(torch.nn.Identity())
    for prec in ("fp16x3", "fp16x3-unfused", "fp32"):
        got = _run(net, prec, x.to(dev), t.to(dev), ye.to(dev))
        err = rel_l2(got, want)
        print(f"[field condition f={f} {prec}] HIP vs fp64 {err:.2e}, bound {bound:.2e}")
        assert err < bound


def test_conditional_network_and_range_escalation(M, dev):
    """PUNetGCond at f = 3; an input channel 1e8 times larger moves the input layer to the exact-fp32 kernel, and the range
    guard's switch to bf16x6 keeps the factor's route."""
    f = 3
    torch.manual_seed(80)
    cfg = M.PUNetGConfig(model_channels=16, input_channels=2, transition_scale_factor=f)
    net = _perturb(M.nets.PUNetGCond(cfg, channel_conditional_items=["c"]), 81)
    with torch.no_grad():
        net.convin.weight[:, 1] *= 1e8
    d = R.default_config(model_channels=16, input_channels=2)
    g = torch.Generator().manual_seed(82)
    x, t, c = torch.randn(2, 1, 36, 36, generator=g), torch.rand(2, generator=g), torch.randn(2, 1, 36, 36, generator=g) * 1e-8
    want, bound = _oracle(net, d, torch.cat([x, c], dim=1), t, f)
    net = net.to(dev).eval()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = net(x.to(dev), t.to(dev), {"c": c.to(dev)}).cpu()
    assert net.exact_input_layer and any("exact-fp32" in str(r.message) for r in rec)
    assert rel_l2(got, want) < bound, rel_l2(got, want)
    from diffsci_amd.models.nets import precision
    with pytest.warns(RuntimeWarning, match="fp16x3 convolution range"):
        precision.escalate(net)
    assert net.conv_precision == "bf16x6"
    got = net(x.to(dev), t.to(dev), {"c": c.to(dev)}).cpu()
    assert rel_l2(got, want) < bound, rel_l2(got, want)


def test_stages_compose_to_forward(M, dev):
    f = 3
    net, _ = _net(M, f, 90)
    net = net.to(dev).eval()
    net.fuse_norm = False                  # the stage methods run the standalone norms: compare like with like
    g = torch.Generator().manual_seed(91)
    x, t = torch.randn(2, 1, 54, 54, generator=g).to(dev), torch.rand(2, generator=g).to(dev)
    te = net.embed_time(t)
    with torch.no_grad():
        h = net._conv(net.convin, x, net.packed_weights())
        h, skips = net.encode(h, te)
        assert h.shape[-2:] == (6, 6) and [s.shape[-1] for s in skips] == [54, 18]
        h = net.bottom_forward(h, te)
        h = net.decode(h, te, skips)
        staged = net._out_conv(net.convout, h, net.packed_weights(), None, net.circular)
        full = net(x, t)
    err = rel_l2(staged.cpu(), full.cpu())
    print(f"[stages f={f}] encode -> bottom_forward -> decode vs forward {err:.2e}")
    assert staged.shape == full.shape and err < 1e-5


def test_captured_sampling_is_eager_bit_for_bit(M, dev):
    net, _ = _net(M, 4, 100, mc=8)
    module = M.KarrasModule(net.to(dev).eval(), M.KarrasModuleConfig.from_edm())
    wn = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(101)).to(dev)     # 64 -> 16 -> 4
    module.use_graph = False
    eager = module.propagate_white_noise(wn, nsteps=3).cpu()
    module.use_graph = True
    a = module.propagate_white_noise(wn, nsteps=3).cpu()
    b = module.propagate_white_noise(wn, nsteps=3).cpu()
    assert torch.isfinite(eager).all()
    print(f"[captured f=4] bit-identical: {torch.equal(a, eager)}, rel {rel_l2(a, eager):.2e}")
    assert torch.equal(a, eager) and torch.equal(a, b)


def test_factor_two_unchanged_next_to_another_factor(M, dev):
    n2, cfg = _net(M, 2, 110)
    n3 = M.PUNetG(M.PUNetGConfig(model_channels=16, transition_scale_factor=3))
    n3.load_state_dict(n2.state_dict())
    n2, n3 = n2.to(dev).eval(), n3.to(dev).eval()
    g = torch.Generator().manual_seed(111)
    x, t = torch.randn(2, 1, 36, 36, generator=g), torch.rand(2, generator=g)
    before = n2(x.to(dev), t.to(dev)).clone()
    assert n3(x.to(dev), t.to(dev)).shape == x.shape                 # 36 -> 12 -> 4
    assert torch.equal(n2(x.to(dev), t.to(dev)), before)
    want = R.punetg_forward({k: v.double().cpu() for k, v in n2.state_dict().items()}, cfg, x.double(), t.double())
    assert rel_l2(before.cpu(), want) < 1e-5


def test_divisibility_is_refused_before_any_launch(M, dev, monkeypatch):
    from diffsci_amd import _native as N
    net, _ = _net(M, 3, 120)
    net = net.to(dev).eval()
    vol, _ = _net(M, 4, 121, dim=3, mc=8)
    vol = vol.to(dev).eval()
    cond = M.nets.PUNetGCond(M.PUNetGConfig(model_channels=8, input_channels=2, transition_scale_factor=3),
                             channel_conditional_items=["c"]).to(dev).eval()
    real, calls = N.lib, []
    monkeypatch.setattr(N, "lib", lambda: calls.append(1) or real())
    t = torch.rand(1, device=dev)
    with pytest.raises(ValueError, match=r"transition_scale_factor \*\* 2 = 9"):
        net(torch.randn(1, 1, 27, 30, device=dev), t)
    with pytest.raises(ValueError, match=r"\*\* 2 = 16"):
        vol(torch.randn(1, 1, 16, 16, 24, device=dev), t)
    with pytest.raises(ValueError, match="divide"):
        cond(torch.randn(1, 1, 18, 20, device=dev), t, {"c": torch.randn(1, 1, 18, 20, device=dev)})
    assert not calls
    monkeypatch.undo()
    assert net(torch.randn(1, 1, 27, 27, device=dev), t).shape == (1, 1, 27, 27)
