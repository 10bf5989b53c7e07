"""ADM resampling by any integer factor on a real MI355X: the resampling kernels against torch, the ADM blocks (2-D and 3-D)
and the whole ADM against an fp64 torch composition with the factor, eager vs captured sampling, and factor 2 unchanged
next to another factor.

Bounds: nearest upsampling is a copy, so it is bit-identical to torch.nn.Upsample; pooling stays within 2x torch fp32's own
error against fp64; blocks and networks within max(4 x torch-fp32-vs-fp64, 2e-6) as tests/test_gpu_adm.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import adm_ref  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


# ---------------------------------------------------------------- kernels
UP_SHAPES = [(2, 3, 5, 7), (1, 4, 8, 8), (3, 2, 1, 1), (2, 3, 3, 5, 7), (1, 2, 4, 4, 4)]


@pytest.mark.parametrize("f", [1, 3, 4, 5, 7])
def test_upsample_is_torch_nearest_bit_for_bit(dev, f):
    from diffsci_amd import ops
    g = torch.Generator().manual_seed(f)
    for shape in UP_SHAPES:
        x = torch.randn(shape, generator=g)
        want = torch.nn.Upsample(scale_factor=f, mode="nearest")(x)
        got = ops.upsample_f(x.to(dev), f).cpu()
        assert got.shape == want.shape and torch.equal(got, want), (shape, f)
        # torch's own GPU kernel as well
        assert torch.equal(got, torch.nn.Upsample(scale_factor=f, mode="nearest")(x.to(dev)).cpu())


def test_upsample_large_plane(dev):
    from diffsci_amd import ops
    for f, shape in ((4, (1, 1, 1024, 1024)), (3, (2, 1, 700, 701))):           # 64 MiB and 35 MiB outputs
        x = torch.randn(shape, device=dev)
        got = ops.upsample_f(x, f)
        assert got.numel() * 4 >= 30 << 20
        assert torch.equal(got, torch.nn.Upsample(scale_factor=f, mode="nearest")(x)), (f, shape)


POOL_SHAPES_2D = [(2, 3, 12, 12), (2, 3, 13, 14), (1, 5, 25, 31), (2, 2, 64, 64)]
POOL_SHAPES_3D = [(2, 3, 12, 12, 12), (1, 2, 13, 9, 14), (1, 2, 8, 16, 20)]


@pytest.mark.parametrize("f", [1, 3, 4])
def test_pooling_vs_fp64(dev, f):
    from diffsci_amd import ops
    g = torch.Generator().manual_seed(10 + f)
    for shape in POOL_SHAPES_2D + POOL_SHAPES_3D:
        x = torch.randn(shape, generator=g) * 2 + 0.3
        pool = F.avg_pool2d if x.dim() == 4 else F.avg_pool3d
        want = pool(x.double(), f)
        ref = pool(x.to(dev), f).cpu()
        got = ops.avgpool_f(x.to(dev), f).cpu()
        assert got.shape == want.shape, (shape, f)
        ref_err, err = rel_l2(ref, want), rel_l2(got, want)
        assert err <= max(2 * ref_err, 1e-12), (shape, f, err, ref_err)


@pytest.mark.parametrize("f", [1, 3, 4])
def test_norm_silu_pool_vs_fp64(dev, f):
    from diffsci_amd import ops
    g = torch.Generator().manual_seed(20 + f)
    for (B, C, H, W) in [(2, 8, 24, 24), (3, 5, 13, 14), (2, 16, 64, 64)]:
        x = torch.randn(B, C, H, W, generator=g) * 3 + 0.7
        w, b, film = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, 2 * C, generator=g)
        xd = x.to(dev)
        for kind in (0, 1):
            st = ops.gnorm1_stats(xd, kind)
            n = (F.group_norm(x.double(), 1, w.double(), b.double(), 1e-5) if kind == 0
                 else adm_ref.group1_rms_norm(x.double(), w.double(), b.double()))
            for fl in (None, film, film[:1].contiguous()):
                v = n if fl is None else n * fl[:, :C, None, None].double() + fl[:, C:, None, None].double()
                want = F.avg_pool2d(F.silu(v), f)
                got = ops.gnorm1_apply_poolf(xd, st, w.to(dev), b.to(dev), kind, f,
                                             film=None if fl is None else fl.to(dev)).cpu()
                assert got.shape == want.shape
                assert rel_l2(got, want) < 5e-7, ((B, C, H, W), f, kind, fl is None)


# ---------------------------------------------------------------- fp64 compositions with the factor
def _norm(kind, x, w, b):
    if kind == "GroupLN":
        return F.group_norm(x, 1, w, b, 1e-5)
    return adm_ref.group1_rms_norm(x, w, b)


def _resample(v, sample, f):
    if sample == "down":
        return (F.avg_pool3d if v.dim() == 5 else F.avg_pool2d)(v, f)
    if sample == "up":
        return F.interpolate(v, scale_factor=f, mode="nearest")
    return v


def _attention(sd, p, y, heads, residual=True):
    B, C = y.shape[:2]
    mh = torch.nn.MultiheadAttention(C, num_heads=heads, batch_first=True).to(y.dtype)
    mh.load_state_dict({k[len(p + "attn.mhattn."):]: v for k, v in sd.items() if k.startswith(p + "attn.mhattn.")})
    t = y.reshape(B, C, -1).transpose(1, 2)
    with torch.no_grad():
        a, _ = mh(t, t, t, need_weights=False)
    a = a.transpose(1, 2).reshape(y.shape)
    return y + a if residual else a


def _block(sd, p, x, te, sample, f, kinds=("GroupLN", "GroupRMS"), skip=None, residual=True, heads=0):
    """ADMBaseBlock.forward (adm.py:292-349) with image_sample_factor f: norm1 -> SiLU -> resample -> conv1 -> norm2 -> FiLM
    -> SiLU -> conv2 (+ convresidual(resample(x))) (-> attention with `heads` heads)."""
    if skip is not None:
        x = torch.cat([x, skip], dim=1)
    conv = F.conv3d if x.dim() == 5 else F.conv2d
    y = F.silu(_norm(kinds[0], x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]))
    y = conv(_resample(y, sample, f), sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1)
    y = _norm(kinds[1], y, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    te1, te2 = torch.chunk(F.linear(te, sd[p + "embed_linear.weight"], sd[p + "embed_linear.bias"]), 2, dim=-1)
    one = (1,) * (y.dim() - 2)
    y = conv(F.silu(y * te1.view(*te1.shape, *one) + te2.view(*te2.shape, *one)), sd[p + "conv2.weight"], sd[p + "conv2.bias"],
             padding=1)
    if residual:
        y = y + conv(_resample(x, sample, f), sd[p + "convresidual.weight"], sd[p + "convresidual.bias"])
    if heads:
        y = _attention(sd, p, y, heads)
    return y


def _adm(sd, cfg, x, t, f):
    """ADM.forward (adm.py:199-216) with transition_scale_factor f, decoder_type 1, concat skips."""
    nl = len(cfg.channel_expansion)
    te = adm_ref.time_embedding(sd, t)
    x = F.conv2d(x, sd["input_layer.weight"], sd["input_layer.bias"], padding="same")
    skips = [x]
    for i in range(nl):
        nb = cfg.number_resnet_downward_block
        for j in range(nb):
            x = _block(sd, f"encoder.layers.{i}.input_blocks.{j}.", x, te, "down" if j == nb - 1 else None, f)
        skips.append(x)
    for j, a in enumerate(cfg.middle_block_attn_config):
        x = _block(sd, f"middle_block.middle_blocks.{j}.", x, te, None, f, heads=1 if a else 0)
    for i in range(nl):
        x = torch.cat([x, skips.pop()], dim=1)
        nb = cfg.number_resnet_upward_block
        for j in range(nb):
            x = _block(sd, f"decoder.layers.{i}.input_blocks.{j}.", x, te, "up" if j == nb - 1 else None, f)
    return F.conv2d(x, sd["output_layer.weight"], sd["output_layer.bias"], padding="same")


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                            # non-trivial norm affines and biases
        for k, w in m.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                w.add_(0.1 * torch.randn(w.shape, generator=g))
    return m


# ---------------------------------------------------------------- blocks
BLOCK_CASES = {
    # tag: (class, kwargs, x shape, skip shape or None)
    "enc2d_f3": ("ADMEncoderBlock", dict(has_downsample=True, downsample_factor=3), (2, 16, 25, 25), None),
    "enc2d_f4": ("ADMEncoderBlock", dict(has_downsample=True, downsample_factor=4), (2, 16, 32, 32), None),
    "dec2d_f3": ("ADMDecoderBlock", dict(has_upsample=True, upsample_factor=3, channels_skip=8), (2, 16, 8, 8), (2, 8, 8, 8)),
    "dec2d_f4": ("ADMDecoderBlock", dict(has_upsample=True, upsample_factor=4, channels_skip=8), (2, 16, 6, 7), (2, 8, 6, 7)),
    "enc3d_f3": ("ADMEncoderBlock", dict(has_downsample=True, downsample_factor=3, dimension=3), (2, 16, 12, 12, 13), None),
    "enc3d_f4": ("ADMEncoderBlock", dict(has_downsample=True, downsample_factor=4, dimension=3), (2, 16, 12, 12, 12), None),
    "dec3d_f3": ("ADMDecoderBlock", dict(has_upsample=True, upsample_factor=3, channels_skip=8, dimension=3),
                 (2, 16, 3, 3, 3), (2, 8, 3, 3, 3)),
    "dec3d_f4": ("ADMDecoderBlock", dict(has_upsample=True, upsample_factor=4, channels_skip=8, dimension=3,
                                         first_norm="GroupRMS", second_norm="GroupLN"), (2, 16, 2, 3, 2), (2, 8, 2, 3, 2)),
}


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("tag", sorted(BLOCK_CASES))
def test_blocks_vs_fp64(M, dev, tag, precision):
    cls, kw, xs, ss = BLOCK_CASES[tag]
    torch.manual_seed(7)
    blk = _perturb(getattr(M.nets, cls)(16, 32, 24, has_residual=True, has_attn=True, attn_heads=2, **kw), 8)
    sd = {k: w.detach().clone() for k, w in blk.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    x, te = torch.randn(xs, generator=g), torch.randn(2, 24, generator=g)
    skip = torch.randn(ss, generator=g) if ss else None
    blk = blk.to(dev).eval()
    blk.conv_precision = precision
    got = blk(*([x.to(dev), te.to(dev)] + ([skip.to(dev)] if skip is not None else []))).cpu()
    sample = "down" if kw.get("has_downsample") else "up"
    f = kw.get("downsample_factor", kw.get("upsample_factor"))
    kinds = (kw.get("first_norm", "GroupLN"), kw.get("second_norm", "GroupRMS"))

    def ref(dt):
        s = {k: v.to(dt) for k, v in sd.items()}
        return _block(s, "", x.to(dt), te.to(dt), sample, f, kinds, None if skip is None else skip.to(dt), heads=2)
    want, want32 = ref(torch.float64), ref(torch.float32)
    assert got.shape == want.shape
    err, ref_err = rel_l2(got, want), rel_l2(want32, want)
    print(f"[{tag} {precision}] HIP vs fp64 {err:.2e}, torch fp32 vs fp64 {ref_err:.2e}")
    assert err < max(4 * ref_err, 2e-6)


def test_factor_two_unchanged_next_to_another_factor(M, dev):
    """Factor 2 keeps its route: the same output, bit for bit, before and after a factor-3 block ran in the process."""
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(12)
    x, skip, te = torch.randn(2, 16, 8, 8, generator=g), torch.randn(2, 8, 8, 8, generator=g), torch.randn(2, 24, generator=g)
    kw = dict(channels_skip=8, has_upsample=True, has_residual=True, has_attn=True, attn_heads=2)
    b2 = _perturb(M.nets.ADMDecoderBlock(16, 32, 24, **kw), 13).to(dev).eval()
    b3 = M.nets.ADMDecoderBlock(16, 32, 24, upsample_factor=3, **kw).to(dev).eval()
    b3.load_state_dict(b2.state_dict())
    e2 = M.nets.ADMEncoderBlock(16, 32, 24, has_downsample=True, has_residual=True).to(dev).eval()
    e3 = M.nets.ADMEncoderBlock(16, 32, 24, has_downsample=True, has_residual=True, downsample_factor=3).to(dev).eval()
    e3.load_state_dict(e2.state_dict())
    args = (x.to(dev), te.to(dev), skip.to(dev))
    before, before_e = b2(*args).clone(), e2(x.to(dev), te.to(dev)).clone()
    assert b3(*args).shape[-1] == 24 and e3(x.to(dev), te.to(dev)).shape[-1] == 2
    assert torch.equal(b2(*args), before) and torch.equal(e2(x.to(dev), te.to(dev)), before_e)
    # and the f = 2 result is the fp64 composition's, as before
    sd = {k: v.double().cpu() for k, v in b2.state_dict().items()}
    want = _block(sd, "", x.double(), te.double(), "up", 2, skip=skip.double(), heads=2)
    assert rel_l2(before.cpu(), want) < 1e-5


# ---------------------------------------------------------------- the whole network
def _small_adm(M, f, seed):
    torch.manual_seed(seed)
    cfg = M.ADMConfig(model_channels=8, time_embed_dim=8, output_embed_dim=16, transition_scale_factor=f)
    return _perturb(M.ADM(cfg), seed + 1), cfg


@pytest.mark.parametrize("f,size", [(3, 54), (4, 64)])
def test_adm_network_vs_fp64(M, dev, f, size):
    net, cfg = _small_adm(M, f, 30 + f)
    sd = {k: w.detach().clone() for k, w in net.state_dict().items()}
    g = torch.Generator().manual_seed(40 + f)
    x, t = torch.randn(2, 1, size, size, generator=g), torch.rand(2, generator=g)
    net = net.to(dev)
    want = _adm({k: v.double() for k, v in sd.items()}, cfg, x.double(), t.double(), f)
    want32 = _adm(sd, cfg, x, t, f)
    bound = max(4 * rel_l2(want32, want), 2e-6)
    for fuse in (True, False):
        net.fuse_norm = fuse
        got = net(x.to(dev), t.to(dev)).cpu()
        assert got.shape == x.shape
        err = rel_l2(got, want)
        print(f"[ADM f={f} {size}^2 fuse={fuse}] HIP vs fp64 {err:.2e}, bound {bound:.2e}")
        assert err < bound
    with pytest.raises(ValueError, match="divide"):
        net(torch.randn(2, 1, size + f, size + f, device=dev), t.to(dev))


def test_adm_captured_sampling_factor_four(M, dev):
    net, _ = _small_adm(M, 4, 50)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).to(dev)
    wn = torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(51)).to(dev)    # 32 -> 8 -> 2
    module.use_graph = False
    eager = module.propagate_white_noise(wn, nsteps=4).cpu()
    module.use_graph = True
    a = module.propagate_white_noise(wn, nsteps=4).cpu()
    b = module.propagate_white_noise(wn, nsteps=4).cpu()
    assert torch.isfinite(eager).all()
    print(f"[captured f=4] bit-identical: {torch.equal(a, eager)}, rel {rel_l2(a, eager):.2e}")
    assert rel_l2(a, eager) < 1e-5 and torch.equal(a, b)
