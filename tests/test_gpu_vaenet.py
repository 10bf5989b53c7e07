"""VAENet first stage on a real MI355X: the stride-2 convolution kernels of ds_conv_s2.hip and the posterior draw against torch on
the CPU in fp64 and fp32, the blocks against the restatement tests/vaenet_ref.py, the networks against the fixtures the
reference produced (tests/golden/vaenet_*.npz) on both norm routes, and a latent KarrasModule that encodes and decodes through it.

Bounds.  Convolutions, blocks, networks: rel-L2 < 1e-5 against the fp32 reference and, against fp64, within max(4 x the
reference's own fp32-vs-fp64 distance, 2e-6) -- the referee rule of tests/test_gpu_ldm_decoder.py.  Two routes of one arithmetic
(the stride-2 launch against stride-1 + subsampling; folded against standalone norms): rel-L2 < 2e-6.  Elementwise kernel
(posterior draw): rel-L2 < 5e-7 against fp64.  In-kernel noise: mean and variance of 2^18 recovered normals within 5 standard
errors (1/sqrt(n), sqrt(2/n)) of 0 and 1.  The stride-2 matrix-core kernel's tile is 8 rows x 32 columns of the output."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import vaenet_ref  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

REL = 1e-5
TILE = (8, 32)                 # output rows x columns of one workgroup of ds_conv2d_s2_h3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = vaenet_ref.load_golden(tag)
        return cache[tag]
    return get


def referee(got, want32, want64, what=""):
    e32, e64, ref = rel_l2(got, want32), rel_l2(got, want64), rel_l2(want32, want64)
    print(f"{what}: vs fp32 {e32:.2e}; vs fp64 {e64:.2e}; reference fp32 vs fp64 {ref:.2e}")
    assert e32 < REL, (what, e32)
    assert e64 < max(4 * ref, 2e-6), (what, e64, ref)


def conv_ref(x, w, b):
    d = x.dim() - 2
    fn = F.conv3d if d == 3 else F.conv2d
    return (fn(F.pad(x, (0, 1) * d), w, b, stride=2), fn(F.pad(x.double(), (0, 1) * d), w.double(), b.double(), stride=2))


# (B, Cin, Cout, spatial)
FIELDS = [
    (2, 32, 32, (2, 2)),          # output 1 x 1: every tap but one row and one column lies in the pad
    (3, 64, 64, (7, 9)),          # odd sides
    (1, 96, 96, (8, 8)),          # six 16-channel chunks, two channel tiles
    (2, 32, 48, (24, 40)),        # Cin != Cout; 12 x 20 outputs: two tiles, the second ragged
    (1, 1, 32, (16, 16)),         # thin input
    (1, 32, 3, (16, 16)),         # thin output
    (1, 32, 32, (38, 145)),       # 19 x 72 outputs against the 8 x 32 tile: 3 x 3 tiles, ragged in both axes; an odd input width
    (1, 16, 16, (22, 75)),        # 11 x 37 outputs: a width that is no multiple of 4 (the epilogue's element-wise path), two column tiles
]
VOLUMES = [
    (1, 32, 32, (2, 2, 2)),
    (2, 32, 32, (7, 10, 12)),
    (1, 64, 64, (8, 8, 8)),
]


def _case(shape, seed):
    B, Cin, Cout, sp = shape
    torch.manual_seed(seed)
    x = torch.randn(B, Cin, *sp) * 1.5 + 0.3
    w = torch.randn(Cout, Cin, *(3,) * len(sp)) / (3 ** (len(sp) / 2) * Cin ** 0.5)
    b = torch.randn(Cout)
    return x, w, b


@pytest.mark.parametrize("form", ["fp16x3", "fp32"])
@pytest.mark.parametrize("case", range(len(FIELDS)))
def test_stride2_fields_against_fp64(dev, case, form):
    from diffsci_amd import ops
    x, w, b = _case(FIELDS[case], 200 + case)
    w32, w64 = conv_ref(x, w, b)
    assert TILE == (8, 32)
    # the matrix-core kernel on every shape, thin ones included (pack_conv_s2 would route those to the exact kernel)
    pk = ops.pack_conv(w.to(dev), "fp16x3") if form == "fp16x3" else ops.pack_conv_s2(w.to(dev), "fp32")
    assert pk.kind == ("fp16x3" if form == "fp16x3" else "direct")
    am = ops.amax_new(x.shape[0], dev)
    got = ops.conv_s2(x.to(dev), pk, bias=b.to(dev), out_amax=am)
    assert tuple(got.shape) == tuple(w32.shape) and bool(torch.isfinite(got).all())
    referee(got.cpu(), w32, w64, f"conv_s2 {form} {FIELDS[case]}")
    assert torch.equal(am.view(torch.float32), got.reshape(x.shape[0], -1).abs().amax(1))     # out_amax = a pass over the output
    res = torch.randn_like(w32)
    got2 = ops.conv_s2(x.to(dev), pk, bias=b.to(dev), res1=res.to(dev))
    assert torch.equal(got2, got + res.to(dev))                                               # res1: one rounded addition
    if form == "fp16x3":
        routed = ops.pack_conv_s2(w.to(dev), "fp16x3")
        assert routed.kind == ("fp16x3" if min(w.shape[:2]) > 4 else "direct")


@pytest.mark.parametrize("form", ["fp16x3", "fp32"])
@pytest.mark.parametrize("case", range(len(VOLUMES)))
def test_stride2_volumes_against_fp64(dev, case, form):
    from diffsci_amd import ops
    x, w, b = _case(VOLUMES[case], 300 + case)
    w32, w64 = conv_ref(x, w, b)
    packs = ops.pack_conv3d_s2(w.to(dev), form)
    assert isinstance(packs, list) == (form == "fp16x3")
    got = ops.conv3d_s2(x.to(dev), packs, bias=b.to(dev))
    assert tuple(got.shape) == tuple(w32.shape)
    referee(got.cpu(), w32, w64, f"conv3d_s2 {form} {VOLUMES[case]}")
    res = torch.randn_like(w32).to(dev)
    assert torch.equal(ops.conv3d_s2(x.to(dev), packs, bias=b.to(dev), res1=res), got + res)


def test_stride2_thin_volume_layers_take_the_exact_kernel(dev):
    from diffsci_amd import ops
    for shape in ((1, 1, 32, (6, 7, 8)), (1, 32, 3, (6, 7, 8))):
        x, w, b = _case(shape, 320)
        packs = ops.pack_conv3d_s2(w.to(dev), "fp16x3")
        assert not isinstance(packs, list) and packs.kind == "direct"
        referee(ops.conv3d_s2(x.to(dev), packs, bias=b.to(dev)).cpu(), *conv_ref(x, w, b), f"conv3d_s2 thin {shape}")


def test_stride2_per_sample_magnitudes(dev):
    """Samples scaled by 2^-10, 1 and 2^10 in one batch: the per-sample activation exponent holds the bound for each of them."""
    from diffsci_amd import ops
    x, w, b = _case((3, 64, 64, (12, 20)), 340)
    x = x * torch.tensor([2.0 ** -10, 1.0, 2.0 ** 10]).view(3, 1, 1, 1)
    b = torch.zeros_like(b)                                    # a bias of order one would hide the small sample's error
    w32, w64 = conv_ref(x, w, b)
    got = ops.conv_s2(x.to(dev), ops.pack_conv(w.to(dev), "fp16x3"), bias=b.to(dev)).cpu()
    for i in range(3):
        referee(got[i], w32[i], w64[i], f"conv_s2 fp16x3 sample scaled by 2^{(-10, 0, 10)[i]}")
    am = ops.absmax_rows(x.to(dev))
    assert torch.equal(ops.conv_s2(x.to(dev), ops.pack_conv(w.to(dev), "fp16x3"), bias=b.to(dev), in_amax=am).cpu(), got)


@pytest.mark.parametrize("shape", [(2, 32, 48, (24, 40)), (3, 64, 64, (7, 9)), (1, 32, 32, (38, 145))])
def test_stride2_agrees_with_stride1_then_subsample(dev, shape):
    """The route the package had before: the stride-1 'same' convolution of the input zero-padded by one row and column at the
    far end, of which the stride-2 result is every second output starting at (1, 1) (the phase at which a 'same' window
    covers rows 2i .. 2i+2)."""
    from diffsci_amd import ops
    x, w, b = _case(shape, 360)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    got = ops.conv_s2(xd, ops.pack_conv(wd, "fp16x3"), bias=bd)
    full = ops.conv(F.pad(xd, (0, 1, 0, 1)), ops.pack_conv(wd, "fp16x3"), bias=bd)
    want = full[..., 1::2, 1::2][..., :got.shape[2], :got.shape[3]]
    err = rel_l2(got.cpu(), want.cpu())
    print(f"stride-2 launch vs stride-1 + subsample {shape}: {err:.2e}")
    assert err < 2e-6


def test_stride2_refuses_small_sides(dev):
    from diffsci_amd import ops
    pk = ops.pack_conv_s2(torch.randn(8, 8, 3, 3, device=dev), "fp16x3")
    with pytest.raises(ValueError, match="at least 2"):
        ops.conv_s2(torch.zeros(1, 8, 1, 8, device=dev), pk)
    with pytest.raises(ValueError, match="at least 2"):
        ops.conv3d_s2(torch.zeros(1, 8, 4, 4, 1, device=dev), ops.pack_conv3d_s2(torch.randn(8, 8, 3, 3, 3, device=dev)))


# ---- posterior draw ------------------------------------------------------------------------------------------------------------
POSTERIOR_SHAPES = [(2, 6, 5, 7), (1, 8, 3, 4, 5), (3, 2, 3, 3)]        # the last: 27 elements of z, no multiple of 4


@pytest.mark.parametrize("shape", POSTERIOR_SHAPES)
@pytest.mark.parametrize("clamp", [None, (-30.0, 20.0)])
def test_posterior_with_given_noise(dev, shape, clamp):
    from diffsci_amd import ops
    torch.manual_seed(400)
    m = torch.randn(*shape)
    Z = shape[1] // 2
    m[:, Z:] *= 4
    m[0, Z].flatten()[:3] = torch.tensor([-45.0, 31.0, 20.5])[:m[0, Z].numel()]          # logvar outside (-30, 20)
    eps = torch.randn(shape[0], Z, *shape[2:])
    want = vaenet_ref.posterior(m.double(), eps.double(), clamp)
    got = ops.posterior_sample(m.to(dev), eps.to(dev), clamp=clamp)
    assert tuple(got.shape) == tuple(want.shape)
    err = rel_l2(got.cpu(), want)
    print(f"posterior {shape} clamp={clamp}: {err:.2e}")
    assert err < 5e-7
    out = torch.empty_like(got)
    assert ops.posterior_sample(m.to(dev), eps.to(dev), clamp=clamp, out=out) is out and torch.equal(out, got)


def _recovered(z, m):
    mean, logvar = m.double().chunk(2, dim=1)
    return ((z.double() - mean) / torch.exp(0.5 * logvar)).flatten()


def _check_normal(e, what):
    n = e.numel()
    mu, var = float(e.mean()), float(e.var(unbiased=False))
    print(f"{what}: n = {n}, mean {mu:+.2e} (5 s.e. = {5 / n ** 0.5:.2e}), variance - 1 {var - 1:+.2e} (5 s.e. = {5 * (2 / n) ** 0.5:.2e})")
    assert abs(mu) < 5 / n ** 0.5 and abs(var - 1) < 5 * (2 / n) ** 0.5


def test_posterior_in_kernel_noise(dev):
    from diffsci_amd import ops
    torch.manual_seed(401)
    m = torch.randn(4, 32, 64, 64, device=dev)                 # z: 2^18 elements
    m[:, 16:] *= 0.5                                           # std in a range where fp32 recovers eps to ~1e-6
    torch.manual_seed(5)
    off0 = torch.cuda.default_generators[dev.index].get_offset()
    a = ops.posterior_sample(m)
    assert torch.cuda.default_generators[dev.index].get_offset() > off0            # the device generator advances
    b = ops.posterior_sample(m)
    torch.manual_seed(5)
    a2 = ops.posterior_sample(m)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    e = _recovered(a.cpu(), m.cpu())
    _check_normal(e, "in-kernel noise")
    # the draw is ds_philox_normal's stream: element e of z <- counter offset + e/4
    state = torch.tensor([5, off0], dtype=torch.int64, device=dev)
    eps = ops.philox_normal(state, 0, a.shape)
    assert torch.equal(ops.posterior_sample(m, eps), a)
    for shape in POSTERIOR_SHAPES:                             # ragged counts: every element drawn, none twice
        mm = torch.zeros(*shape, device=dev)
        torch.manual_seed(6)
        z = ops.posterior_sample(mm).flatten()                 # mean 0, std 1: z is the noise itself
        assert bool(torch.isfinite(z).all()) and z.unique().numel() == z.numel()


def test_posterior_in_kernel_noise_under_graph_capture(dev):
    from diffsci_amd import ops
    torch.manual_seed(402)
    m = torch.randn(4, 32, 64, 64, device=dev) * 0.5
    ops.posterior_sample(m)                                    # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        z = ops.posterior_sample(m)
    g.replay()
    torch.cuda.synchronize()
    z1 = z.clone()
    g.replay()
    torch.cuda.synchronize()
    z2 = z.clone()
    _check_normal(_recovered(z1.cpu(), m.cpu()), "captured draw, first replay")
    _check_normal(_recovered(z2.cpu(), m.cpu()), "captured draw, second replay")
    assert not torch.equal(z1, z2)                             # every replay draws fresh noise


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def _perturb(blk):
    with torch.no_grad():
        for k, v in blk.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                v.add_(0.25 * torch.randn_like(v))


def _pair(fn, x, sd, **kw):
    with torch.inference_mode():
        return fn(x, sd, **kw), fn(x.double(), {k: v.double() for k, v in sd.items()}, **kw)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("with_conv", [True, False])
@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_downsample_against_the_restatement(dev, dim, with_conv, precision):
    from diffsci_amd.models.nets import vaenet as vn
    torch.manual_seed(500 + dim)
    blk = vn.Downsample(dim, 32, with_conv)
    _perturb(blk)
    sp = (15, 22) if dim == 2 else (6, 7, 10)
    if not with_conv:
        sp = tuple(s + s % 2 for s in sp)
    x = torch.randn(2, 32, *sp) * 1.5 + 0.3
    w32, w64 = _pair(vaenet_ref.downsample, x, blk.state_dict())
    blk.conv_precision = precision
    got = blk.to(dev)(x.to(dev)).cpu()
    assert got.shape == w32.shape
    referee(got, w32, w64, f"Downsample dim={dim} with_conv={with_conv} {precision}")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", ["res", "attn"])
def test_blocks_with_eight_groups(dev, dim, kind):
    from diffsci_amd.models.nets import vaenet as vn
    torch.manual_seed(520 + dim)
    sp = (16, 24) if dim == 2 else (4, 6, 8)
    if kind == "res":
        blk, fn = vn.ResnetBlock(dimension=dim, in_channels=24, out_channels=48, dropout=0.0, num_groups=8), vaenet_ref.resnet_block
    else:
        blk, fn = vn.AttnBlock(dim, 24, num_groups=8), vaenet_ref.attn_block
    _perturb(blk)
    x = torch.randn(2, 24, *sp) * 1.5 + 0.3
    w32, w64 = _pair(fn, x, blk.state_dict(), G=8)
    with torch.inference_mode():
        assert rel_l2(fn(x, blk.state_dict(), G=4), w32) > 1e-3            # the group count matters on this input
    blk = blk.to(dev)
    outs = {}
    for fuse in (True, False):
        blk.fuse_norm = fuse
        outs[fuse] = blk(x.to(dev)).cpu()
        referee(outs[fuse], w32, w64, f"{kind} dim={dim} num_groups=8 fuse_norm={fuse}")
    assert rel_l2(outs[True], outs[False]) < 2e-6


# ---- networks ------------------------------------------------------------------------------------------------------------------
def _net(dev, golden, tag):
    v, sd, info = golden(tag)
    net = vaenet_ref.build(info)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).eval(), v


@pytest.mark.parametrize("tag", ["a", "a2", "b", "c", "c2"])
def test_networks_against_the_reference_on_both_norm_routes(dev, golden, tag):
    net, v = _net(dev, golden, tag)
    x, eps = v["x"].to(dev), v["eps"].to(dev)
    outs = {}
    for fuse in (True, False):
        net.fuse_norm = fuse
        m = net.encode(x, sample=False)
        z = net.encode(x, eps=eps)
        referee(m.cpu(), v["moments_f32"], v["moments_f64"], f"vaenet_{tag} moments fuse_norm={fuse}")
        referee(z.cpu(), v["z_f32"], v["z_f64"], f"vaenet_{tag} sampled z fuse_norm={fuse}")
        outs[fuse] = [m.cpu(), z.cpu()]
        if "zin" in v:
            o = net.decode(v["zin"].to(dev))
            referee(o.cpu(), v["dec_f32"], v["dec_f64"], f"vaenet_{tag} decode fuse_norm={fuse}")
            outs[fuse].append(o.cpu())
    for a, b in zip(outs[True], outs[False]):
        assert rel_l2(a, b) < 2e-6


def test_network_exact_fp32_convolutions(dev, golden):
    net, v = _net(dev, golden, "a")
    net.conv_precision = "fp32"
    referee(net.encode(v["x"].to(dev), sample=False).cpu(), v["moments_f32"], v["moments_f64"], "vaenet_a moments conv_precision=fp32")
    referee(net.decode(v["zin"].to(dev)).cpu(), v["dec_f32"], v["dec_f64"], "vaenet_a decode conv_precision=fp32")


def test_forward_returns_the_sample_and_its_reconstruction(dev, golden):
    net, v = _net(dev, golden, "a")
    torch.manual_seed(9)
    z, rec = net(v["x"].to(dev))
    torch.manual_seed(9)
    z2 = net.encode(v["x"].to(dev))
    assert tuple(z.shape) == (2, 3, 16, 16) and tuple(rec.shape) == (2, 1, 32, 32)
    assert torch.equal(z, z2) and torch.equal(rec, net.decode(z))


def test_latent_karras_module_encodes_and_decodes_through_vaenet(dev, golden):
    import diffsci_amd.models as M
    vae, v = _net(dev, golden, "a")
    torch.manual_seed(3)
    net = M.PUNetG(M.PUNetGConfig(model_channels=8, input_channels=3, output_channels=3))
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), autoencoder=vae).to(dev).eval()
    got = module.sample(2, [1, 32, 32], nsteps=3)                       # the latent shape is learned through encode
    assert tuple(got.shape) == (2, 1, 32, 32) and bool(torch.isfinite(got).all())
    z = module.sample(2, [3, 16, 16], nsteps=3, is_latent_shape=True, return_in_latent_space=True)
    assert tuple(z.shape) == (2, 3, 16, 16)
    sd = {k: t.detach().cpu() for k, t in vae.decoder.state_dict().items()}
    with torch.inference_mode():
        w32 = vaenet_ref.decoder(sd, z.cpu())
        w64 = vaenet_ref.decoder({k: t.double() for k, t in sd.items()}, z.cpu().double())
    referee(module.decode(z).cpu(), w32, w64, "latent sample decoded")
    x = v["x"].to(dev)
    torch.manual_seed(21)
    a = module.encode(x)
    torch.manual_seed(21)
    b = vae.encode(x)
    assert tuple(a.shape) == (2, 3, 16, 16) and torch.equal(a, b)
