"""LDM AutoencoderKL decoder on a real MI355X: the GroupNorm(G, C) kernels of ds_groupnorm.hip against torch in fp64, the blocks
against the restatement tests/ldm_ref.py, the decoders against the fixtures the reference produced (tests/golden/ldm_*.npz), on
the folded and the standalone norm routes, and a latent KarrasModule that decodes through it.

Bounds.  Kernels: rel-L2 < 5e-7 against fp64, the bound of test_group1_norm_kernels (same input distribution).  Statistics from
tile statistics: 1e-6 relative, the means with the absolute floor of 1e-7 that the other tile-route test uses (a tile's shifted
fp32 sum carries an absolute error proportional to the tensor's scale, not to the mean).  Folded against standalone: rel-L2 < 2e-6
(test_adm_fused_and_standalone_norms_agree).  Networks and blocks: rel-L2 < 1e-5 against the fp32 reference and, against fp64,
within max(4 x the reference's own fp32-vs-fp64 distance, 2e-6) -- the referee rule of tests/test_gpu_adm.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import ldm_ref  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

REL = 1e-5
G = 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = ldm_ref.load_golden(tag)
        return cache[tag]
    return get


def _mod(which):
    import importlib
    return importlib.import_module("diffsci_amd.models.nets.autoencoderldm" + which)


def referee(got, want32, want64, what=""):
    e32, e64, ref = rel_l2(got, want32), rel_l2(got, want64), rel_l2(want32, want64)
    print(f"{what}: vs fp32 {e32:.2e}; vs fp64 {e64:.2e}; reference fp32 vs fp64 {ref:.2e}")
    assert e32 < REL, (what, e32)
    assert e64 < max(4 * ref, 2e-6), (what, e64, ref)


NORM_SHAPES = [
    (2, 32, 32, (5, 7)),          # one channel per group; 35-float planes: unaligned group starts, the scalar path
    (3, 64, 32, (8, 8)),          # two channels per group
    (1, 96, 32, (3, 5)),          # three channels per group
    (2, 12, 3, (4, 4)),           # G != 32
    (2, 64, 32, (3, 4, 5)),       # a volume
    (1, 64, 32, (128, 128)),      # a group spanning two reduction chunks
    (2, 32, 32, (8, 8)),          # with one group constant (variance 0 under eps 1e-6)
]


@pytest.mark.parametrize("case", range(len(NORM_SHAPES)))
def test_groupnorm_kernels_against_fp64(dev, case):
    from diffsci_amd import ops
    B, C, groups, spatial = NORM_SHAPES[case]
    torch.manual_seed(100 + case)
    x = torch.randn(B, C, *spatial) * 3 + 0.7
    if case == len(NORM_SHAPES) - 1:
        x[:, 5] = 0.7
    w, b = torch.randn(C), torch.randn(C)
    xd = x.to(dev)
    st = ops.groupnorm_stats(xd, groups, eps=1e-6)
    assert tuple(st.shape) == (B, groups, 2) and bool(torch.isfinite(st).all())
    xg = x.double().reshape(B, groups, -1)
    assert torch.allclose(st[..., 0].cpu().double(), xg.mean(-1), rtol=1e-6, atol=3e-6)
    # rstd where the variance carries it; under a variance of 0 it is 1/sqrt(eps + rounding of E[x^2] - mean^2), which multiplies
    # an exact x - mean = 0, so there only the output is compared
    live = xg.var(-1, unbiased=False) > 1e-3
    assert torch.allclose(st[..., 1].cpu().double()[live], (xg.var(-1, unbiased=False) + 1e-6).rsqrt()[live], rtol=2e-6, atol=0)
    assert int((~live).sum()) == (B if case == len(NORM_SHAPES) - 1 else 0)
    for act in (0, 1):
        want = F.group_norm(x.double(), groups, w.double(), b.double(), 1e-6)
        want = F.silu(want) if act else want
        am = ops.amax_new(B, dev)
        got = ops.groupnorm_apply(xd, st, w.to(dev), b.to(dev), groups, act=bool(act), out_amax=am)
        assert bool(torch.isfinite(got).all())
        err = rel_l2(got.cpu(), want)
        print(f"groupnorm {NORM_SHAPES[case]} act={act}: rel-L2 {err:.2e}")
        assert err < 5e-7
        assert torch.equal(am.view(torch.float32), got.reshape(B, -1).abs().amax(1))
        assert torch.equal(ops.groupnorm_apply(xd, st, w.to(dev), b.to(dev), groups, act=bool(act)), got)
    plain = ops.groupnorm_apply(xd, st, None, None, groups)
    assert rel_l2(plain.cpu(), F.group_norm(x.double(), groups, None, None, 1e-6)) < 5e-7


@pytest.mark.parametrize("shape", [(2, 16, 64, 24, 40), (3, 8, 96, 7, 9), (1, 32, 32, 64, 64)])
def test_statistics_and_table_from_tile_statistics(dev, shape):
    """A 3x3 fp16x3 convolution leaves tile statistics: the group statistics from them against a pass over its output, and the
    consumer's folded loader (table from the tiles, table from plain statistics) against apply + convolution."""
    from diffsci_amd import ops
    B, Cin, C, H, W = shape
    torch.manual_seed(7)
    x = torch.randn(B, Cin, H, W, device=dev)
    pw = ops.pack_conv(torch.randn(C, Cin, 3, 3, device=dev) / (3 * Cin ** 0.5), "fp16x3")
    ts = torch.zeros(B, C, ops.conv_tile_count(H, W), 4, device=dev)
    y = ops.conv(x, pw, bias=torch.randn(C, device=dev) * 3, tile_stats=ts)
    want = ops.groupnorm_stats(y, G, eps=1e-6)
    got = ops.groupnorm_stats_tiles(ts, G, H * W, eps=1e-6)
    # rstd: 1e-6 relative, no floor.  mean: 1e-6 relative plus the 1e-7 floor the other tile-route test uses (test_gpu_round2.py:772):
    # both sides are fp64 recombinations of fp32 partial sums, whose absolute error follows the tensor's scale (here ~3), not the
    # mean, so a group mean near zero cannot be held to a relative bound
    assert torch.allclose(got[..., 1], want[..., 1], rtol=1e-6, atol=0), ((got - want)[..., 1] / want[..., 1]).abs().max()
    assert torch.allclose(got[..., 0], want[..., 0], rtol=1e-6, atol=1e-7), (got - want)[..., 0].abs().max()
    w, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
    pw2 = ops.pack_conv(torch.randn(48, C, 3, 3, device=dev) / (3 * C ** 0.5), "fp16x3")
    am = ops.amax_new(B, dev)
    a = ops.groupnorm_apply(y, want, w, b, G, act=True, out_amax=am)
    ref = ops.conv(a, pw2, in_amax=am)
    Cpad = ops.table_channels(C)
    for name, tab in (("tiles", ops.groupnorm_table(w, b, G, H * W, tile_stats=ts, eps=1e-6)),
                      ("stats", ops.groupnorm_table(w, b, G, H * W, stats=want, eps=1e-6))):
        assert tuple(tab.shape) == (B, Cpad, 4)
        assert bool((tab[:, C:, :3] == 0).all())                                    # zero rows past C
        cpg = C // G
        if name == "stats":                                                          # the given pairs, one rounding for A
            assert torch.equal(tab[:, :C, 0], want[..., 0].repeat_interleave(cpg, 1))
            assert torch.equal(tab[:, :C, 1], want[..., 1].repeat_interleave(cpg, 1) * w)
        else:
            assert torch.allclose(tab[:, :C, 0], got[..., 0].repeat_interleave(cpg, 1), rtol=1e-6, atol=1e-7)
            assert torch.allclose(tab[:, :C, 1], got[..., 1].repeat_interleave(cpg, 1) * w, rtol=1e-6, atol=0)
        assert torch.equal(tab[:, :C, 2], b.expand(B, C))
        # fourth column: 2^-k with k = 13 - floor(log2 U), U = max_c |A_c| sqrt(n_g var_g) + |C_c| (one binade of slack: U is rounded)
        inv = tab[:, :, 3]
        assert bool((inv == inv[:, :1]).all()) and bool((torch.frexp(inv)[0] == 0.5).all())
        yg = y.double().reshape(B, G, -1)
        dev2 = (yg.var(-1, unbiased=False) * yg.shape[-1]).sqrt().repeat_interleave(cpg, 1)
        U = (tab[:, :C, 1].double().abs() * dev2 + tab[:, :C, 2].double().abs()).amax(1)
        assert float((torch.log2(inv[:, 0]).double() + 13 - torch.floor(torch.log2(U))).abs().max()) <= 1
        err = rel_l2(ops.conv(y, pw2, prenorm=tab).cpu(), ref.cpu())
        print(f"folded ({name}) vs apply + conv at {shape}: {err:.2e}")
        assert err < 2e-6


def _block_case(dev, which, kind):
    """(module on the device, input, fp32 and fp64 restatement outputs) for one block of one dimension."""
    mod = _mod(which)
    torch.manual_seed({"res32_64": 1, "res64_64": 2, "res_convsc": 3, "attn": 4, "up_conv": 5, "up_plain": 6}[kind])
    sp = (16, 24) if which == "2d" else (4, 6, 8)
    if kind.startswith("res"):
        cin = 32 if kind != "res64_64" else 64
        blk = mod.ResnetBlock(in_channels=cin, out_channels=64, conv_shortcut=kind == "res_convsc", dropout=0.0, temb_channels=0)
        fn = ldm_ref.resnet_block
    elif kind == "attn":
        cin, blk, fn = 64, mod.AttnBlock(64), ldm_ref.attn_block
    else:
        cin, blk, fn = 64, mod.Upsample(64, kind == "up_conv"), ldm_ref.upsample
    with torch.no_grad():
        for k, v in blk.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                v.add_(0.25 * torch.randn_like(v))
    x = torch.randn(2, cin, *sp) * 1.5 + 0.3
    sd = blk.state_dict()
    with torch.inference_mode():
        w32, w64 = fn(x, sd), fn(x.double(), {k: v.double() for k, v in sd.items()})
    return blk.to(dev), x.to(dev), w32, w64


@pytest.mark.parametrize("which", ["2d", "3d"])
@pytest.mark.parametrize("kind", ["res32_64", "res64_64", "res_convsc", "attn", "up_conv", "up_plain"])
def test_blocks_against_the_restatement(dev, which, kind):
    blk, x, w32, w64 = _block_case(dev, which, kind)
    outs = {}
    for fuse in (True, False):
        blk.fuse_norm = fuse
        out = blk(x, None) if kind.startswith("res") else blk(x)
        outs[fuse] = out.cpu()
        assert out.shape == w32.shape
        if kind == "up_plain":
            assert torch.equal(outs[fuse], w32)
        else:
            referee(outs[fuse], w32, w64, f"{which} {kind} fuse_norm={fuse}")
    assert rel_l2(outs[True], outs[False]) < 2e-6


def _decoder(dev, golden, tag):
    v, sd, info = golden(tag)
    net = ldm_ref.build(info)
    net.load_state_dict({k: t for k, t in sd.items()}, strict=True)
    return net.to(dev).eval(), v


@pytest.mark.parametrize("tag", ["a", "a2", "b", "c"])
def test_decoders_against_the_reference_on_both_norm_routes(dev, golden, tag):
    net, v = _decoder(dev, golden, tag)
    z = v["z"].to(dev)
    outs = {}
    for fuse in (True, False):
        net.fuse_norm = fuse
        outs[fuse] = net(z).cpu()
        assert outs[fuse].shape == v["out_f32"].shape and tuple(net.last_z_shape) == tuple(z.shape)
        referee(outs[fuse], v["out_f32"], v["out_f64"], f"ldm_{tag} fuse_norm={fuse}")
    assert rel_l2(outs[True], outs[False]) < 2e-6


def test_decoder_exact_fp32_convolutions(dev, golden):
    net, v = _decoder(dev, golden, "a")
    net.conv_precision = "fp32"
    referee(net(v["z"].to(dev)).cpu(), v["out_f32"], v["out_f64"], "ldm_a conv_precision=fp32")


def test_decoder_options_against_the_restatement(dev, golden):
    """give_pre_end, resamp_with_conv=False and attn_type='none' on case a's weights (strict=False drops the unused ones)."""
    v, sd, info = golden("a")
    mod = ldm_ref.module_of(info)
    net = mod.Decoder(mod.ddconfig(**info["ddconfig"]), resamp_with_conv=False, give_pre_end=True, attn_type="none")
    r = net.load_state_dict(sd, strict=False)
    assert not r.missing_keys
    kept = {k: t for k, t in sd.items() if k in net.state_dict()}
    with torch.inference_mode():
        w32 = ldm_ref.decoder(kept, v["z"], give_pre_end=True)
        w64 = ldm_ref.decoder({k: t.double() for k, t in kept.items()}, v["z"], give_pre_end=True)
    referee(net.to(dev)(v["z"].to(dev)).cpu(), w32, w64, "ldm_a give_pre_end, no upsampling convolution, no attention")


def _vae(dev, golden, embed_dim):
    v, sd, info = golden("ae")
    a2 = _mod("2d")
    vae = a2.AutoencoderKL(a2.ddconfig(**info["ddconfig"]), embed_dim=embed_dim)
    if embed_dim == info["embed_dim"]:
        vae.load_state_dict(sd, strict=True)
    else:
        vae.decoder.load_state_dict(ldm_ref.sub(sd, "decoder."), strict=True)
    return vae.to(dev).eval(), v


def test_autoencoder_decode_with_embed_dim_other_than_z_channels(dev, golden):
    vae, v = _vae(dev, golden, 3)
    outs = {}
    for fuse in (True, False):
        vae.fuse_norm = fuse
        outs[fuse] = vae.decode(v["z"].to(dev)).cpu()
        referee(outs[fuse], v["out_f32"], v["out_f64"], f"ldm_ae fuse_norm={fuse}")
    assert rel_l2(outs[True], outs[False]) < 2e-6


def test_latent_karras_module_decodes_through_the_hip_decoder(dev, golden):
    import diffsci_amd.models as M
    vae, _ = _vae(dev, golden, 4)
    torch.manual_seed(3)
    net = M.PUNetG(M.PUNetGConfig(model_channels=8, input_channels=4, output_channels=4))
    wrapper = M.nets.LDMAutoencoderKLWrapper(vae)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), autoencoder=wrapper).to(dev).eval()
    torch.manual_seed(11)
    got = module.sample(2, [4, 16, 16], nsteps=3, is_latent_shape=True)
    torch.manual_seed(11)
    z = module.sample(2, [4, 16, 16], nsteps=3, is_latent_shape=True, return_in_latent_space=True)
    assert tuple(got.shape) == (2, 1, 32, 32) and tuple(z.shape) == (2, 4, 16, 16)
    sd = {k: t.detach().cpu() for k, t in vae.state_dict().items()}
    with torch.inference_mode():
        w32 = ldm_ref.autoencoder_decode(sd, z.cpu())
        w64 = ldm_ref.autoencoder_decode({k: t.double() for k, t in sd.items()}, z.cpu().double())
    referee(got.cpu(), w32, w64, "latent sample")
    one = wrapper.decode(z[0], has_batch_dim=False)
    assert tuple(one.shape) == (1, 32, 32) and rel_l2(one.cpu(), w32[0]) < REL
    with pytest.raises(NotImplementedError, match="encoder.*outside the HIP sampling path"):
        module.sample(2, [1, 32, 32], nsteps=3)
