"""Multi-head attention (nn.MultiheadAttention(E, H) core) on the HIP kernels: ops.attention(..., heads=H) against torch's
fp64 scaled_dot_product_attention on the per-head split, the ADM blocks with attn_heads=4 against an fp64 torch composition
of the same weights, and a captured sampling run through such blocks.

Tolerance: the kernels' rel-L2 against fp64 is at most 3x torch's own fp32 error against fp64 on the same input."""

import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


def _sdpa(qkv, E, H, dtype):
    """torch's attention on the per-head split of channel-major qkv [B, 3E, L] -> [B, E, L]."""
    B, _, L = qkv.shape
    q, k, v = (t.to(dtype).reshape(B, H, E // H, L).transpose(-1, -2) for t in qkv.split(E, dim=1))
    return F.scaled_dot_product_attention(q, k, v).transpose(-1, -2).reshape(B, E, L)


def _check(name, got, qkv, E, H):
    want = _sdpa(qkv, E, H, torch.float64)
    ref_err = rel_l2(_sdpa(qkv, E, H, torch.float32), want)
    err = rel_l2(got, want)
    print(f"[{name}] HIP vs fp64 {err:.2e}, torch fp32 vs fp64 {ref_err:.2e}")
    return err <= 3 * ref_err, f"{name}: {err:.3e} > 3 x {ref_err:.3e}"


CASES = [(E, H, L, B) for E in (128, 256) for H in (2, 4, 8) for L in (256, 1024, 4096) for B in (1, 3)]
CASES += [(128, 16, L, B) for L in (256, 1024, 4096) for B in (1, 3)]          # d = 8: outside the MFMA widths


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
def test_attention_heads_vs_fp64(dev, precision):
    from diffsci_amd import ops
    bad = []
    for E, H, L, B in CASES:
        if precision == "fp32" and L == 4096 and B == 3:
            continue                                 # the exact path is a correctness path: one batch tail at this length
        g = torch.Generator().manual_seed(E * 7 + H * 3 + L + B)
        qkv = torch.randn(B, 3 * E, L, generator=g)
        got = ops.attention(qkv.to(dev), E, precision=precision, heads=H).cpu()
        ok, msg = _check(f"{precision} E={E} H={H} L={L} B={B}", got, qkv, E, H)
        if not ok:
            bad.append(msg)
    assert not bad, bad


def test_attention_heads_per_sample_magnitudes(dev):
    """in_amax carries one exponent pair per sample; every head of the sample is staged with it."""
    from diffsci_amd import ops
    E, H = 256, 4
    for L in (1024, 2048):                          # K / V staged in every workgroup; pre-split images (d = 64 from L = 2048)
        g = torch.Generator().manual_seed(11 + L)
        qkv = torch.randn(2, 3 * E, L, generator=g)
        qkv[0] *= 2.0 ** -20
        qkv[1] *= 2.0 ** 20
        qkv[1, :2 * E] *= 2.0 ** -20               # sample 1: q, k of order 1 (finite logits), v of order 2^20
        x = qkv.to(dev)
        in_amax = torch.cat([ops.absmax_rows(x[:, :2 * E]), ops.absmax_rows(x[:, 2 * E:])])
        assert (ops.attention_workspace_floats(2, E, L, "fp16x3", heads=H) > 0) == (L == 2048)
        out_amax = ops.amax_new(2, dev)
        got = ops.attention(x, E, precision="fp16x3", heads=H, in_amax=in_amax, out_amax=out_amax).cpu()
        for b in range(2):
            ok, msg = _check(f"magnitudes L={L} sample {b}", got[b:b + 1], qkv[b:b + 1], E, H)
            assert ok, msg
        want_amax = got.abs().flatten(1).max(dim=1).values
        assert torch.equal(out_amax.cpu().view(torch.float32), want_amax)


def test_attention_heads_one_is_the_single_head_call(dev):
    from diffsci_amd import ops
    for E, L in ((256, 1024), (128, 4096), (64, 256)):
        qkv = torch.randn(3, 3 * E, L, generator=torch.Generator().manual_seed(E + L)).to(dev)
        for precision in ("fp16x3", "fp32"):
            a = ops.attention(qkv, E, precision=precision)
            b = ops.attention(qkv, E, precision=precision, heads=1)
            assert torch.equal(a, b)


def test_image_and_staging_forms_agree(dev):
    """ds_attention_h3_heads with and without the K / V image workspace: the same bits."""
    from diffsci_amd import _native as N
    for E, H, L in ((256, 4, 1024), (128, 2, 512), (256, 8, 256)):
        B = 3
        qkv = torch.randn(B, 3 * E, L, generator=torch.Generator().manual_seed(L + H)).to(dev)
        outs = []
        for ws in (False, True):
            out = torch.empty(B, E, L, device=dev)
            work = torch.empty(N.lib().ds_attention_h3_heads_workspace_bytes(B, E, H, L) // 4, device=dev) if ws else None
            N.check(N.lib().ds_attention_h3_heads(out.data_ptr(), qkv.data_ptr(), None if work is None else work.data_ptr(),
                                                  B, E, H, L, None, None, torch.cuda.current_stream().cuda_stream),
                    "ds_attention_h3_heads")
            outs.append(out)
        assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- ADM blocks with attn_heads = 4
def _norm(kind, x, w, b):
    if kind == "GroupLN":
        return F.group_norm(x, 1, w, b, 1e-5)
    dims = tuple(range(1, x.dim()))                  # GroupRMSNorm(1, C): RMS over (C, spatial) of each sample
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return x / torch.sqrt(x.pow(2).mean(dim=dims, keepdim=True) + 1e-5) * w.view(shape) + b.view(shape)


def _block_torch(blk, sd, x, te, skip=None, sample=None):
    """ADMBaseBlock.forward as a torch composition of the state_dict's tensors (dtype of x): norm1 -> SiLU -> resample ->
    conv1 -> norm2 -> FiLM -> SiLU -> conv2 (+ convresidual(resample(x))) -> nn.MultiheadAttention over the positions
    (+ residual)."""
    vol = x.dim() == 5
    conv = F.conv3d if vol else F.conv2d
    if skip is not None:
        x = torch.cat([x, skip], dim=1)

    def resample(v):
        if sample == "down":
            return (F.avg_pool3d if vol else F.avg_pool2d)(v, 2)
        if sample == "up":
            return F.interpolate(v, scale_factor=2.0, mode="nearest")
        return v
    kinds = ("GroupLN" if blk.kinds[0] == 0 else "GroupRMS", "GroupLN" if blk.kinds[1] == 0 else "GroupRMS")
    y = F.silu(_norm(kinds[0], x, sd["norm1.weight"], sd["norm1.bias"]))
    y = conv(resample(y), sd["conv1.weight"], sd["conv1.bias"], padding=1)
    y = _norm(kinds[1], y, sd["norm2.weight"], sd["norm2.bias"])
    te1, te2 = torch.chunk(F.linear(te, sd["embed_linear.weight"], sd["embed_linear.bias"]), 2, dim=-1)
    one = (1,) * (y.dim() - 2)
    y = conv(F.silu(y * te1.view(*te1.shape, *one) + te2.view(*te2.shape, *one)), sd["conv2.weight"], sd["conv2.bias"],
             padding=1)
    y = y + conv(resample(x), sd["convresidual.weight"], sd["convresidual.bias"])
    B, C = y.shape[:2]
    mh = torch.nn.MultiheadAttention(C, num_heads=4, batch_first=True).to(y.dtype)
    mh.load_state_dict({k[len("attn.mhattn."):]: v for k, v in sd.items() if k.startswith("attn.mhattn.")})
    t = y.reshape(B, C, -1).transpose(1, 2)
    with torch.no_grad():
        a, _ = mh(t, t, t, need_weights=False)
    return y + a.transpose(1, 2).reshape(y.shape)


@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("case", ["enc2d", "dec3d"])
def test_adm_blocks_with_four_heads_vs_fp64(M, dev, case, precision):
    torch.manual_seed(3)
    if case == "enc2d":      # E = 128, d = 32: the MFMA kernel; L = 32 x 32 = 1024
        blk = M.nets.ADMEncoderBlock(16, 128, 24, has_residual=True, has_attn=True, attn_heads=4)
        x, skip, sample = torch.randn(2, 16, 32, 32), None, None
    else:                    # E = 64, d = 16: the exact per-head path; L = 8^3 = 512 after the upsampling
        blk = M.nets.ADMDecoderBlock(16, 64, 24, channels_skip=8, has_residual=True, has_attn=True, has_upsample=True,
                                     dimension=3, attn_heads=4)
        x, skip, sample = torch.randn(2, 16, 4, 4, 4), torch.randn(2, 8, 4, 4, 4), "up"
    with torch.no_grad():    # non-trivial norm affines and biases
        for k, w in blk.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                w.add_(0.1 * torch.randn_like(w))
    sd = {k: w.detach().clone() for k, w in blk.state_dict().items()}
    te = torch.randn(2, 24)
    fresh = type(blk)(*((16, 128, 24) if case == "enc2d" else (16, 64, 24)),
                      **(dict(has_residual=True, has_attn=True, attn_heads=4) if case == "enc2d" else
                         dict(channels_skip=8, has_residual=True, has_attn=True, has_upsample=True, dimension=3, attn_heads=4)))
    r = fresh.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    fresh = fresh.to(dev).eval()
    fresh.conv_precision = precision
    args = [x.to(dev), te.to(dev)] + ([skip.to(dev)] if skip is not None else [])
    got = fresh(*args).cpu()
    sd64 = {k: v.double() for k, v in sd.items()}
    sd32 = {k: v.float() for k, v in sd.items()}
    want = _block_torch(fresh, sd64, x.double(), te.double(), None if skip is None else skip.double(), sample)
    want32 = _block_torch(fresh, sd32, x, te, skip, sample)
    ref_err = rel_l2(want32, want)
    err = rel_l2(got, want)
    print(f"[{case} {precision}] HIP vs fp64 {err:.2e}, torch fp32 vs fp64 {ref_err:.2e}")
    assert got.shape == want.shape
    assert err < max(4 * ref_err, 2e-6)


class _HeadsNet(torch.nn.Module):
    """A small score network of ADM blocks with 4-head attention: net(x, c_noise)."""

    def __init__(self, M):
        super().__init__()
        self.emb = torch.nn.Parameter(torch.randn(1, 24))
        self.enc = M.nets.ADMEncoderBlock(16, 128, 24, has_residual=True, has_attn=True, attn_heads=4)
        self.out = M.nets.ADMEncoderBlock(128, 16, 24, has_residual=True)

    def forward(self, x, t):
        te = torch.sin(t.view(-1, 1) * self.emb)
        return self.out(self.enc(x, te), te)


def test_captured_sampling_with_heads(M, dev):
    torch.manual_seed(4)
    net = _HeadsNet(M).to(dev).eval()
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).to(dev)
    wn = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(5)).to(dev)
    eager = module.propagate_white_noise(wn, nsteps=4).cpu()
    assert torch.isfinite(eager).all() and len(module._plans.plans) == 0
    module.capture_eager = True                      # the same run captured as a graph and replayed
    a = module.propagate_white_noise(wn, nsteps=4).cpu()
    b = module.propagate_white_noise(wn, nsteps=4).cpu()
    assert len(module._plans.plans) == 1
    assert torch.equal(a, eager) and torch.equal(b, eager)
