"""runtime.attention -- the one attention launch sequence of PUNetG, ADM, DiffusionTransformer and the LDM / VAENet blocks --
against fp64 torch (fp64 projections, scaled_dot_product_attention per head), on the smallest shape that takes each of its
branches.  Sample 0 of every input is scaled by 2^-20 (the per-sample activation exponents), and every figure is judged per
sample as well as over the batch, since the batch figure does not see a sample 2^20 times smaller than its neighbour.

Bound (tests/test_gpu_sampler.py::test_punetg_forward_vs_reference): rel_l2(got, fp64) < max(4 * rel_l2(torch fp32, fp64), 2e-6)."""
import math
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import rel_l2

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "E heads H W B cosine precision", defaults=(False, "fp16x3"))
CASES = {
    "split_staging": Case(32, 1, 8, 8, 2),                       # epilogue split rows, staging kernel
    "no_split": Case(48, 1, 8, 8, 2),                            # explicit reductions, exact-fp32 attention, out_amax by reduction
    "heads": Case(64, 2, 8, 8, 2),                               # head-axis kernel at d = 32
    "odd_length": Case(32, 1, 5, 7, 2),                          # L % 32 != 0
    "images": Case(32, 1, 32, 64, 1),                            # L = 2048: the image form and its workspace buffer
    "cosine": Case(32, 1, 8, 8, 2, cosine=True),
    "fp32": Case(32, 1, 8, 8, 2, precision="fp32"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sdpa(qkv, E, H, dtype):
    B, _, L = qkv.shape
    q, k, v = (t.to(dtype).reshape(B, H, E // H, L).transpose(-1, -2) for t in qkv.split(E, dim=1))
    return F.scaled_dot_product_attention(q, k, v).transpose(-1, -2).reshape(B, E, L)


def _torch_attention(c, t, dtype):
    """The block in torch at `dtype`, without residuals -> [B, E, H, W]."""
    x = t["x"].to(dtype).flatten(2)
    qkv = torch.einsum("oc,bcl->bol", t["w_in"].to(dtype), x)
    if t["b_in"] is not None:
        qkv = qkv + t["b_in"].to(dtype)[None, :, None]
    if c.cosine:                 # unit queries and keys, logits q.k (the kernels' 1/sqrt(E) is cancelled by the queries' gain)
        q, k, v = qkv.split(c.E, dim=1)
        q = q / (q.norm(dim=1, keepdim=True) + 1e-8) * math.sqrt(c.E)
        k = k / (k.norm(dim=1, keepdim=True) + 1e-8)
        qkv = torch.cat([q, k, v], dim=1)
    y = torch.einsum("oc,bcl->bol", t["w_out"].to(dtype), _sdpa(qkv, c.E, c.heads, dtype))
    if t["b_out"] is not None:
        y = y + t["b_out"].to(dtype)[None, :, None]
    return y.reshape(t["x"].shape)


_REFERENCES = {}


def _reference(name):
    """Inputs and the fp64 / fp32 torch results of a case, computed once and left unchanged."""
    if name not in _REFERENCES:
        c = CASES[name]
        g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
        t = {"x": torch.randn(c.B, c.E, c.H, c.W, generator=g),
             "w_in": torch.randn(3 * c.E, c.E, generator=g) / math.sqrt(c.E),
             "w_out": torch.randn(c.E, c.E, generator=g) / math.sqrt(c.E),
             # the in-house attention (cosine) carries no biases; there sample 0's output is 2^-20 of sample 1's
             "b_in": None if c.cosine else 0.1 * torch.randn(3 * c.E, generator=g),
             "b_out": None if c.cosine else 0.1 * torch.randn(c.E, generator=g),
             "res1": torch.randn(c.B, c.E, c.H, c.W, generator=g),
             "res2": torch.randn(c.B, c.E, c.H, c.W, generator=g)}
        for k in ("x", "res1", "res2"):
            t[k][0] *= 2.0 ** -20
        t["f64"] = _torch_attention(c, t, torch.float64)
        t["f32"] = _torch_attention(c, t, torch.float32)
        _REFERENCES[name] = t
    return _REFERENCES[name]


def _run(c, t, dev, pooled, want_amax=False, residuals=False):
    """-> (y on the host, out_amax or None, tile statistics or None, the pool or None)."""
    from diffsci_amd import ops
    from diffsci_amd.models.nets import runtime
    kind = "fp16x3" if c.precision == "fp16x3" else "fp32"
    E = c.E
    w_in = ops.pack_conv(t["w_in"].reshape(3 * E, E, 1, 1).to(dev), kind)
    w_out = ops.pack_conv(t["w_out"].reshape(E, E, 1, 1).to(dev), kind)
    b_in, b_out = (None if t[k] is None else t[k].to(dev) for k in ("b_in", "b_out"))
    ws = runtime.Workspace() if pooled else None
    am = runtime.AmaxArena(ws, c.B, dev) if (pooled and kind == "fp16x3") else None
    kw = {}
    if want_amax:
        kw["out_amax"] = ops.amax_new(c.B, dev)
    if residuals:
        kw.update(res1=t["res1"].to(dev), res2=t["res2"].to(dev))
        if kind == "fp16x3":
            kw["tile_stats"] = torch.full((c.B, E, ops.conv_tile_count(c.H, c.W), 4), float("nan"), device=dev)
    y = runtime.attention(t["x"].to(dev), w_in, b_in, w_out, b_out, E=E, heads=c.heads, precision=c.precision, ws=ws, am=am,
                          cosine=c.cosine, **kw)
    if am is not None:
        am.release()
    return y.cpu(), kw.get("out_amax"), kw.get("tile_stats"), ws


def _judge(what, got, want64, want32):
    """The bound over the batch and per sample; prints every figure first."""
    bad = []
    for label, sl in [("batch", slice(None))] + [(f"sample {b}", slice(b, b + 1)) for b in range(got.shape[0])]:
        err, ref = rel_l2(got[sl], want64[sl]), rel_l2(want32[sl], want64[sl])
        print(f"[{what}] {label}: HIP vs fp64 {err:.3e}, torch fp32 vs fp64 {ref:.3e}")
        if not err < max(4 * ref, 2e-6):
            bad.append(f"{what} {label}: {err:.3e} >= max(4 x {ref:.3e}, 2e-6)")
    return bad


@pytest.mark.parametrize("name", list(CASES))
def test_attention_vs_fp64(dev, name):
    from diffsci_amd import ops
    c, t = CASES[name], _reference(name)
    h3 = c.precision == "fp16x3"
    L = c.H * c.W
    pooled, amax, _, ws = _run(c, t, dev, True, want_amax=h3)
    plain, _, _, _ = _run(c, t, dev, False)
    assert torch.equal(pooled, plain)                # pool + arena or fresh tensors, out_amax asked or not: the same bits
    nws = ops.attention_workspace_floats(c.B, c.E, L, c.precision, heads=c.heads)
    assert (nws > 0) == (name == "images")
    if nws:
        assert ((nws,), str(dev)) in ws.free         # the image buffer came from the pool and went back
    assert ((c.B, 3 * c.E, c.H, c.W), str(dev)) in ws.free and ((c.B, c.E, L), str(dev)) in ws.free
    if h3:                                           # (the exact-fp32 packings take no amax arguments: no network asks there)
        assert torch.equal(amax.cpu().view(torch.float32), pooled.abs().flatten(1).max(dim=1).values)
    bad = _judge(name, pooled, t["f64"], t["f32"])
    # + res1 + res2 in the out-projection's epilogue, which also leaves the tile statistics of what it stored
    with_res, _, stats, _ = _run(c, t, dev, True, residuals=True)
    res64 = t["res1"].double() + t["res2"].double()
    bad += _judge(name + " + residuals", with_res, t["f64"] + res64, (t["f32"] + t["res1"]) + t["res2"])
    assert not bad, bad
    if stats is not None:
        K, S, Q, n = stats.cpu().double().unbind(-1)              # per (channel, tile); see test_conv_tile_stats_and_fused_prenorm
        assert torch.equal(n.sum(-1), torch.full((c.B, c.E), float(L), dtype=torch.float64))
        y = with_res.double()
        # fp32 accumulation of L terms: |error| <= L * 2^-24 * sum |y|
        assert ((n * K + S).sum(-1) - y.sum(dim=(2, 3))).abs().le(L * 2.0 ** -24 * y.abs().sum(dim=(2, 3))).all()


def test_adm_refuses_per_sample_rows_of_another_batch(dev):
    """[n_evals, B', 2C] FiLM tables with B' != B raise before any block runs (runtime.shift_rows, as in PUNetG)."""
    import diffsci_amd.models as M
    net = M.ADM(M.ADMConfig(model_channels=8, time_embed_dim=8, output_embed_dim=16)).to(dev).eval()
    shifts = [torch.zeros(2, 3, 2 * b.cout, device=dev) for b in net._blocks()]
    with pytest.raises(ValueError, match="time embedding batch does not match x"):
        net.forward_with_shifts(torch.zeros(2, 1, 16, 16, device=dev), shifts, row=0)
