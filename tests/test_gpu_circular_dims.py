"""Periodic padding per axis (circular_dims of CircularConv2d / CircularConv3d, commonlayers.py:918-1034) on a real MI355X:
every kernel route that wraps, with each single-axis mask (volumes: each complementary two-axis mask as well), against torch
on the CPU in fp64 -- F.pad per axis ("circular" or "constant"), then the convolution without padding; the same in fp32 is the
yardstick.  Bounds are those of test_conv_circular_padding (fp16x3: 3 x) and test_conv_direct_small_cout (direct: 4 x).  A
mixed mask must also differ (> 1e-3) from both the zero-padded and the all-periodic result of the same input."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import circular_dims_pc as PC  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

T, Fa = True, False
MASKS2 = [(T, Fa), (Fa, T)]
MASKS3 = [(T, Fa, Fa), (Fa, T, Fa), (Fa, Fa, T), (Fa, T, T), (T, Fa, T), (T, T, Fa)]


def _id(m):
    return "".join("p" if a else "z" for a in m)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


def pad_axes(t, mask, p=1):
    """Pad the last len(mask) axes of t by p on both sides, axis by axis: periodic where the mask says so, zeros elsewhere."""
    n = len(mask)
    for i, a in enumerate(mask):
        pads = [0] * (2 * n)
        pads[2 * (n - 1 - i)] = pads[2 * (n - 1 - i) + 1] = p
        t = F.pad(t, pads, mode="circular" if a else "constant")
    return t


def _bound(got, ref32, want, k=3):
    e, e32 = rel_l2(got, want), rel_l2(ref32, want)
    print(f"rel_l2 {e:.3e}  torch fp32 {e32:.3e}")
    assert e <= max(k * e32, 3e-7), (e, e32)


def _mixed(got, zero, full):
    """Conditions of a mixed mask: it is neither the zero-padded nor the all-periodic result."""
    assert rel_l2(got, zero) > 1e-3 and rel_l2(got, full) > 1e-3, (rel_l2(got, zero), rel_l2(got, full))


# (B, Cin, Cout, H, W, load mode, form)
ONE_SHOT = {
    "plain": (2, 16, 24, 32, 32, 0, None),
    "ragged-two-channel-tiles": (1, 40, 8, 20, 36, 0, None),
    "scalar-staging": (1, 8, 8, 9, 13, 0, None),
    "plane-below-tile": (1, 4, 4, 8, 8, 0, None),
    "three-rows": (1, 8, 8, 3, 35, 0, None),
    "maxpool": (1, 16, 32, 16, 32, 1, None),
    "upsample-one-shot": (1, 24, 12, 16, 32, 2, None),
    "upsample-parity": (1, 24, 12, 16, 64, 2, "parity"),
    "fused-loader": (2, 16, 24, 32, 32, 0, "prenorm"),
    "k5": (1, 8, 8, 12, 40, 0, "k5"),
}


@pytest.mark.parametrize("mask", MASKS2, ids=_id)
@pytest.mark.parametrize("name", list(ONE_SHOT))
def test_one_shot_3x3(dev, ops, name, mask):
    B, Cin, Cout, H, W, mode, form = ONE_SHOT[name]
    k = 5 if form == "k5" else 3
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    Hin, Win = (2 * H, 2 * W) if mode == 1 else ((H // 2, W // 2) if mode == 2 else (H, W))
    x = torch.randn(B, Cin, Hin, Win, generator=g) * 1.3 + 0.2
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    bias = torch.randn(Cout, generator=g)
    kw = {}
    src = F.max_pool2d(x, 2) if mode == 1 else (F.interpolate(x, scale_factor=2.0, mode="nearest") if mode == 2 else x)
    src64 = src.double()
    if form == "prenorm":
        # x = a producer's output with its tile statistics; the reference normalises first and pads after
        w0 = torch.randn(Cin, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
        ts = torch.zeros(B, Cin, ops.conv_tile_count(H, W), 4, device=dev)
        xd = ops.conv(x.to(dev), ops.pack_conv(w0.to(dev), "fp16x3"), tile_stats=ts)
        wn, bn = torch.randn(Cin, generator=g), torch.randn(Cin, generator=g)
        kw["prenorm"] = ops.inorm_table(ts, wn.to(dev), bn.to(dev), 0, H * W)
        x = xd.cpu()
        src64 = F.silu(F.group_norm(x.double(), Cin, wn.double(), bn.double(), 1e-5))
        src = src64.float()
    pw = ops.pack_conv(w.to(dev), "fp16x3", upsampled=form == "parity")
    if form == "parity":
        assert pw.up is not None and ops.N.lib().ds_conv2d_h3_up_supported(Hin, Win)
    run = lambda c: ops.conv(x.to(dev), pw, bias=bias.to(dev), load_mode=mode, circular=c, **kw).cpu()   # noqa: E731
    got = run(mask)
    want = F.conv2d(pad_axes(src64, mask, k // 2), w.double(), bias.double())
    _bound(got, F.conv2d(pad_axes(src, mask, k // 2), w, bias), want)
    zero, full = run(False), run(True)
    _mixed(got, zero, full)
    assert torch.equal(run((Fa, Fa)), zero) and torch.equal(run((T, T)), full)


@pytest.fixture(scope="module")
def pc_one_shot(tmp_path_factory):
    """The fused-loader launches of the persistent case on the one-shot kernel: a child process with DS_CONV_PC=0."""
    out = str(tmp_path_factory.mktemp("pc") / "one_shot.pt")
    p = subprocess.run([sys.executable, PC.__file__, out], env=dict(os.environ, DS_CONV_PC="0"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return torch.load(out, weights_only=False)


@pytest.mark.parametrize("mask", PC.MASKS, ids=_id)
def test_persistent_kernel(dev, ops, pc_one_shot, mask):
    """ds_conv3p.hip: raw input (pc_raw) and the fused loader, against fp64 and bit for bit against the one-shot launch."""
    B, Cin, Cout, H, W = PC.SHAPE
    assert B * (Cout // 64) * (H // 8) * (W // 32) >= torch.cuda.get_device_properties(dev).multi_processor_count
    x, w, bias, wn, bn = PC.inputs()
    # raw input: the one-shot arm is the same call without pc_raw
    got = PC.run(ops, dev, mask, False, True)
    want = F.conv2d(pad_axes(x.double(), mask), w.double(), bias.double())
    _bound(got[0], F.conv2d(pad_axes(x, mask), w, bias), want)
    for a, b in zip(got, PC.run(ops, dev, mask, False, False)):
        assert torch.equal(a, b)
    for pre, raw in ((False, True), (True, False)):                    # both arms: the identities, and what a mixed mask is not
        zero, full = PC.run(ops, dev, False, pre, raw), PC.run(ops, dev, True, pre, raw)
        for a, b, c, d in zip(zero, PC.run(ops, dev, (Fa, Fa), pre, raw), full, PC.run(ops, dev, (T, T), pre, raw)):
            assert torch.equal(a, b) and torch.equal(c, d)
        _mixed(PC.run(ops, dev, mask, pre, raw)[0], zero[0], full[0])
    # fused norm + SiLU loader
    got = PC.run(ops, dev, mask, True, False)
    act = F.silu(F.group_norm(x.double(), Cin, wn.double(), bn.double(), PC.EPS))
    want = F.conv2d(pad_axes(act, mask), w.double(), bias.double())
    _bound(got[0], F.conv2d(pad_axes(act.float(), mask), w, bias), want)
    for a, b in zip(got, pc_one_shot[mask]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mask", MASKS2, ids=_id)
@pytest.mark.parametrize("case", [(2, 16, 2, 16, 16), (1, 5, 4, 18, 70), (1, 8, 3, 16, 64)], ids=["small", "ragged", "vector-loads"])
def test_conv_direct(dev, ops, case, mask):
    B, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    run = lambda c: ops.conv_direct(x.to(dev), w.to(dev), bias.to(dev), circular=c).cpu()   # noqa: E731
    got = run(mask)
    _bound(got, F.conv2d(pad_axes(x, mask), w, bias), F.conv2d(pad_axes(x.double(), mask), w.double(), bias.double()), k=4)
    zero, full = run(False), run(True)
    _mixed(got, zero, full)
    assert torch.equal(run((Fa, Fa)), zero) and torch.equal(run((T, T)), full)


def _vol(case, mode, seed):
    B, Cin, Cout, D, H, W = case
    g = torch.Generator().manual_seed(seed)
    sides = [2 * n if mode == 1 else (n // 2 if mode == 2 else n) for n in (D, H, W)]
    x = torch.randn(B, Cin, *sides, generator=g)
    src = F.max_pool3d(x, 2) if mode == 1 else (F.interpolate(x, scale_factor=2.0, mode="nearest") if mode == 2 else x)
    return g, x, src


@pytest.mark.parametrize("mask,mode", [(m, 0) for m in MASKS3] + [((Fa, T, Fa), 1), ((T, Fa, T), 2)],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else ("plain", "maxpool", "upsample")[v])
def test_conv3d_direct(dev, ops, mask, mode):
    case = (1, 5, 3, 6, 10, 12)
    g, x, src = _vol(case, mode, 31 + mode)
    w = torch.randn(3, 5, 3, 3, 3, generator=g) / math.sqrt(5 * 27)
    bias = torch.randn(3, generator=g)
    run = lambda c: ops.conv3d(x.to(dev), w.to(dev), bias=bias.to(dev), load_mode=mode, circular=c).cpu()   # noqa: E731
    got = run(mask)
    _bound(got, F.conv3d(pad_axes(src, mask), w, bias), F.conv3d(pad_axes(src.double(), mask), w.double(), bias.double()), k=4)
    zero, full = run(False), run(True)
    _mixed(got, zero, full)
    assert torch.equal(run((Fa, Fa, Fa)), zero) and torch.equal(run((T, T, T)), full)


@pytest.mark.parametrize("mask", MASKS3, ids=_id)
@pytest.mark.parametrize("k", [3, 5])
def test_conv3d_mfma(dev, ops, k, mask):
    case = (1, 16, 16, 4, 16, 32)
    g, x, _ = _vol(case, 0, 57 + k)
    w = torch.randn(16, 16, k, k, k, generator=g) / math.sqrt(16 * k ** 3)
    bias = torch.randn(16, generator=g)
    packs = ops.pack_conv3d(w.to(dev))
    run = lambda c: ops.conv3d_mfma(x.to(dev), packs, bias=bias.to(dev), circular=c).cpu()   # noqa: E731
    got = run(mask)
    _bound(got, F.conv3d(pad_axes(x, mask, k // 2), w, bias), F.conv3d(pad_axes(x.double(), mask, k // 2), w.double(), bias.double()))
    zero, full = run(False), run(True)
    _mixed(got, zero, full)
    assert torch.equal(run((Fa, Fa, Fa)), zero) and torch.equal(run((T, T, T)), full)


def test_conv3d_mfma_depth_one(dev, ops):
    """'A depth of at least P' is the periodic depth's precondition only."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 16, 1, 16, 32, generator=g)
    w = torch.randn(16, 16, 5, 5, 5, generator=g) / math.sqrt(16 * 125)
    packs = ops.pack_conv3d(w.to(dev))
    mask = (Fa, T, T)
    got = ops.conv3d_mfma(x.to(dev), packs, circular=mask).cpu()
    _bound(got, F.conv3d(pad_axes(x, mask, 2), w), F.conv3d(pad_axes(x.double(), mask, 2), w.double()))
    for m in ((T, Fa, Fa), (T, T, T), True):
        with pytest.raises(ValueError, match="depth of at least"):
            ops.conv3d_mfma(x.to(dev), packs, circular=m)


@pytest.mark.parametrize("mask", [(T, Fa, Fa), (Fa, T, T)], ids=_id)
def test_resblock3d_fused(dev, ops, mask):
    """The folded residual block on a volume: against fp64 and against the unfused sequence of this library's own ops."""
    torch.manual_seed(12)
    B, C, D, H, W = 1, 16, 4, 16, 32
    h = torch.randn(B, C, D, H, W, device=dev) * 1.3 - 0.2
    w1, b1, w2, b2 = (torch.randn(C, device=dev) for _ in range(4))
    v = h.double()
    mean, var = v.mean(dim=(2, 3, 4)), v.var(dim=(2, 3, 4), unbiased=False)
    tab = torch.zeros(B, ops.table_channels(C), 4, device=dev)
    tab[:, :C, 0], tab[:, :C, 1], tab[:, :C, 2] = mean.float(), (w1.double() / torch.sqrt(var + 1e-5)).float(), b1
    cw = [torch.randn(C, C, 3, 3, 3, device=dev) / (27 * C) ** 0.5 for _ in range(2)]
    cb = [torch.randn(C, device=dev) * 0.1 for _ in range(2)]
    shift = torch.randn(B, C, device=dev)
    p1, p2 = ops.pack_conv3d(cw[0]), ops.pack_conv3d(cw[1])
    run = lambda c: ops.resblock3d_fused(h, tab, p1, cb[0], shift, p2, cb[1], w2, b2, 0, circular=c).cpu()   # noqa: E731
    got = run(mask)

    def ref(dt):
        c = lambda t: t.to(dt).cpu()                                                        # noqa: E731
        a = F.silu(F.group_norm(c(h), C, c(w1), c(b1), 1e-5))
        y = F.conv3d(pad_axes(a, mask), c(cw[0]), c(cb[0])) + c(shift)[:, :, None, None, None]
        a2 = F.silu(F.group_norm(y, C, c(w2), c(b2), 1e-5))
        return F.conv3d(pad_axes(a2, mask), c(cw[1]), c(cb[1])) + c(h)
    want = ref(torch.float64)
    e, e32 = rel_l2(got, want), rel_l2(ref(torch.float32), want)
    print(f"rel_l2 {e:.3e}  torch fp32 {e32:.3e}")
    assert e <= max(3 * e32, 3e-7), (e, e32)
    # the unfused sequence
    a = F.silu(F.group_norm(h, C, w1, b1, 1e-5))
    y = ops.conv3d_mfma(a, p1, bias=cb[0], shift=shift, circular=mask)
    a2 = F.silu(F.group_norm(y, C, w2, b2, 1e-5))
    plain = ops.conv3d_mfma(a2, p2, bias=cb[1], res1=h, circular=mask).cpu()
    assert rel_l2(got, plain) <= 2e-6, rel_l2(got, plain)
    zero, full = run(False), run(True)
    _mixed(got, zero, full)
    assert torch.equal(run((Fa, Fa, Fa)), zero) and torch.equal(run((T, T, T)), full)


@pytest.mark.parametrize("dim,k,dims,bias", [(2, 3, [0], True), (2, 1, [1], True), (2, 5, [1], False), (2, 7, None, True),
                                             (3, 3, [0, 2], True), (3, 1, [1], False), (3, 5, [2], True)])
def test_circular_conv_forward(dev, dim, k, dims, bias):
    """CircularConv2d / CircularConv3d.forward against the reference's forward (F.pad per axis, then the convolution): odd
    kernels 1 - 7, with and without bias; the packed weights follow an in-place change of the weights."""
    from diffsci_amd.models.nets.commonlayers import CircularConv2d, CircularConv3d
    torch.manual_seed(40 + dim + k)
    layer = (CircularConv3d if dim == 3 else CircularConv2d)(16, 24, k, dims, bias=bias)
    x = torch.randn(2, 16, *((6, 16, 32) if dim == 3 else (20, 36)))
    conv = F.conv3d if dim == 3 else F.conv2d

    def check():
        w, b = layer.conv.weight.detach().cpu(), None if not bias else layer.conv.bias.detach().cpu()
        want = conv(pad_axes(x.double(), layer.axes, k // 2), w.double(), None if b is None else b.double())
        with torch.no_grad():
            got = layer(x.to(dev)).cpu()
        _bound(got, conv(pad_axes(x, layer.axes, k // 2), w, b), want)
        return got
    layer = layer.to(dev)
    first = check()
    with torch.no_grad():
        assert torch.equal(layer(x.to(dev)).cpu(), first)                # the cached packing
        layer.conv.weight.mul_(-0.5)
    assert rel_l2(check(), first) > 1e-1                                  # ... is not kept past a change of the weights


def test_axis_swap(dev, ops):
    """conv(x, w, circular=(T, F)) is the transpose of conv(x^T, w^T, circular=(F, T))."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 16, 24, 40, generator=g)
    w = torch.randn(24, 16, 3, 3, generator=g) / 12.0
    a = ops.conv(x.to(dev), ops.pack_conv(w.to(dev), "fp16x3"), circular=(T, Fa)).cpu()
    xt, wt = x.transpose(2, 3).contiguous(), w.transpose(2, 3).contiguous()
    b = ops.conv(xt.to(dev), ops.pack_conv(wt.to(dev), "fp16x3"), circular=(Fa, T)).cpu().transpose(2, 3)
    want = F.conv2d(pad_axes(x.double(), (T, Fa)), w.double())
    ref32 = F.conv2d(pad_axes(x, (T, Fa)), w)
    _bound(a, ref32, want)
    _bound(b, ref32, want)
    assert rel_l2(a, b) <= max(3 * rel_l2(ref32, want), 3e-7)


def test_wrong_length_and_unsupported_kernels(dev, ops):
    x = torch.randn(1, 8, 8, 32, device=dev)
    w = torch.randn(8, 8, 3, 3, device=dev)
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.conv(x, ops.pack_conv(w, "fp16x3"), circular=(T, Fa, T))
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.conv3d(x[None], torch.randn(8, 8, 3, 3, 3, device=dev), circular=(T, Fa))
    for kind in ("fp32", "bf16x6"):
        with pytest.raises(NotImplementedError, match="periodic padding"):
            ops.conv(x, ops.pack_conv(w, kind), circular=(Fa, T))
    # the C ABI refuses undefined bit combinations (DS_ERR_UNSUPPORTED = -4)
    N = ops.N
    pw = ops.pack_conv(w, "fp16x3")
    out = torch.empty_like(x)
    for word in (N.DS_PAD_ZERO_H, N.DS_PAD_CIRCULAR | N.DS_PAD_ZERO_H | N.DS_PAD_ZERO_W, N.DS_PAD_CIRCULAR | N.DS_PAD_ZERO_D):
        rc = N.lib().ds_conv2d_h3(ops._p(out), ops._p(x), ops._p(pw.data), pw.wshift, None, None, 0, None, None, 1, 8, 8, 8, 32, word,
                                  None, None, None, None, ops._stream())
        assert rc == -4, (word, rc)
    for circ in (2, 64, 1 | 64 | 128, 1 | N.DS_PAD_ZERO_D):
        rc = N.lib().ds_conv2d_direct(ops._p(out), ops._p(x), ops._p(w[:2].contiguous()), None, 1, 8, 2, 8, 32, circ, ops._stream())
        assert rc == -4, (circ, rc)


# ---------------------------------------------------------------- networks: the reference's converted nets (tools/make_circular_dims_golden.py)
from tests import test_circular_dims as HOST  # noqa: E402  (fixture loader and builders, shared with the host-side tests)


def _converted(tag, dev, dims=None):
    """This package's default network with the unconverted half of the fixture's weights, converted by this package's converter."""
    import json
    from diffsci_amd.extra import convert_conv_to_circular
    vals, sd = HOST.fixture(tag)
    net = HOST.build(tag)
    net.load_state_dict(HOST.unconverted(sd), strict=True)
    net = convert_conv_to_circular(net, json.loads(vals["circular_dims"]) if dims is None else dims)
    return vals, net.to(dev).eval()


def _referee(got, vals, f32="out_f32", f64="out_f64"):
    """The referee rule (tests/test_gpu_ldm_decoder.py): within 4 x the reference's own fp32-versus-fp64 error."""
    e, ref = rel_l2(got, vals[f64]), rel_l2(vals[f32], vals[f64])
    print(f"rel_l2 {e:.3e}  reference fp32 {ref:.3e}")
    assert e < max(4 * ref, 2e-6), (e, ref)


@pytest.mark.parametrize("tag,precision", [("pc2_h", "fp16x3"), ("pc2_w", "fp16x3"), ("pc2_k5", "fp16x3"), ("padm_h", "fp16x3"),
                                           ("pc3_dh", "fp16x3"), ("pc3_w", "fp16x3"), ("pc3_dh", "fp32"), ("pc3_w", "fp32")])
def test_converted_network(dev, tag, precision):
    """precision: fp16x3 everywhere; on volumes also "fp32", which is the direct-kernel route (ops.conv3d)."""
    vals, net = _converted(tag, dev)
    net.conv_precision = precision
    got = net(vals["x"].to(dev), vals["t"].to(dev)).cpu()
    _referee(got, vals)
    assert net.conv_precision == precision                       # no escalation on the way


@pytest.mark.parametrize("tag,dims,axis,zero_axis", [("pc2_h", [0], 2, 3), ("pc2_h", [1], 3, 2), ("padm_h", [0], 2, 3)])
def test_roll_equivariance(dev, tag, dims, axis, zero_axis):
    """Fields: rolling the input by 4 (a multiple of every level's stride) along a periodic axis rolls the output, to
    rel_l2 <= 2e-6; along a zero-padded axis it does not (> 1e-3).  No fixture: the networks of the fixtures' configurations as torch
    initialises them.  (The reference's own fp32 evaluation of these networks is equivariant to 3e-7 - 1.7e-6, so the flat bound is
    one fp32 arithmetic can meet here.  The volume network is no case of this check: two evaluations of it that sum in different
    orders are 1.4e-6 - 3.6e-6 apart, with per-axis flags as with the unchanged all-periodic network (2.4e-6 - 2.9e-6), and the
    reference's own fp32 runs 4.8e-5 - 2.8e-4.  On volumes the check is on the operators: test_roll_equivariance_volume_ops.)"""
    from diffsci_amd.extra import convert_conv_to_circular
    torch.manual_seed(77)
    net = convert_conv_to_circular(HOST.build(tag), dims, inplace=True).to(dev).eval()
    vals, _ = HOST.fixture(tag)
    x, t = vals["x"].to(dev), vals["t"].to(dev)
    y = net(x, t).clone()
    rolled = net(torch.roll(x, 4, axis).contiguous(), t).clone()
    e = rel_l2(rolled.cpu(), torch.roll(y, 4, axis).cpu())
    print(f"periodic axis {axis}: rel_l2 {e:.3e}")
    assert e <= 2e-6, e
    other = net(torch.roll(x, 4, zero_axis).contiguous(), t)
    assert rel_l2(other.cpu(), torch.roll(y, 4, zero_axis).cpu()) > 1e-3


@pytest.mark.parametrize("mask", MASKS3, ids=_id)
@pytest.mark.parametrize("route", ["conv3d_mfma", "conv3d", "resblock3d_fused"])
def test_roll_equivariance_volume_ops(dev, ops, route, mask):
    """The volume operators one by one, where nothing amplifies a rounding error: rolling the input by 4 along a periodic axis rolls
    the output to rel_l2 <= 2e-6; along a zero-padded axis it changes it by more than 1e-3."""
    torch.manual_seed(21)
    B, C, D, H, W = 1, 16, 8, 16, 32
    x = torch.randn(B, C, D, H, W, device=dev) * 1.3 - 0.2
    w = [torch.randn(C, C, 3, 3, 3, device=dev) / (27 * C) ** 0.5 for _ in range(2)]
    b = [torch.randn(C, device=dev) * 0.1 for _ in range(2)]
    if route == "conv3d":
        run = lambda v: ops.conv3d(v, w[0], bias=b[0], circular=mask)                      # noqa: E731
    elif route == "conv3d_mfma":
        packs = ops.pack_conv3d(w[0])
        run = lambda v: ops.conv3d_mfma(v, packs, bias=b[0], circular=mask)                # noqa: E731
    else:
        p1, p2 = ops.pack_conv3d(w[0]), ops.pack_conv3d(w[1])
        w1, b1, w2, b2 = (torch.randn(C, device=dev) for _ in range(4))
        v64 = x.double()
        mean, var = v64.mean(dim=(2, 3, 4)), v64.var(dim=(2, 3, 4), unbiased=False)
        tab = torch.zeros(B, ops.table_channels(C), 4, device=dev)      # a roll leaves the volume's statistics as they are
        tab[:, :C, 0], tab[:, :C, 1], tab[:, :C, 2] = mean.float(), (w1.double() / torch.sqrt(var + 1e-5)).float(), b1
        shift = torch.randn(B, C, device=dev)
        run = lambda v: ops.resblock3d_fused(v, tab, p1, b[0], shift, p2, b[1], w2, b2, 0, circular=mask)   # noqa: E731
    y = run(x).clone()
    for d, periodic in enumerate(mask):
        ax = 2 + d
        e = rel_l2(run(torch.roll(x, 4, ax).contiguous()).cpu(), torch.roll(y, 4, ax).cpu())
        print(f"axis {ax} {'periodic' if periodic else 'zero-padded'}: rel_l2 {e:.3e}")
        assert (e <= 2e-6) if periodic else (e > 1e-3), (ax, e)


def test_sampler_replans_after_conversion(dev):
    """KarrasModule.propagate_white_noise on the converted net (captured, N = 4 Heun) against the reference's end state; a second
    call replays the plan; converting again in place must not replay it."""
    import diffsci_amd.models as M
    from diffsci_amd.extra import convert_conv_to_circular
    traj, _ = HOST.fixture("pc2_traj")
    _, net = _converted("pc2_h", dev)
    mod = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).to(dev).eval()
    wn = traj["white_noise"].to(dev)
    a = mod.propagate_white_noise(wn, nsteps=4).clone()
    _referee(a.cpu(), traj, "end_f32", "end_f64")
    assert len(mod._plans.plans) == 1, "the run was not captured"
    assert torch.equal(mod.propagate_white_noise(wn, nsteps=4), a) and len(mod._plans.plans) == 1
    assert convert_conv_to_circular(mod, [1], inplace=True) is mod and net.circular_axes == (False, True)
    b = mod.propagate_white_noise(wn, nsteps=4).clone()
    _, fresh = _converted("pc2_h", dev, dims=[1])
    want = M.KarrasModule(fresh, M.KarrasModuleConfig.from_edm()).to(dev).eval().propagate_white_noise(wn, nsteps=4)
    assert torch.equal(b, want)
    assert rel_l2(b.cpu(), a.cpu()) > 1e-3
