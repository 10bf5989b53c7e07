"""The normalisation kernels on the data their comments make claims about and no other test feeds them: means that dominate
the deviation (E[x^2] - mean^2 cancels), variances below eps, constant planes, tiny and huge magnitudes; at every plane size,
alignment and chunk count where the code takes another path.  The error model and the data families: tests/norm_bounds.py
(checked on the CPU by tests/test_norm_bounds.py).  Every case prints its measured error, its bound and their ratio (pytest -s).

  a  ds_gnorm1_stats / ds_groupnorm_stats (k_g1_partial, k_g1_final): the statistics bound, 16-byte and scalar paths
  b  the apply kernels, given the kernel's own statistics: only the apply arithmetic
  c  ds_inorm_silu: every instantiation of launch_inorm with a ragged last vector row, in place, kinds 2 and 3, the image form
  d  tile statistics and norm tables of mean-dominated and tiny convolution outputs, the fused loader, the volume's slice tables
  e  ds_batchnorm_eval
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import norm_bounds as nb  # noqa: E402
from tests.norm_bounds import U, REL, rel_l2  # noqa: E402

EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


def aligned(t, dev):
    d = t.to(dev).contiguous()
    assert d.data_ptr() % 16 == 0
    return d


def shifted(t, dev):
    """The same values one float past a 16-byte boundary: torch.empty(n + 1)[1:], which every wrapper takes as contiguous."""
    v = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


PLACE = {"aligned": aligned, "shifted": shifted}


def report(what, **ratios):
    """Print error / bound ratios and assert each is at most 1."""
    print(f"{what}: " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)


def report_rel(what, err, bound=REL):
    print(f"{what}: rel-L2 {err:.2e}, bound {bound:.1e}, ratio {err / bound:.3f}")
    assert err < bound, (what, err)


def whole_samples(fam, shape, seed=0):
    """A family over whole samples: D is sample 0 exactly zero and, where the sample size is a power of two, sample 1 exactly 3."""
    x = nb.family(fam if fam != "D" else "A", shape, seed)
    if fam == "D":
        x[0] = 0.0
        if shape[0] > 1 and nb.is_pow2(x[0].numel()):
            x[1] = 3.0
    return x


def torch_images(a):
    """The pre-split image layout of the norm kernels' image forms from an fp32 tensor, with torch ops."""
    B, C, H, W = a.shape
    nch = (C + 15) // 16
    ap = torch.zeros(B, nch * 16, H + 2, W + 2, device=a.device)
    ap[:, :C, 1:-1, 1:-1] = a
    hi = ap.half()
    lo = (ap - hi.float()).half()
    v = torch.stack([hi, lo], dim=1).view(B, 2, nch, 2, 8, H + 2, W + 2).permute(0, 2, 1, 3, 5, 6, 4).contiguous()
    return v.view(torch.float32).reshape(-1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ a. the statistics kernels
# the branch of k_g1_partial each shape reaches (n = C H W per sample; a chunk is 256 threads x 64 floats)
STAT_SHAPES = {
    "one chunk, 16-byte path": ((2, 8, 16, 16), "aligned"),
    "one chunk, scalar path": ((2, 8, 16, 16), "shifted"),
    "n % 4 = 3: vector body + tail, then misaligned samples": ((3, 5, 5, 7), "aligned"),
    "two chunks, per rounded up, ragged last chunk": ((2, 6, 61, 67), "aligned"),
    "six exact chunks": ((1, 24, 64, 64), "aligned"),
    "above the chunk cap": ((1, 4, 1025, 1024), "aligned"),
}
STAT_FAMILIES = nb.FAMILIES
# the chunk cap is a property of the size, 4.2 M floats: families A and B only
STAT_CASES = [(c, f) for c in STAT_SHAPES for f in STAT_FAMILIES if STAT_SHAPES[c][0][2] < 1000 or f == "A" or f.startswith("B")]


def _check_gnorm1_stats(ops, xd, x, eps, what):
    B = x.shape[0]
    st0 = ops.gnorm1_stats(xd, 0, eps=eps).cpu()
    st1 = ops.gnorm1_stats(xd, 1, eps=eps).cpu()
    assert torch.isfinite(st0).all() and torch.isfinite(st1).all()
    s = nb.Stats(x.reshape(B, -1), eps, 2, True)
    assert not st1[:, 0].any()
    report(what, mean=s.mean_ratio(st0[:, 0]), rstd=s.rstd_ratio(st0[:, 1]), rms=s.rms_ratio(st1[:, 1]))
    return st0, s


@pytest.mark.parametrize("case,fam", STAT_CASES)
def test_gnorm1_stats(dev, ops, case, fam):
    shape, place = STAT_SHAPES[case]
    x = whole_samples(fam, shape)
    st, s = _check_gnorm1_stats(ops, PLACE[place](x, dev), x, EPS, f"gnorm1_stats {shape} {place} {fam}")
    if place == "shifted":                    # the same tensor, the other path: the two results agree within the bound
        sa = ops.gnorm1_stats(aligned(x, dev), 0, eps=EPS).cpu()
        dm = ((sa[:, 0].double() - st[:, 0].double()).abs() / (2 * s.dm).clamp_min(1e-300)).max()
        dr = ((sa[:, 1].double() / st[:, 1].double() - 1).abs() / (2 * s.rho)).max()
        report(f"gnorm1_stats {shape} aligned against shifted {fam}", mean=float(dm), rstd=float(dr))


@pytest.mark.parametrize("fam", STAT_FAMILIES)
@pytest.mark.parametrize("shape,G", [((2, 32, 12, 12), 1), ((2, 32, 12, 12), 8), ((2, 32, 12, 12), 32), ((1, 6, 5, 7), 3)])
def test_groupnorm_stats(dev, ops, shape, G, fam):
    """(1, 6, 5, 7) with G = 3: groups of 70 floats start aligned and misaligned in turn."""
    x = nb.family(fam, shape, seed=G)
    st = ops.groupnorm_stats(aligned(x, dev), G, eps=1e-6).cpu()
    assert torch.isfinite(st).all()
    s = nb.Stats(x.reshape(shape[0], G, -1), 1e-6, 2, True)
    report(f"groupnorm_stats {shape} G={G} {fam}", mean=s.mean_ratio(st[..., 0]), rstd=s.rstd_ratio(st[..., 1]))


# ------------------------------------------------------------------------------------------------ b. the apply kernels
APPLY_FAMILIES = ("B1e3", "C", "E40", "E1e-7")
APPLY_SHAPES = [((2, 8, 8, 16), "aligned"), ((2, 5, 6, 6), "aligned"), ((2, 8, 8, 16), "shifted")]


def _gnorm1_ref(x, st, w, b, kind, film):
    """fp64 evaluation of k_g1_apply's formula with the fp32 statistics the kernel was given."""
    C = x.shape[1]
    x, st = x.double(), st.double()
    m, sd = st[:, 0, None, None, None], st[:, 1, None, None, None]
    w, b = w.double()[None, :, None, None], b.double()[None, :, None, None]
    v = (x - m) * sd * w + b if kind == 0 else x / sd * w + b
    if film is not None:
        f = film.double().expand(x.shape[0], 2 * C)
        v = v * f[:, :C, None, None] + f[:, C:, None, None]
    return nb.silu64(v)


@pytest.mark.parametrize("fam", APPLY_FAMILIES)
@pytest.mark.parametrize("shape,place", APPLY_SHAPES)
def test_gnorm1_apply_kernels(dev, ops, shape, place, fam):
    B, C, H, W = shape
    x = nb.family(fam, shape, seed=3)
    g = torch.Generator().manual_seed(17)
    w, b, film = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, 2 * C, generator=g) * 0.5
    xd, wd, bd = PLACE[place](x, dev), w.to(dev), b.to(dev)
    for kind in (0, 1):
        st = ops.gnorm1_stats(xd, kind, eps=EPS)
        for fl in (None, film, film[:1]):
            fd = None if fl is None else fl.contiguous().to(dev)
            act = _gnorm1_ref(x, st.cpu(), w, b, kind, fl)
            tag = f"{shape} {place} {fam} kind {kind} film {None if fl is None else tuple(fl.shape)}"
            plain = ops.gnorm1_apply(xd, st, wd, bd, kind, film=fd)
            assert torch.isfinite(plain).all()
            report_rel(f"gnorm1_apply {tag}", rel_l2(plain.cpu(), act))
            pooled = ops.gnorm1_apply(xd, st, wd, bd, kind, pool=True, film=fd)
            report_rel(f"gnorm1_apply pool {tag}", rel_l2(pooled.cpu(), F.avg_pool2d(act, 2)))
            for f in (2, 3, 4):
                got = ops.gnorm1_apply_poolf(xd, st, wd, bd, kind, f, film=fd)
                report_rel(f"gnorm1_apply_poolf {f} {tag}", rel_l2(got.cpu(), F.avg_pool2d(act, f)))
                if f == 2:
                    assert torch.equal(got, pooled)                  # the same window order
            for pool, ref in ((False, plain), (True, pooled)):       # the image form: gnorm1_apply's values, bit for bit
                img = ops.gnorm1_apply_images(xd, st, wd, bd, kind, pool=pool, film=fd)
                assert same_bits(img, torch_images(ref)), (tag, pool)
    assert torch.equal(ops.gnorm1_apply(xd, None, None, None, 2), xd)


@pytest.mark.parametrize("fam", APPLY_FAMILIES)
@pytest.mark.parametrize("shape,place", APPLY_SHAPES)
def test_groupnorm_apply(dev, ops, shape, place, fam):
    B, C, H, W = shape
    G = 4 if C % 4 == 0 else C
    x = nb.family(fam, shape, seed=5)
    g = torch.Generator().manual_seed(19)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xd, wd, bd = PLACE[place](x, dev), w.to(dev), b.to(dev)
    st = ops.groupnorm_stats(xd, G, eps=1e-6)
    s64 = st.cpu().double().repeat_interleave(C // G, 1)
    v = (x.double() - s64[:, :, 0, None, None]) * s64[:, :, 1, None, None] * w.double()[None, :, None, None] \
        + b.double()[None, :, None, None]
    for act in (False, True):
        am = ops.amax_new(B, dev)
        got = ops.groupnorm_apply(xd, st, wd, bd, G, act=act, out_amax=am)
        assert torch.isfinite(got).all()
        report_rel(f"groupnorm_apply {shape} {place} {fam} act={act}", rel_l2(got.cpu(), nb.silu64(v) if act else v))
        assert torch.equal(am.view(torch.float32), got.reshape(B, -1).abs().amax(1))
        assert torch.equal(ops.groupnorm_apply(xd, st, wd, bd, G, act=act), got)


# ------------------------------------------------------------------------------------------------ c. ds_inorm_silu
# H x W -> the instantiation of launch_inorm; hw4 = H W / 4 is no multiple of the thread count, so the masked tail lanes matter
INORM_PLANES = {
    (4, 4): "wave, VPT 1", (16, 16): "wave, VPT 1 (full lanes)", (12, 24): "wave, VPT 2", (20, 36): "wave, VPT 4",
    (32, 40): "wave, VPT 8", (48, 52): "wave, VPT 16", (72, 80): "block 256, VPT 8", (100, 100): "block 256, VPT 16",
    (136, 140): "block 1024, VPT 8", (200, 204): "block 1024, VPT 16", (33, 33): "generic: HW % 4 != 0",
    (260, 256): "generic: HW > 65536", (20, 36, "shifted"): "generic: misaligned",
}
INORM_FAMILIES = ("A", "B1e3", "C", "D", "E40", "E1e-7")


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


@pytest.mark.parametrize("fam", INORM_FAMILIES)
@pytest.mark.parametrize("plane", list(INORM_PLANES), ids=lambda p: "x".join(str(v) for v in p))
def test_inorm_silu_every_instantiation(dev, ops, plane, fam):
    """B C = 6 planes: the wave kernel's last workgroup is partial and c = plane % C is exercised."""
    H, W = plane[:2]
    place = PLACE[plane[2] if len(plane) > 2 else "aligned"]
    x = nb.family(fam, (2, 3, H, W), seed=H)
    w, b = _affine(3, W)
    xd, wd, bd = place(x, dev), w.to(dev), b.to(dev)
    tag = f"inorm_silu {H}x{W} [{INORM_PLANES[plane]}] {fam}"
    x2 = x.reshape(2, 3, H * W)
    w2, b2 = w.double()[None, :, None], b.double()[None, :, None]
    # kind 0: the element bound
    got = ops.inorm_silu(xd, wd, bd, 0, eps=EPS)
    assert torch.isfinite(got).all()
    st = nb.Stats(x2, EPS, nb.k_tree(H * W), False)
    ratio, err = nb.element_ratio(got.cpu().reshape(2, 3, -1), x2, st, w2, b2)
    print(f"{tag} kind 0: max error {err:.3e}")
    report(f"{tag} kind 0", element=ratio)
    if fam == "D":                                                     # var = 0: SiLU(b[c]) whatever rstd is
        flat = got.cpu().reshape(2, 3, -1)
        const = (x2 == x2[..., :1]).all(-1)
        assert const.sum() >= 3
        want = F.silu(b.double())[None, :, None].expand_as(flat)
        assert ((flat.double() - want).abs()[const] <= 8 * U * (want.abs() + b2.abs().expand_as(flat))[const]).all()
    # kind 1: no subtraction, the project's rel-L2 bound
    got1 = ops.inorm_silu(xd, wd, bd, 1, eps=EPS)
    assert torch.isfinite(got1).all()
    want1 = nb.silu64(x2.double() / st.rms_den[..., None] * w2 + b2)
    report_rel(f"{tag} kind 1", rel_l2(got1.cpu().reshape(2, 3, -1), want1))
    # in place: the same launch with out = x
    for kind, ref in ((0, got), (1, got1)):
        xi = place(x, dev)
        assert ops.inorm_silu(xi, wd, bd, kind, eps=EPS, out=xi) is xi
        assert torch.equal(xi, ref), (tag, kind, "in place")


@pytest.mark.parametrize("fam", INORM_FAMILIES)
@pytest.mark.parametrize("plane", [(4, 4), (20, 36), (33, 33), (260, 256)], ids=lambda p: "x".join(str(v) for v in p))
def test_pointwise_kinds(dev, ops, plane, fam):
    """Kinds 2 (SiLU alone) and 3 (GroupPixNorm(C, C) + SiLU) of ds_inorm_silu (k_pointwise_silu); 260 x 256 passes its cap of 64
    workgroups per plane.  Kind 3 has the slope w / sqrt(eps) = 316 w at zero: the tiny families."""
    H, W = plane
    x = nb.family(fam, (2, 3, H, W), seed=H + 1)
    w, b = _affine(3, W + 1)
    xd = aligned(x, dev)
    xx, w2, b2 = x.double(), w.double()[None, :, None, None], b.double()[None, :, None, None]
    got2 = ops.inorm_silu(xd, None, None, 2)
    got3 = ops.inorm_silu(xd, w.to(dev), b.to(dev), 3, eps=EPS)
    assert torch.isfinite(got2).all() and torch.isfinite(got3).all()
    report_rel(f"inorm_silu {H}x{W} {fam} kind 2", rel_l2(got2.cpu(), nb.silu64(xx)))
    report_rel(f"inorm_silu {H}x{W} {fam} kind 3", rel_l2(got3.cpu(), nb.silu64(xx / torch.sqrt(xx * xx + EPS) * w2 + b2)))


@pytest.mark.parametrize("fam", ["A", "B1e3", "C"])
@pytest.mark.parametrize("plane", [(8, 8), (16, 24), (20, 36), (48, 40), (64, 64)], ids=lambda p: "x".join(str(v) for v in p))
def test_inorm_silu_images_values(dev, ops, plane, fam):
    """The image form's values are ds_inorm_silu's, bit for bit; and, on their own, they meet the bounds of ds_inorm_silu
    (read back as hi + lo, two fp16 pieces: 2^-22 |v| for the low piece's rounding and 2^-25 for its subnormal spacing).

    Both forms reduce a plane of up to 4096 floats, all the image form takes, with one wave and k_inorm_wave's summation
    order.  48 x 40 and 64 x 64 are the sizes at which ds_inorm_silu used to switch to k_inorm_block (256 threads, the waves'
    sums added through LDS): another correct fp32 tree, after which 810 to 5774 image words differed on families A and B(1e3)
    (decoded rel-L2 up to 2.4e-5 on B(1e3), an ulp of a mean near 1000 against deviations of order one)."""
    H, W = plane
    x = nb.family(fam, (2, 3, H, W), seed=H + 2)
    w, b = _affine(3, W + 2)
    xd, wd, bd = aligned(x, dev), w.to(dev), b.to(dev)
    x2, w2, b2 = x.reshape(2, 3, H * W), w.double()[None, :, None], b.double()[None, :, None]
    st = nb.Stats(x2, EPS, nb.k_tree(H * W), False)
    differ = {}
    for kind in (0, 1):
        act = ops.inorm_silu(xd, wd, bd, kind, eps=EPS)
        img = ops.inorm_silu_images(xd, wd, bd, kind, eps=EPS)
        want = torch_images(act)
        differ[kind] = int((img.view(torch.int32) != want.view(torch.int32)).sum())
        v = img.view(torch.float16).view(2, 1, 2, 2, H + 2, W + 2, 8).double()
        dec = (v[:, :, 0] + v[:, :, 1]).permute(0, 1, 2, 5, 3, 4).reshape(2, 16, H + 2, W + 2)
        assert not dec[:, 3:].any() and not dec[:, :, 0].any() and not dec[:, :, -1].any()          # channel padding, border
        assert not dec[:, :, :, 0].any() and not dec[:, :, :, -1].any()
        vals = dec[:, :3, 1:-1, 1:-1].cpu()
        tag = f"inorm_silu_images {H}x{W} {fam} kind {kind}"
        print(f"{tag}: {differ[kind]} of {img.numel()} words differ, decoded values against inorm_silu: "
              f"rel-L2 {rel_l2(vals, act.cpu()):.2e}")
        if kind == 0:
            report(tag, element=nb.element_ratio(vals.reshape(2, 3, -1), x2, st, w2, b2, slack_rel=2.0 ** -22, slack_abs=2.0 ** -25)[0])
        else:
            report_rel(tag, rel_l2(vals.reshape(2, 3, -1), nb.silu64(x2.double() / st.rms_den[..., None] * w2 + b2)), REL + 2.0 ** -22)
    assert differ == {0: 0, 1: 0}, (plane, fam, differ)


# ------------------------------------------------------------------------------------------------ d. tile statistics and tables
def _tile_sums(ts):
    """(K, S, Q, n) per tile -> sums of x and x^2 and the count per (sample, channel), in fp64."""
    K, S, Q, n = ts.cpu().double().unbind(-1)
    return (n * K + S).sum(-1), (Q + 2 * K * S + n * K * K).sum(-1), n.sum(-1)


def _check_rows(what, tab, s, w64, kind, c_want=None):
    """Table rows [..., 0:3] of channels against the statistics s (shape of tab[..., 0]): M to the mean bound (k_m = 2), A to 1e-5."""
    M, A = tab[..., 0].double(), tab[..., 1].double()
    if kind == 0:
        a_want, m_ratio = s.rstd * w64, s.mean_ratio(tab[..., 0])
    else:
        a_want, m_ratio = w64 / s.rms_den, 0.0
        assert not M.any()
    a_err = float(((A - a_want).abs() / a_want.abs().clamp_min(1e-300)).max())
    print(f"{what}: A relative error {a_err:.2e}, bound 1.0e-05")
    report(what, M=m_ratio, A=a_err / 1e-5)
    if c_want is not None:
        assert torch.equal(tab[..., 2], c_want)


def _check_exponent(what, tab, y64, C):
    """Fourth column with the kernel's own rows: 2^-k, one per sample, max |(y - M) A + C| 2^k below 2^14, and above 2^5 unless
    |k| <= 80 clamps."""
    t = tab.cpu().double()
    inv = t[..., 3]
    assert (inv == inv[:, :1]).all() and (torch.log2(inv[:, 0]) % 1 == 0).all()
    t = t[:, :C]
    arg = ((y64 - t[..., 0, None, None]) * t[..., 1, None, None] + t[..., 2, None, None]).abs().amax(dim=(1, 2, 3))
    scaled, k = arg / inv[:, 0], -torch.log2(inv[:, 0])
    print(f"{what}: k = {k.tolist()}, max |arg| 2^k = 2^{[round(math.log2(max(float(v), 1e-300)), 2) for v in scaled]}")
    assert (scaled < 2.0 ** 14).all(), what
    assert ((scaled > 2.0 ** 5) | (k.abs() == 80)).all(), what


def _producers(ops, dev, B, C, H, W, small):
    """y = conv(x) + 1000 (mean-dominated), or with weights scaled by 2^-40 and no offset (tiny): the 3x3 and the 1x1 kernel,
    each leaving tile statistics."""
    g = torch.Generator().manual_seed(B + C + H + W)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    scale = 2.0 ** -40 if small else 1.0
    bias = None if small else torch.full((C,), 1000.0, device=dev)
    out = []
    for k in (3, 1):
        wt = torch.randn(C, C, k, k, generator=g) / math.sqrt(C * k * k) * scale
        ts = torch.full((B, C, ops.conv_tile_count(H, W), 4), float("nan"), device=dev)
        y = ops.conv(x, ops.pack_conv(wt.to(dev), "fp16x3"), bias=bias, tile_stats=ts)
        assert torch.isfinite(ts).all() and torch.isfinite(y).all()
        out.append((y, ts))
    return out


@pytest.mark.parametrize("small", [False, True], ids=["offset 1000", "scale 2^-40"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 32), (1, 40, 20, 36)])
def test_tile_statistics_and_tables(dev, ops, shape, small):
    B, C, H, W = shape
    n = H * W
    (y3, ts3), (y1, ts1) = _producers(ops, dev, B, C, H, W, small)
    g = torch.Generator().manual_seed(23)
    w, b, film = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, 2 * C, generator=g) * 0.5
    wd, bd, fd = w.to(dev), b.to(dev), film.to(dev)
    for name, y, ts in (("3x3", y3, ts3), ("1x1", y1, ts1)):
        tag = f"tiles {shape} {'tiny' if small else 'offset'} {name}"
        yc = y.cpu().double()
        sx, sxx, cnt = _tile_sums(ts)
        assert torch.equal(cnt, torch.full_like(cnt, n))
        # plane and sample variances recombined from the tiles
        for what, v_got, v_want in (("plane", sxx / n - (sx / n) ** 2, yc.var(dim=(2, 3), unbiased=False)),
                                    ("sample", sxx.sum(1) / (C * n) - (sx.sum(1) / (C * n)) ** 2, yc.var(dim=(1, 2, 3), unbiased=False))):
            err = float(((v_got - v_want).abs() / v_want).max())
            print(f"{tag}: {what} variance from the tiles, relative error {err:.2e}, bound 1.0e-05")
            assert err <= 1e-5, (tag, what, err)
        planes = nb.Stats(yc.reshape(B, C, n), EPS, 2, True)
        sample = nb.Stats(yc.reshape(B, C * n), EPS, 2, True)
        for kind in (0, 1):
            tab = ops.inorm_table(ts, wd, bd, kind, n, eps=EPS)
            assert not tab[:, C:, :3].any()
            _check_rows(f"{tag} inorm_table kind {kind}", tab[:, :C].cpu(), planes, w.double()[None, :], kind, b.expand(B, C))
            _check_exponent(f"{tag} inorm_table kind {kind}", tab, yc, C)
            for fl in (None, fd):
                tab = ops.gnorm1_table(ts, wd, bd, kind, C * n, film=fl, eps=EPS)
                t1 = film[:, :C] if fl is not None else torch.ones(B, C)
                t2 = film[:, C:] if fl is not None else torch.zeros(B, C)
                rows = nb.Stats(yc.reshape(B, 1, C * n), EPS, 2, True)                   # one row of statistics per sample
                what = f"{tag} gnorm1_table kind {kind} film {fl is not None}"
                _check_rows(what, tab[:, :C].cpu(), rows, (w * t1).double(), kind, (b * t1 + t2) if fl is not None else b.expand(B, C))
                _check_exponent(what, tab, yc, C)
            # the statistics from the tiles against a pass over the tensor: the two routes of ADM's norms
            st_t = ops.gnorm1_stats_tiles(ts, kind, C * n, eps=EPS).cpu()
            st_x = ops.gnorm1_stats(y, kind, eps=EPS).cpu()
            if kind == 0:
                rt = float(((st_t[:, 1].double() / sample.rstd - 1).abs() / 1e-5).max())
                report(f"{tag} gnorm1_stats_tiles", mean=sample.mean_ratio(st_t[:, 0]), rstd=rt)
                report(f"{tag} gnorm1_stats", mean=sample.mean_ratio(st_x[:, 0]), rstd=sample.rstd_ratio(st_x[:, 1]))
                dm = float(((st_t[:, 0].double() - st_x[:, 0].double()).abs() / (2 * sample.dm)).max())
                dr = float(((st_t[:, 1].double() / st_x[:, 1].double() - 1).abs() / (sample.rho + 1e-5)).max())
                report(f"{tag} gnorm1_stats against gnorm1_stats_tiles", mean=dm, rstd=dr)
            else:
                assert not st_t[:, 0].any() and not st_x[:, 0].any()
                dr = float(((st_t[:, 1].double() / st_x[:, 1].double() - 1).abs() / (nb.RHO0 + 1e-5)).max())
                report(f"{tag} gnorm1_stats against gnorm1_stats_tiles, kind 1", rms=sample.rms_ratio(st_x[:, 1]), agree=dr)
        # GroupNorm(G, C): statistics from the tiles, table from the tiles and from plain statistics
        G = C // 4
        grp = nb.Stats(yc.reshape(B, G, 4 * n), 1e-6, 2, True)
        gt = ops.groupnorm_stats_tiles(ts, G, n, eps=1e-6).cpu()
        report(f"{tag} groupnorm_stats_tiles", mean=grp.mean_ratio(gt[..., 0]),
               rstd=float(((gt[..., 1].double() / grp.rstd - 1).abs() / 1e-5).max()))
        rows = nb.Stats(yc.reshape(B, G, 1, 4 * n).expand(B, G, 4, 4 * n).reshape(B, C, 4 * n), 1e-6, 2, True)
        for src, tab in (("tiles", ops.groupnorm_table(wd, bd, G, n, tile_stats=ts, eps=1e-6)),
                         ("stats", ops.groupnorm_table(wd, bd, G, n, stats=ops.groupnorm_stats(y, G, eps=1e-6), eps=1e-6))):
            _check_rows(f"{tag} groupnorm_table from {src}", tab[:, :C].cpu(), rows, w.double()[None, :], 0, b.expand(B, C))
            _check_exponent(f"{tag} groupnorm_table from {src}", tab, yc, C)
    # two sources: the statistics of a channel concatenation
    ycat = torch.cat([y3, y1], 1).cpu().double()
    w2, b2 = torch.cat([w, -w]), torch.cat([b, b + 1])
    both = nb.Stats(ycat.reshape(B, 1, 2 * C * n), EPS, 2, True)
    for kind in (0, 1):
        tab = ops.gnorm1_table(ts3, w2.to(dev), b2.to(dev), kind, 2 * C * n, stats_b=ts1, eps=EPS)
        what = f"tiles {shape} {'tiny' if small else 'offset'} gnorm1_table of two sources kind {kind}"
        _check_rows(what, tab[:, :2 * C].cpu(), both, w2.double()[None, :], kind, b2.expand(B, 2 * C))
        _check_exponent(what, tab, ycat, 2 * C)


@pytest.mark.parametrize("small", [False, True], ids=["offset 1000", "scale 2^-40"])
@pytest.mark.parametrize("mode", [0, 2], ids=["plain load", "upsampling load"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 32), (1, 40, 20, 36)])
def test_fused_loader_on_such_outputs(dev, ops, shape, mode, small):
    """conv(y, prenorm = table) against fp64 conv(SiLU((y - M) A + C)) evaluated from the table as it was read back."""
    B, C, H, W = shape
    (y, ts), _ = _producers(ops, dev, B, C, H, W, small)
    g = torch.Generator().manual_seed(29)
    w, b = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    wt = torch.randn(8, C, 3, 3, generator=g) / math.sqrt(9 * C)
    pw = ops.pack_conv(wt.to(dev), "fp16x3")
    up = (lambda t: F.interpolate(t, scale_factor=2.0, mode="nearest")) if mode == 2 else (lambda t: t)
    yc = y.cpu().double()
    tables = [(f"inorm_table kind {k}", ops.inorm_table(ts, w, b, k, H * W, eps=EPS)) for k in (0, 1)]
    tables += [(f"gnorm1_table kind {k}", ops.gnorm1_table(ts, w, b, k, C * H * W, eps=EPS)) for k in (0, 1)]
    tables.append(("groupnorm_table", ops.groupnorm_table(w, b, C // 4, H * W, tile_stats=ts, eps=1e-6)))
    for name, tab in tables:
        t = tab[:, :C].cpu().double()
        act = nb.silu64((yc - t[..., 0, None, None]) * t[..., 1, None, None] + t[..., 2, None, None])
        want = F.conv2d(up(act), wt.double(), padding=1)
        got = ops.conv(y, pw, load_mode=mode, prenorm=tab)
        assert torch.isfinite(got).all()
        report_rel(f"fused loader {shape} mode {mode} {'tiny' if small else 'offset'} {name}", rel_l2(got.cpu(), want), 3e-6)


class _Pool:
    """A buffer pool that keeps what it handed out, so the block's intermediates can be read afterwards."""

    def __init__(self):
        self.taken = []

    def take(self, shape, device):
        t = torch.empty(shape, dtype=torch.float32, device=device)
        self.taken.append(t)
        return t

    def give(self, t):
        pass


def test_volume_slice_tables(dev, ops):
    """k_slice_tables (ds_conv3d.hip) recombines tile statistics once more.  A folded residual block on a volume whose first
    convolution adds 1000: the intermediate S2 = conv1(SiLU(norm1(h))) + 1000 is mean-dominated, and its norm is known only
    through the slice table.  The table against S2's fp64 statistics; conv2 with the fused loader against fp64 from the table as
    read back; the block against the unfolded route (standalone norms), whose own fp32 mean is off by its tree's rounding."""
    B, C, D, H, W = 1, 16, 4, 8, 32
    n = D * H * W
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, C, D, H, W, generator=g).to(dev)
    wts = [torch.randn(C, C, 3, 3, 3, generator=g) / math.sqrt(27 * C) for _ in range(3)]
    packs = [ops.pack_conv3d(t.to(dev)) for t in wts]
    offset = torch.full((C,), 1000.0, device=dev)
    w1, b1, w2, b2 = (torch.randn(C, generator=g).to(dev) for _ in range(4))
    bias2 = torch.randn(C, generator=g).to(dev)
    # the producer of the block's input leaves volume statistics of a mean-dominated h
    st = torch.empty(B, C, ops.volume_stat_tiles(D, H * W), 4, device=dev)
    h = ops.conv3d_mfma(x, packs[0], bias=offset, out_stats=st)
    hc = h.cpu().double()
    hs = nb.Stats(hc.reshape(B, C, n), EPS, 2, True)
    for kind in (0, 1):
        tab1 = ops.inorm_table(st, w1, b1, kind, n, eps=EPS)
        _check_rows(f"volume statistics, inorm_table kind {kind}", tab1[:, :C].cpu(), hs, w1.cpu().double()[None, :], kind)
    tab1 = ops.inorm_table(st, w1, b1, 0, n, eps=EPS)
    for kind2 in (0, 1):
        pool = _Pool()
        out = ops.resblock3d_fused(h, tab1, packs[1], offset, None, packs[2], bias2, w2, b2, kind2, ws=pool, eps=EPS)
        s3, s2, ts, tab2 = pool.taken[:4]
        assert tuple(tab2.shape) == (B * (D + 2), 16, 4) and tuple(s2.shape) == (D + 2, C, H, W)
        assert not tab2[0].any() and not tab2[D + 1].any()                            # pad slices: zero rows
        assert all(torch.equal(tab2[1 + d, :, :3], tab2[1, :, :3]) for d in range(D))  # one row per channel and sample
        s2c = s2[1:D + 1].cpu().double()                                               # [D, C, H, W]
        ss = nb.Stats(s2c.permute(1, 0, 2, 3).reshape(1, C, n), EPS, 2, True)
        _check_rows(f"slice tables kind {kind2}", tab2[1:2, :C].cpu(), ss, w2.cpu().double()[None, :], kind2,
                    b2.cpu()[None, :])
        t = tab2[1, :C].cpu().double()
        act = nb.silu64((s2c - t[None, :, 0, None, None]) * t[None, :, 1, None, None] + t[None, :, 2, None, None])
        want3 = F.conv3d(act.permute(1, 0, 2, 3)[None], wts[2].double(), bias2.cpu().double(), padding=1)
        got3 = s3[1:D + 1].permute(1, 0, 2, 3)[None]
        report_rel(f"slice tables kind {kind2}: conv2 with the fused loader", rel_l2(got3.cpu(), want3), 3e-6)
        assert torch.equal(out, got3 + h)
        # the unfolded route
        a1 = ops.inorm_silu(h, w1, b1, 0, eps=EPS)
        u2 = ops.conv3d_mfma(a1, packs[1], bias=offset, in_amax=ops.NORMALISED)
        a2 = ops.inorm_silu(u2, w2, b2, kind2, eps=EPS)
        plain = ops.conv3d_mfma(a2, packs[2], bias=bias2, res1=h, in_amax=ops.NORMALISED)
        report_rel(f"slice tables kind {kind2}: the block, folded against unfolded", rel_l2(out.cpu(), plain.cpu()), 3e-6)
        # conv2's part alone, without the residual of 1000 that hides it.  The RMS kind has no mean and is held to the same 3e-6;
        # under kind 0 each route rounds S2's mean (near 1000) to fp32 on its own -- the table once, the standalone norm through
        # its tree -- and (x - mean) rstd of a deviation of order one moves by ulp(1000) rstd: the figure is printed, the checks
        # against fp64 above are what pins the folded route
        d = rel_l2(got3, ops.conv3d_mfma(a2, packs[2], bias=bias2, in_amax=ops.NORMALISED))
        if kind2 == 1:
            report_rel("slice tables kind 1: conv2 alone, folded against unfolded", d, 3e-6)
        else:
            print(f"slice tables kind 0: conv2 alone, folded against unfolded: rel-L2 {d:.2e} (ulp(1000) rstd = "
                  f"{float(2.0 ** -14 * ss.rstd.max()):.1e})")


# ------------------------------------------------------------------------------------------------ e. ds_batchnorm_eval
def _bn64(x, mean, var, w, b, eps, sigma, inverse):
    """The kernel header's operation order in fp64; statistics broadcast over dim 1."""
    shp = [1, -1] + [1] * (x.dim() - 2)
    m, sd = mean.double().view(shp), torch.sqrt(var.double() + eps).view(shp)
    v = x.double()
    if not inverse:
        v = (v - m) / sd
        if w is not None:
            v = v * w.double().view(shp) + b.double().view(shp)
        return v * sigma
    v = v / sigma
    if w is not None:
        v = (v - b.double().view(shp)) / w.double().view(shp)
    return v * sd + m


@pytest.mark.parametrize("fam", ["A", "B1e3"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 33), (2, 4, 4, 4, 4)])
def test_batchnorm_eval(dev, ops, shape, fam):
    C = shape[1]
    x = nb.family(fam, shape, seed=7)
    xd = aligned(x, dev)
    g = torch.Generator().manual_seed(37)
    for nc in (1, C):
        mean = torch.randn(nc, generator=g) * 0.3 + (1000.0 if fam == "B1e3" else 0.7)
        var = torch.rand(nc, generator=g) * 2 + 0.5
        weight, bias = torch.rand(nc, generator=g) + 0.5, torch.randn(nc, generator=g) * 0.2
        md, vd, wd, bd = (t.to(dev) for t in (mean, var, weight, bias))
        for affine in (False, True):
            wa, ba = (weight, bias) if affine else (None, None)
            wda, bda = (wd, bd) if affine else (None, None)
            for sigma in (1.0, 0.5):
                tag = f"batchnorm_eval {shape} {fam} nc={nc} affine={affine} sigma={sigma}"
                fwd = ops.batchnorm_eval(xd, md, vd, wda, bda, eps=EPS, sigma=sigma)
                want = _bn64(x, mean, var, wa, ba, EPS, sigma, False)
                back = ops.batchnorm_eval(fwd, md, vd, wda, bda, eps=EPS, sigma=sigma, inverse=True)
                inv = ops.batchnorm_eval(xd, md, vd, wda, bda, eps=EPS, sigma=sigma, inverse=True)
                assert torch.isfinite(fwd).all() and torch.isfinite(back).all()
                e_f = rel_l2(fwd.cpu(), want)
                e_i = rel_l2(inv.cpu(), _bn64(x, mean, var, wa, ba, EPS, sigma, True))
                m_abs = mean.abs().view([1, -1] + [1] * (x.dim() - 2))
                rt = float(((back.cpu().double() - x.double()).abs() / (4 * U * (x.double().abs() + m_abs))).max())
                print(f"{tag}: forward rel-L2 {e_f:.2e}, inverse rel-L2 {e_i:.2e} (bound {REL:.1e}); "
                      f"inverse(forward(x)) error / bound = {rt:.3f}")
                assert e_f < REL and e_i < REL, (tag, e_f, e_i)
                assert rt <= 1.0, (tag, rt)
