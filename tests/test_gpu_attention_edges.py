"""The attention kernels with a head axis (k_attn3h<*, *, MH = true>, ds_attn3h.hip) and the two exact-fp32 generic kernels
(k_attn_heads_generic, ds_attn3h.hip; k_attn_generic, ds_small.hip) at their edges: head width 256 under a head axis, sequence
lengths that leave waves of the last query block without queries, ragged lengths and odd head widths on the generic kernel, the
48-64 KiB window of the generic kernels' dynamic LDS with its cap, heads of very different magnitude inside one sample, logits
that climb tile by tile (the deferred rescale), and a max-abs bound for the shapes test_gpu_attention_heads.py checks in rel-L2.

Reference: fp64 softmax(Q K^T / sqrt(d)) V on the per-head split.  Bound, per (sample, head) row (check_kernel of
test_gpu_convit.py): rel-L2 <= max(4 x torch-CPU fp32's rel-L2 on the same input, 1e-7) and max-abs <= max(4 x torch fp32's
max-abs, one fp32 ulp of the row's max |ref|).  Every case prints its worst row: the measured pair, torch's pair and the ratios.

Forms: "staged" is ds_attention_h3_heads without a workspace (every workgroup splits its K / V tiles), "image" the same entry
point with the workspace (k_attn_images + LDS-DMA staging); both are called directly because ops.attention picks one by L.  Where
ops chooses, the choice is asserted through attention_workspace_floats."""
import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import rel_l2

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
BIG = 3e38                                           # a slot value no output exceeds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


@pytest.fixture(scope="module")
def N():
    from diffsci_amd import _native as N
    return N


def _sdpa(qkv, E, H, dtype, qidx=None):
    """torch's attention on the per-head split of channel-major qkv [B, 3E, L] -> [B, E, L] (or [B, E, len(qidx)]: the queries
    qidx against all keys)."""
    B, _, L = qkv.shape
    q, k, v = (t.to(dtype).reshape(B, H, E // H, L).transpose(-1, -2) for t in qkv.split(E, dim=1))
    if qidx is not None:
        q = q[:, :, qidx]
    return F.scaled_dot_product_attention(q, k, v).transpose(-1, -2).reshape(B, E, -1)


def check_rows(what, got, qkv, E, H, qidx=None):
    """The kernel bound on every (sample, head) row of got [B, E, L]; prints the row with the largest ratio to its bound."""
    got = got.detach().cpu()
    want = _sdpa(qkv, E, H, torch.float64, qidx)
    t32 = _sdpa(qkv, E, H, torch.float32, qidx)
    if qidx is not None:
        got = got[:, :, qidx]
    assert got.shape == want.shape
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    B, d = got.shape[0], E // H
    rows = lambda t: t.reshape(B * H, d, -1)
    bad, worst = [], None
    for r, (g, t, w) in enumerate(zip(rows(got), rows(t32), rows(want))):
        e_rel, t_rel = rel_l2(g, w), rel_l2(t, w)
        e_abs, t_abs = float((g.double() - w).abs().max()), float((t.double() - w).abs().max())
        b_rel, b_abs = max(4 * t_rel, 1e-7), max(4 * t_abs, ULP * float(w.abs().max()))
        ratio = max(e_rel / b_rel, e_abs / b_abs)
        if worst is None or ratio > worst[0]:
            worst = (ratio, r, e_rel, t_rel, e_abs, t_abs)
        if e_rel > b_rel or e_abs > b_abs:
            bad.append(f"row (b={r // H}, h={r % H}): rel-L2 {e_rel:.3e} > {b_rel:.3e} or max-abs {e_abs:.3e} > {b_abs:.3e}")
    _, r, e_rel, t_rel, e_abs, t_abs = worst
    print(f"[edges] {what}: worst row (b={r // H}, h={r % H}) rel-L2 {e_rel:.2e} (torch fp32 {t_rel:.2e}, "
          f"x{e_rel / max(t_rel, 1e-300):.2f}); max-abs {e_abs:.2e} (torch fp32 {t_abs:.2e}, x{e_abs / max(t_abs, 1e-300):.2f})")
    assert not bad, f"{what}: {bad}"


def _slots(dev, B, value=0.0):
    return torch.full((B,), value, dtype=torch.float32, device=dev).view(torch.int32)


def _in_amax(ops, x, E):
    """The per-sample exponent sources as ops.attention reduces them: max |q, k| and max |v|."""
    return torch.cat([ops.absmax_rows(x[:, :2 * E]), ops.absmax_rows(x[:, 2 * E:])])


def _heads_form(N, x, E, H, image, in_amax, out_amax):
    """ds_attention_h3_heads on a NaN-filled output; image: with the K / V image workspace."""
    B, _, L = x.shape
    out = torch.full((B, E, L), float("nan"), device=x.device)
    work = None
    if image:
        nbytes = N.lib().ds_attention_h3_heads_workspace_bytes(B, E, H, L)
        assert nbytes == B * L * E * 8
        work = torch.empty(nbytes // 4, device=x.device)
    N.check(N.lib().ds_attention_h3_heads(out.data_ptr(), x.data_ptr(), None if work is None else work.data_ptr(), B, E, H, L,
                                          None if in_amax is None else in_amax.data_ptr(),
                                          None if out_amax is None else out_amax.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "ds_attention_h3_heads")
    return out


def run_forms(what, ops, N, qkv, E, H, dev, through_ops=True):
    """Both forms of the MFMA head kernel on qkv (CPU), every query stored, the two forms bit-equal, out_amax merged and equal to
    the per-sample max |out|, ops.attention (in_amax passed / reduced inside) the same bits; then the bound per row."""
    B, _, L = qkv.shape
    assert L % 32 == 0 and E // H in (32, 64, 128, 256)
    x = qkv.to(dev)
    in_amax = _in_amax(ops, x, E)
    outs = {}
    for image in (False, True):
        form = "image" if image else "staged"
        slots = _slots(dev, B)
        out = _heads_form(N, x, E, H, image, in_amax, slots)
        assert torch.isfinite(out).all(), f"{what} {form}: a query was not stored"
        assert torch.equal(slots.view(torch.float32), out.abs().flatten(1).amax(dim=1)), f"{what} {form}: out_amax"
        kept = _slots(dev, B, BIG)                   # the maximum is merged into the slot, not written over it
        again = _heads_form(N, x, E, H, image, in_amax, kept)
        assert torch.equal(kept, _slots(dev, B, BIG)), f"{what} {form}: a slot above the maximum was overwritten"
        assert torch.equal(again, out)
        outs[form] = out
    assert torch.equal(outs["staged"], outs["image"]), f"{what}: staged and image forms differ"
    if through_ops:
        for passed in (in_amax, None):
            slots = _slots(dev, B)
            o = ops.attention(x, E, out=torch.full((B, E, L), float("nan"), device=dev), precision="fp16x3", heads=H,
                              in_amax=passed, out_amax=slots)
            assert torch.equal(o, outs["staged"]), f"{what}: ops.attention differs (in_amax {'passed' if passed is not None else 'inside'})"
            assert torch.equal(slots.view(torch.float32), o.abs().flatten(1).amax(dim=1))
    check_rows(what, outs["staged"], qkv, E, H)
    return outs["staged"]


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- 1. head width 256 under a head axis: k_attn3h<8, *, MH = true>
@pytest.mark.parametrize("E,H,L", [(512, 2, 32), (512, 2, 160), (1024, 4, 32)])
def test_head_width_256_with_head_axis(ops, N, dev, E, H, L):
    """Route: ds_attention_h3_heads, d = 256, staged (512 VGPRs, 128 KiB LDS) and image form; L = 32 is one key tile with three
    inactive waves, L = 160 a second query block with one active wave.  ops picks the staged form at these lengths."""
    for B in (1, 2):
        assert ops.attention_workspace_floats(B, E, L, "fp16x3", heads=H) == 0
        run_forms(f"d=256 E={E} H={H} L={L} B={B}", ops, N, _randn(E + H + L + B, B, 3 * E, L), E, H, dev)


def test_head_width_256_through_ops_uses_images(ops, N, dev):
    """Route: ops.attention(heads=2) at E = 512, L = 1024: the predicate says images (d = 256 from L = 1024)."""
    E, H, L, B = 512, 2, 1024, 1
    assert ops.attention_workspace_floats(B, E, L, "fp16x3", heads=H) == N.lib().ds_attention_h3_heads_workspace_bytes(B, E, H, L) // 4 > 0
    qkv = _randn(77, B, 3 * E, L)
    got = ops.attention(qkv.to(dev), E, out=torch.full((B, E, L), float("nan"), device=dev), precision="fp16x3", heads=H)
    check_rows(f"d=256 through ops E={E} H={H} L={L}", got, qkv, E, H)


# ---------------------------------------------------------------- 2. the head axis at L % 128 != 0
@pytest.mark.parametrize("L", [32, 64, 96, 160])
@pytest.mark.parametrize("E,H", [(64, 2), (96, 3), (128, 2), (256, 2)])
def test_head_axis_with_inactive_waves(ops, N, dev, E, H, L):
    """Route: ds_attention_h3_heads at d = 32 / 64 / 128, staged and image; 128 - L % 128 queries' worth of waves recompute block
    L - 32 and must store nothing, and every wave commits to out_amax."""
    for B in (1, 3):
        assert ops.attention_workspace_floats(B, E, L, "fp16x3", heads=H) == 0
        run_forms(f"ragged block E={E} H={H} L={L} B={B}", ops, N, _randn(3 * E + H + L + B, B, 3 * E, L), E, H, dev)


# ---------------------------------------------------------------- 3. the generic head kernel
GENERIC = [(48, 4, 35, 2), (96, 4, 100, 1), (130, 2, 65, 1), (128, 16, 33, 3), (64, 2, 63, 1), (64, 2, 1, 2), (30, 3, 7, 1),
           (64, 2, 64, 1)]


@pytest.mark.parametrize("E,H,L,B", GENERIC)
def test_generic_head_kernel(ops, dev, E, H, L, B):
    """Route: k_attn_heads_generic for precision "fp32" always, and for "fp16x3" unless d is an MFMA width and L % 32 == 0 (only
    (64, 2, 64, 1) here).  Fewer keys than lanes, one key, a second trip of the query fill (d = 65), d % 4 != 0, odd B * heads."""
    qkv = _randn(E + 5 * H + L + B, B, 3 * E, L)
    x = qkv.to(dev)
    generic16 = not (L % 32 == 0 and E // H in (32, 64, 128, 256))
    assert generic16 == ((E, H, L, B) != (64, 2, 64, 1))
    outs = {}
    for precision in ("fp32", "fp16x3"):
        assert ops.attention_workspace_floats(B, E, L, precision, heads=H) == 0
        slots = _slots(dev, B)
        out = ops.attention(x, E, out=torch.full((B, E, L), float("nan"), device=dev), precision=precision, heads=H, out_amax=slots)
        assert torch.equal(slots.view(torch.float32), out.abs().flatten(1).amax(dim=1)), f"{precision}: out_amax"
        check_rows(f"generic E={E} H={H} L={L} B={B} {precision}", out, qkv, E, H)
        outs[precision] = out
    if generic16:
        assert torch.equal(outs["fp32"], outs["fp16x3"])


# ---------------------------------------------------------------- 4. dynamic LDS of the generic kernels between 48 and 64 KiB
def _subset(L):
    """The first and last 70 queries and every 97th between."""
    return torch.tensor(sorted(set(range(70)) | set(range(70, L - 70, 97)) | set(range(L - 70, L))))


@pytest.mark.parametrize("E,H,L", [(64, 2, 12290), (64, 2, 16384 - 32), (48, 1, 12290 - 48), (48, 1, 16384 - 48)])
def test_generic_kernels_lds_window(ops, dev, E, H, L):
    """Routes: k_attn_heads_generic (H = 2, d = 32) and k_attn_generic (H = 1, E = 48) with (d + L) * 4 bytes of dynamic LDS just
    above 48 KiB and at the 64 KiB cap.  fp64 on about 270 of the queries, against all keys."""
    d = E // H
    assert 12288 < d + L <= 16384
    qkv = _randn(E + L, 1, 3 * E, L)
    out = ops.attention(qkv.to(dev), E, out=torch.full((1, E, L), float("nan"), device=dev), precision="fp32", heads=H)
    assert torch.isfinite(out).all()
    check_rows(f"LDS window E={E} H={H} L={L} ({(d + L) * 4} bytes)", out, qkv, E, H, qidx=_subset(L))


@pytest.mark.parametrize("E,H,L", [(64, 2, 16384 - 32 + 1), (48, 1, 16384 - 48 + 1)])
def test_generic_kernels_refuse_past_the_cap(ops, dev, E, H, L):
    """One past the cap: an error from the entry point, nothing launched."""
    x = torch.zeros(1, 3 * E, L, device=dev)
    out = torch.full((1, E, L), float("nan"), device=dev)
    with pytest.raises(RuntimeError, match="too large for the generic path"):
        ops.attention(x, E, out=out, precision="fp32", heads=H)
    assert torch.isnan(out).all()


# ---------------------------------------------------------------- 5. heads of different magnitude inside one sample
@pytest.mark.parametrize("case", ["v", "qk"])
def test_per_head_magnitudes_inside_a_sample(ops, N, dev, case):
    """Route: ds_attention_h3_heads, d = 64, both forms.  One exponent pair per sample serves its four heads: the staging scale
    puts the sample's maximum in [2^13, 2^14) and the lo piece of the split stays a normal fp16 number down to 2^-16 of it, so a
    head 2^-12 below the loudest keeps its 22 bits ("v"); a head whose q and k are 2^-6 of the others' has a near-uniform
    softmax ("qk").  The bound is per row, where whole-tensor rel-L2 would only see the loud heads."""
    E, H, L, B = 256, 4, 128, 2
    d = E // H
    qkv = _randn(5 if case == "v" else 6, B, 3 * E, L)
    if case == "v":
        for h, s in enumerate((1.0, 2.0 ** -12, 2.0 ** -6, 1.0)):
            qkv[:, 2 * E + h * d:2 * E + (h + 1) * d] *= s
    else:
        qkv[:, d:2 * d] *= 2.0 ** -6
        qkv[:, E + d:E + 2 * d] *= 2.0 ** -6
    run_forms(f"per-head magnitudes ({case})", ops, N, qkv, E, H, dev)


# ---------------------------------------------------------------- 6. staircase logits: the deferred rescale
def _staircase(E, H, L, B, c, seed):
    """k_j = 0.1 noise + c floor(j / 32) u, q_i = 0.1 noise + sqrt(d) a_i u, a cycling through (1, -1, 0.5, -0.25), u a unit
    direction per head: query i's logits are a_i c floor(j / 32) -- rising by c per key tile for a > 0 (by 8 = RESCALE_T or more
    only on some tiles at c = 5, on every tile at c = 9), falling for a < 0, with both signs in every wave."""
    d = E // H
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(H, d, generator=g, dtype=torch.float64)
    u = (u / u.norm(dim=1, keepdim=True)).float()
    a = torch.tensor([1.0, -1.0, 0.5, -0.25]).repeat((L + 3) // 4)[:L]
    step = torch.div(torch.arange(L), 32, rounding_mode="floor").float()
    qkv = torch.randn(B, 3, H, d, L, generator=g)
    qkv[:, :2] *= 0.1
    qkv[:, 0] += (d ** 0.5) * u[None, :, :, None] * a
    qkv[:, 1] += c * u[None, :, :, None] * step
    return qkv.reshape(B, 3 * E, L)


@pytest.mark.parametrize("c,L", [(5, 96), (5, 160), (9, 96)])
@pytest.mark.parametrize("d", [32, 128])
def test_staircase_logits_mfma(ops, N, dev, d, c, L):
    """Route: ds_attention_h3_heads, both forms.  Lanes that move their maximum sit next to lanes that keep it, and P reaches e^5
    unrescaled in the fp16 split."""
    E, H, B = 2 * d, 2, 2
    run_forms(f"staircase d={d} c={c} L={L}", ops, N, _staircase(E, H, L, B, c, 100 * d + 10 * c + L), E, H, dev)


@pytest.mark.parametrize("c", [5, 9])
@pytest.mark.parametrize("d", [32, 128])
def test_staircase_logits_generic(ops, dev, d, c):
    """Route: k_attn_heads_generic (L = 95 is no multiple of 32), both precisions, identical bits."""
    E, H, L, B = 2 * d, 2, 95, 2
    qkv = _staircase(E, H, L, B, c, 100 * d + 10 * c + L)
    outs = [ops.attention(qkv.to(dev), E, out=torch.full((B, E, L), float("nan"), device=dev), precision=p, heads=H)
            for p in ("fp32", "fp16x3")]
    assert torch.equal(outs[0], outs[1])
    check_rows(f"staircase generic d={d} c={c} L={L}", outs[0], qkv, E, H)


# ---------------------------------------------------------------- 7. the shapes of test_gpu_attention_heads.py with the max-abs bound
@pytest.mark.parametrize("precision", ["fp16x3", "fp32"])
@pytest.mark.parametrize("E,H", [(128, 4), (256, 8), (128, 16)])
def test_existing_shapes_with_max_abs(ops, dev, E, H, precision):
    """Route: ops.attention at L = 256, B = 3: the staged MFMA head kernel (fp16x3, d = 32) or k_attn_heads_generic (fp32; d = 8)."""
    L, B = 256, 3
    assert ops.attention_workspace_floats(B, E, L, precision, heads=H) == 0
    qkv = _randn(E * 7 + H * 3 + L + B, B, 3 * E, L)
    got = ops.attention(qkv.to(dev), E, out=torch.full((B, E, L), float("nan"), device=dev), precision=precision, heads=H)
    check_rows(f"max-abs E={E} H={H} L={L} B={B} {precision}", got, qkv, E, H)
