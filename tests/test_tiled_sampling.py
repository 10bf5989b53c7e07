"""Host side of the tiled volume sampling: the integers of extra.grid_plan against what the reference's own helpers return
(tests/golden/tiled_plan.npz, recorded by tools/make_tiled_sampling_golden.py), the rows of the fused inpainting run, and
every refusal of the new entry points before any launch.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def plans():
    z = np.load(os.path.join(GOLD, "tiled_plan.npz"))
    return z, json.loads(str(z["info"]))


def test_fixture_holds_the_cases_the_issue_names(plans):
    _, info = plans
    cases = [(tuple(g), tuple(p)) for g, p in info["cases"]]
    for want in (((2, 2, 2), (False,) * 3), ((2, 2, 2), (True, True, False)), ((2, 2, 2), (True,) * 3), ((3, 2, 1), (False,) * 3),
                 ((3, 2, 2), (False,) * 3)):
        assert want in cases
    assert info["base_shape"] == [2, 8, 8, 8] and info["overlap_size"] == 4


@pytest.mark.parametrize("case", range(6))
def test_grid_plan_equals_the_references_helpers(plans, case):
    from diffsci_amd import extra
    z, info = plans
    grid, per = info["cases"][case]
    base, overlap = info["base_shape"], info["overlap_size"]
    final = [b * g for b, g in zip(base[1:], grid)]
    cubes = extra.grid_plan(grid, base, overlap, per)
    order, bounds = z[f"p{case}/order"], z[f"p{case}/bounds"]
    assert [c.position for c in cubes] == [tuple(int(v) for v in p) for p in order]
    assert sum(c.is_corner for c in cubes) == int(z[f"p{case}/corners"])
    assert all(c.is_corner == (i < int(z[f"p{case}/corners"])) for i, c in enumerate(cubes))
    for j, c in enumerate(cubes):
        mask = z[f"p{case}/mask{j}"]
        assert c.start == tuple(int(v) for v in bounds[j, :3])
        assert c.length == tuple(mask.shape)                           # what periodic_getitem returned for the slices
        for a in range(3):                                              # the stop, as the reference states it
            stop = c.start[a] + c.length[a]
            assert int(bounds[j, 3 + a]) == (stop % final[a] if per[a] else stop)
        got = np.zeros(c.length, dtype=np.uint8)
        for (s0, s1, s2), (n0, n1, n2) in c.mask_boxes:
            assert min(s0, s1, s2) >= 0 and s0 + n0 <= c.length[0] and s1 + n1 <= c.length[1] and s2 + n2 <= c.length[2]
            got[s0:s0 + n0, s1:s1 + n1, s2:s2 + n2] = 1
        assert np.array_equal(got, mask), (case, j)
        if c.is_corner:                                                 # a corner never meets an earlier cube
            assert not c.mask_boxes


def test_generation_order_is_the_eight_parities():
    from diffsci_amd.extra import fillinginpainting as F
    order, corners = F.generation_order([3, 2, 2])
    assert corners == 2 and order[:2] == [(0, 0, 0), (2, 0, 0)]
    assert len(order) == 12 and len(set(order)) == 12
    parity = [tuple(v % 2 for v in p) for p in order]
    assert parity == sorted(parity)                                     # (e,e,e) < (e,e,o) < ... < (o,o,o)


class _Module:
    device = torch.device("cpu")


def test_generators_refuse_before_any_launch(monkeypatch):
    from diffsci_amd import _native, extra
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    m = _Module()
    with pytest.raises(ValueError, match="Grid map for dimension 0 is not even, but periodicity is True"):
        extra.sample_grid_volume(m, [3, 2, 2], [2, 8, 8, 8], 4, periodicity=[True, False, False])
    with pytest.raises(ValueError, match="Grid map for dimension 2 is not even"):
        extra.grid_plan([2, 2, 1], [2, 8, 8, 8], 4, [False, False, True])
    with pytest.raises(ValueError, match="Unknown blend_mode: cosine"):
        extra.sample_grid_volume(m, [2, 2, 2], [2, 8, 8, 8], 4, blend_mode="cosine")
    with pytest.raises(ValueError, match="num_blocks must be at least 1"):
        extra.sample_sequential_z(m, 0, [2, 8, 8, 8], 4)
    with pytest.raises(ValueError, match="overlap_size must be non-negative"):
        extra.sample_sequential_z(m, 2, [2, 8, 8, 8], -2)
    with pytest.raises(ValueError, match="overlap_size must be even"):
        extra.sample_sequential_z(m, 2, [2, 8, 8, 8], 3)
    with pytest.raises(ValueError, match="overlap_size must be less than base block z-dimension"):
        extra.sample_sequential_z(m, 2, [2, 8, 8, 8], 8)
    with pytest.raises(ValueError, match="Expected 2 conditions, got 3"):
        extra.sample_sequential_z(m, 2, [2, 8, 8, 8], 4, y=[None, None, None])
    # a module on the host reaches the first op, which says there is no CPU path -- still before any launch
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        extra.sample_grid_volume(m, [2, 2, 2], [2, 4, 4, 4], 2, noise=iter([torch.zeros(1, 2, 8, 8, 8)]))
    assert calls == []


def test_block_extents():
    from diffsci_amd.extra import sequentialinpainting as S
    assert S.block_extents(1, 8, 4) == [8] and S.block_extents(2, 8, 4) == [10, 10] and S.block_extents(4, 8, 4) == [10, 12, 12, 10]
    w = S.cosine_blend_weights(4)
    assert w[0] == 0 and abs(float(w[-1]) - 1) < 1e-6 and torch.allclose(w + w.flip(0), torch.ones(4), atol=1e-6)


def test_box_scatter_refuses_before_any_launch(monkeypatch):
    from diffsci_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    src, dst = torch.zeros(2, 4, 5, 6), torch.zeros(2, 8, 8, 8)
    with pytest.raises(ValueError, match="longer than a destination axis"):
        ops.box_scatter3d(torch.zeros(2, 9, 2, 2), (0, 0, 0), dst, (0, 0, 0), (9, 2, 2))
    with pytest.raises(ValueError, match="leaves src"):
        ops.box_scatter3d(src, (1, 0, 0), dst, (0, 0, 0), (4, 5, 6))
    with pytest.raises(ValueError, match="leaves src"):
        ops.box_scatter3d(src, (0, 0, -1), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="leaves src"):
        ops.box_scatter3d(src, (0, 0, 0), dst, (0, 0, 0), (1, -1, 1))
    with pytest.raises(ValueError, match="different numbers of planes"):
        ops.box_scatter3d(src, (0, 0, 0), torch.zeros(3, 8, 8, 8), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="fp32 only"):
        ops.box_scatter3d(src.double(), (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="at least three axes"):
        ops.box_scatter3d(torch.zeros(4, 4), (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="three integers"):
        ops.box_scatter3d(src, (0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="share storage"):
        ops.box_scatter3d(dst[:, :4], (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(TypeError):
        ops.box_scatter3d(None, (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.box_scatter3d(src, (0, 0, 0), dst, (-3, 7, 5), (4, 5, 6))
    assert calls == []


def _step_args():
    from diffsci_amd._native import EvalCoef, SIStep, DS_IN_FLOW
    k = EvalCoef(c_out=1.0, sigma_sq=1.0, neg_mult=1.0, guidance=1.0, input_kind=DS_IN_FLOW, next_scale=1.0, xin_copies=1)
    s = SIStep(1.0, 1.0, -1.0, -0.5, -0.25, 0.5, 0.75, 0.25, 0.5, 0.5, 1.0)
    return k, s


def test_inpaint_step_refuses_before_any_launch(monkeypatch):
    from diffsci_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    k, s = _step_args()
    x, f = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4)
    xo, m = torch.zeros(3, 4), torch.zeros(3, 4)
    ea, eb = torch.zeros(2, 3, 4), torch.zeros(1, 3, 4)
    out = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="renoise goes with blend"):
        ops.si_inpaint_step(x, f, k, s, renoise=True, eps=(ea,), x_out=out)
    with pytest.raises(ValueError, match="exactly one"):
        ops.si_inpaint_step(x, f, k, s, x_out=out)
    with pytest.raises(ValueError, match="exactly one"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,), philox=(torch.zeros(2, dtype=torch.int64), 0), x_out=out)
    with pytest.raises(ValueError, match="no output requested"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,))
    with pytest.raises(ValueError, match="size mismatch"):
        ops.si_inpaint_step(x, torch.zeros(2, 3, 5), k, s, eps=(ea,), x_out=out)
    with pytest.raises(ValueError, match="size mismatch"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,), x_out=torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match="xin_out holds"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,), xin_out=torch.zeros(2, 2, 3, 4))
    with pytest.raises(ValueError, match="one sample"):
        ops.si_inpaint_step(x, f, k, s, blend=True, x_orig=xo, mask=torch.zeros(2, 3, 4), eps=(ea, eb), x_out=out)
    with pytest.raises(ValueError, match="one sample"):
        ops.si_inpaint_step(x, f, k, s, blend=True, mask=m, eps=(ea, eb), x_out=out)
    with pytest.raises(ValueError, match="reads 2 injected draws"):
        ops.si_inpaint_step(x, f, k, s, blend=True, x_orig=xo, mask=m, eps=(ea,), x_out=out)
    with pytest.raises(ValueError, match="reads 4 injected draws"):
        ops.si_inpaint_step(x, f, k, s, blend=True, renoise=True, x_orig=xo, mask=m, eps=(ea, eb, ea), x_out=out)
    with pytest.raises(ValueError, match="draw 1 holds"):
        ops.si_inpaint_step(x, f, k, s, blend=True, x_orig=xo, mask=m, eps=(ea, ea), x_out=out)
    with pytest.raises(ValueError, match="empty state"):
        ops.si_inpaint_step(torch.zeros(0, 4), torch.zeros(0, 4), k, s, eps=(torch.zeros(0, 4),), x_out=torch.zeros(0, 4))
    with pytest.raises(ValueError, match="overlaps x"):
        big = torch.zeros(40)
        ops.si_inpaint_step(big[:24].view(2, 3, 4), f, k, s, eps=(ea,), x_out=big[4:28].view(2, 3, 4))
    with pytest.raises(ValueError, match="an output overlaps an input"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,), x_out=f)
    with pytest.raises(ValueError, match="an output overlaps an input"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,), x_out=out, xin_out=x)
    with pytest.raises(TypeError, match="philox state"):
        ops.si_inpaint_step(x, f, k, s, philox=(torch.zeros(2), 0), x_out=out)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.si_inpaint_step(x, f, k, s, eps=(ea,), x_out=x)               # in place is allowed; the host tensor is not
    assert calls == []


def test_c_entry_points_refuse_without_launching():
    """The C side's own refusals (no GPU needed: every one returns before the launch)."""
    import build
    from diffsci_amd import _native
    build.build(force=False, verbose=False)
    L = _native.lib()
    k, s = _step_args()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    scatter = lambda dst, src, *a: L.ds_box_scatter3d(dst, src, 1, *a)                       # noqa: E731
    assert scatter(None, p, 4, 4, 4, 0, 0, 0, 2, 2, 2, 0, 0, 0, 2, 2, 2, None, 0) == -2
    assert scatter(p, p + 128, 4, 4, 4, 0, 0, 0, 2, 2, 2, 0, 0, 0, 2, 2, 2, None, 1) == -1    # an undefined flag
    assert b"flags" in L.ds_last_error()
    assert scatter(p, p + 128, 2, 2, 2, 0, 0, 0, 4, 4, 4, 0, 0, 0, 3, 1, 1, None, 0) == -1    # longer than the destination axis
    assert b"more than one period" in L.ds_last_error()
    assert scatter(p, p + 128, 4, 4, 4, 0, 0, 0, 2, 2, 2, 1, 0, 0, 2, 1, 1, None, 0) == -1    # the source box leaves src
    assert scatter(p, p + 128, 4, 4, 4, -9, 0, 0, 2, 2, 2, 0, 0, 0, 0, 2, 2, None, 0) == 0     # an empty box launches nothing
    step = lambda **kw: L.ds_si_inpaint_step(*[kw.get(n, d) for n, d in (                     # noqa: E731
        ("x_out", p), ("xin_out", None), ("x", p), ("f", p + 64), ("fu", None), ("k", ctypes.byref(k)), ("s", ctypes.byref(s)),
        ("x_orig", None), ("mask", None), ("ea", p + 128), ("eb", None), ("ec", None), ("ed", None), ("rng", None), ("off", 0),
        ("B", 2), ("n", 4), ("stream", None), ("flags", 0))])
    assert step(x=None) == -2 and step(x_out=None) == -2 and step(k=None) == -2 and step(s=None) == -2
    assert step(flags=2) == -1 and step(flags=4) == -1                                        # renoise without blend; undefined
    assert step(flags=1) == -2                                                                # a blend without x_orig / mask
    assert step(flags=1, x_orig=p + 160, mask=p + 176) == -2                                  # ... without its draw
    assert step(flags=3, x_orig=p + 160, mask=p + 176, eb=p + 192) == -2                      # a jump without its draws
    assert step(ea=None) == -2 and step(rng=p + 8) == -2                                      # no noise source; two
    assert step(ea=None, rng=p + 4) == -1                                                     # a misaligned state
    assert step(B=-1) == -1 and step(n=0) == -1
    s0 = _native.SIStep(1.0, 1.0, 0.0, -0.5, -0.25, 0.5, 0.75, 0.25, 0.5, 0.5, 1.0)
    assert step(s=ctypes.byref(s0)) == -1 and b"denominator" in L.ds_last_error()
    k.input_kind = _native.DS_IN_SCORE
    assert step() == -1
    k.input_kind, k.xin_copies = _native.DS_IN_FLOW, 3
    assert step() == -1
    k.xin_copies = 1
    assert step(B=0) == 0                                                                     # nothing to do, nothing launched
    assert L.ds_si_inpaint_counters(2, 6, 0) == 3 and L.ds_si_inpaint_counters(2, 6, 1) == 5
    assert L.ds_si_inpaint_counters(2, 6, 3) == 10 and L.ds_si_inpaint_counters(0, 6, 3) == 0
    from diffsci_amd import ops
    assert [ops.si_inpaint_counters(2, 6, b, r) for b, r in ((False, False), (True, False), (True, True))] == [3, 5, 10]


def test_inpaint_rows_follow_the_eager_loop():
    """The row list resolves mask_start_t and jump_length exactly as SIModule.inpaint's nested loops do, and asks for as many
    draws as the reference made on the si8_inpaint fixture."""
    import diffsci_amd.models as M
    from diffsci_amd.models.karras import siloop
    v = np.load(os.path.join(GOLD, "si8_inpaint.npz"))
    for tag, cfgkw, kw in (("hard", dict(scheduler="linear"), dict(nsteps=5)),
                           ("soft_jump", dict(scheduler="cosine", precondition_fn="edm", initial_norm=2.0),
                            dict(nsteps=5, resample_steps=1, mask_start_t=0.8))):
        cfg = M.SIModuleConfig(**cfgkw)
        table = siloop.inpaint_table(cfg, **kw)
        assert sum(r.draws for r in table.rows) == int(v[tag + "_ndraws"])
    cfg = M.SIModuleConfig(scheduler="linear")
    nsteps, resample, jump_length, start = 6, 2, 2, 0.5
    table = siloop.inpaint_table(cfg, nsteps, False, resample, jump_length, start)
    ts = torch.linspace(1, 0, nsteps)
    want = []
    for i in range(nsteps - 1):
        for r in range(resample + 1):
            blend = ts[i + 1].item() <= start
            want.append((float(ts[i]), blend, blend and r < resample and i + jump_length < nsteps - 1))
    assert [(float(r.first.t), r.blend, r.jump) for r in table.rows] == want
    assert any(j for _, _, j in want) and not all(b for _, b, _ in want)
    r = table.rows[4]
    t, tn = ts[1], ts[2]
    assert r.dt == float(tn - t) and r.score_a == float(1 - t) and r.score_b == 1.0 and r.jump_sigma == float(t)
    assert r.patch_alpha == float(1 - tn) and r.patch_sigma == float(tn) and r.neg_half_omega == -float(0.5 * t)
    assert r.score_den == float(t * (-1.0 * t - (1 - t) * 1.0)) and r.noise_coef == float(torch.sqrt(t * abs(r.dt)))
    assert table.digest() != siloop.inpaint_table(cfg, nsteps, False, resample, 1, start).digest()
    em = siloop.em_table(cfg, ts)
    assert len(em.rows) == nsteps - 1 and not any(r.blend or r.jump for r in em.rows) and sum(r.draws for r in em.rows) == nsteps - 1


def test_fused_methods_keep_the_pinned_signatures():
    import inspect
    import diffsci_amd.models as M
    a, b = inspect.signature(M.SIModule.inpaint), inspect.signature(M.SIModule.inpaint_fused.__wrapped__)
    assert list(a.parameters) == list(b.parameters)
    assert [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()]
    a, b = inspect.signature(M.SIModule.sample), inspect.signature(M.SIModule.sample_fused.__wrapped__)
    assert list(a.parameters) + ["noise"] == list(b.parameters)
