"""The tiled volume sampling on the GPU: the fused Euler-Maruyama inpainting step (ds_inpaint.hip) against the eager op chain
it replaces and an fp64 restatement, its Philox stream, the fused captured run on the si8_inpaint fixture, the periodic
scatter (ds_window.hip), and the two generators against volumes the reference produced on the CPU with recorded draws
(tools/make_tiled_sampling_golden.py)."""
import itertools
import json
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden_util import load, rel_l2  # noqa: E402

REL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


def referee(got, want32, want64, what=""):
    """The rule of tests/test_gpu_vaenet.py."""
    e32, e64, ref = rel_l2(got, want32), rel_l2(got, want64), rel_l2(want32, want64)
    print(f"{what}: vs the chain {e32:.2e}; vs fp64 {e64:.2e}; the chain vs fp64 {ref:.2e}")
    assert e32 < REL, (what, e32)
    assert e64 < max(4 * ref, 2e-6), (what, e64, ref)


# ---------------------------------------------------------------- the kernel against the eager chain
SHAPES = [(1, 2, 6, 6, 6), (2, 3, 5, 5, 5), (3, 1, 1, 1, 3), (2, 1, 32, 32)]
MODES = ("no_mask", "skipped", "blend", "renoise")       # no known region at all; a masked run before mask_start_t; ...


def chain(ops, x, f, fu, k, r, c_in_next, x_orig, mask, eps, mode):
    """SIModule._em_step and inpaint's blend, op by op (flowfield.py of this package: the code the fused kernel replaces)."""
    B = x.shape[0]
    v = ops.drift(x, f, k, fu=fu)
    num = ops.axpby(v, r.score_a, x, r.score_b)
    score = ops.div_scalar(num, r.score_den, out=num)
    d = ops.axpby(v, 1.0, score, r.neg_half_omega)
    out = ops.axpby(x, 1.0, d, r.dt)
    out = ops.axpby(out, 1.0, eps[0], r.noise_coef)
    if mode in ("blend", "renoise"):
        patch = ops.axpby(x_orig, r.patch_alpha, eps[1], r.patch_sigma)
        out = ops.mask_blend(out, patch.expand(B, *x.shape[1:]).contiguous(), mask)
    if mode == "renoise":
        out = ops.axpby(out, r.jump_alpha, eps[2], r.jump_sigma)
        patch = ops.axpby(x_orig, r.jump_alpha, eps[3], r.jump_sigma)
        out = ops.mask_blend(out, patch.expand(B, *x.shape[1:]).contiguous(), mask)
    return out, ops.scale(out, c_in_next)


def chain64(x, f, fu, k, r, c_in_next, x_orig, mask, eps, mode, network):
    x, f, x_orig, mask = x.double(), f.double(), x_orig.double(), mask.double()
    eps = [e.double() for e in eps]
    F = f if fu is None else k.one_minus_guidance * fu.double() + k.guidance * f
    if network:
        v = k.neg_mult * ((k.c_out * F + k.c_skip * x - x) / k.sigma_sq)
    else:
        v = k.neg_mult * (F / k.sigma_sq)
    score = (r.score_a * v + r.score_b * x) / r.score_den
    out = x + r.dt * (v + r.neg_half_omega * score) + r.noise_coef * eps[0]
    if mode in ("blend", "renoise"):
        out = out * (1 - mask) + (r.patch_alpha * x_orig + r.patch_sigma * eps[1]) * mask
    if mode == "renoise":
        out = r.jump_alpha * out + r.jump_sigma * eps[2]
        out = out * (1 - mask) + (r.jump_alpha * x_orig + r.jump_sigma * eps[3]) * mask
    return out, c_in_next * out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_step_equals_the_eager_chain(M, dev, shape):
    from diffsci_amd import ops
    from diffsci_amd._native import DS_IN_FLOW, DS_IN_NETWORK
    from diffsci_amd.models.karras import siloop
    g = torch.Generator().manual_seed(sum(shape))
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                               # noqa: E731
    B, one = shape[0], (1,) + shape[1:]
    x, f, fu, x_orig = rnd(*shape), rnd(*shape), rnd(*shape), rnd(*one)
    eps = [rnd(*shape), rnd(*one), rnd(*shape), rnd(*one)]
    hard = (torch.rand(*shape[1:], generator=g) < 0.5).float().to(dev)
    soft = torch.rand(*shape[1:], generator=g).to(dev)
    tc, tn = torch.tensor(0.75), torch.tensor(0.5)
    configs = {"identity": M.SIModuleConfig(scheduler="linear"), "edm": M.SIModuleConfig(scheduler="cosine", precondition_fn="edm")}
    count = 0
    for (pre, cfg), ios, guidance, (mname, mask), mode in itertools.product(configs.items(), (False, True), (1.0, 2.5),
                                                                           (("hard", hard), ("soft", soft)), MODES):
        if mode in ("no_mask", "skipped") and mname == "soft":
            continue                                                                     # the mask is not read
        r = siloop.si_row(cfg, tc, tn, ios, blend=mode in ("blend", "renoise"), jump=mode == "renoise")
        nxt = cfg.preconditioner.eval_row(tc if mode == "renoise" else tn, ios)          # after a jump the next evaluation is at t_curr
        k = r.first.coef(DS_IN_FLOW if pre == "identity" else DS_IN_NETWORK, guidance)
        u = fu if guidance != 1.0 else None
        want, want_in = chain(ops, x, f, u, k, r, nxt.c_in, x_orig, mask, eps, mode)
        want64, want_in64 = chain64(x, f, u, k, r, nxt.c_in, x_orig, mask, eps, mode, pre == "edm")
        out, xin = torch.empty_like(x), torch.empty_like(x)
        masked = mode != "no_mask"                                                       # 'skipped': the buffers are there, the step does not blend
        ops.si_inpaint_step(x, f, k, r.step(nxt.c_in), fu=u, x_orig=x_orig if masked else None, mask=mask if masked else None,
                            blend=r.blend, renoise=r.jump, eps=eps, x_out=out, xin_out=xin)
        what = f"{shape} {pre} ios={ios} g={guidance} {mname} {mode}"
        referee(out.cpu(), want.cpu(), want64.cpu(), what)
        referee(xin.cpu(), want_in.cpu(), want_in64.cpu(), what + " xin")
        assert torch.equal(out, want) and torch.equal(xin, want_in), what               # the chain's own operation order
        count += 1
    assert count == 2 * 2 * 2 * (2 + 2 * 2)
    # in place, one output only, and two copies of the network input (the batched-guidance evaluation)
    r = siloop.si_row(configs["identity"], tc, tn, False, blend=True, jump=True)
    k = r.first.coef(DS_IN_FLOW, 2.5)
    want, want_in = chain(ops, x, f, fu, k, r, 0.7, x_orig, hard, eps, "renoise")
    state = x.clone()
    ops.si_inpaint_step(state, f, k, r.step(0.7), fu=fu, x_orig=x_orig, mask=hard, blend=True, renoise=True, eps=eps, x_out=state)
    assert torch.equal(state, want)
    only_in = torch.empty_like(x)
    ops.si_inpaint_step(x, f, k, r.step(0.7), fu=fu, x_orig=x_orig, mask=hard, blend=True, renoise=True, eps=eps, xin_out=only_in)
    assert torch.equal(only_in, want_in)
    k2 = r.first.coef(DS_IN_FLOW, 2.5, xin_copies=2)
    twice = torch.empty((2 * B,) + shape[1:], device=dev)
    ops.si_inpaint_step(x, f, k2, r.step(0.7), fu=fu, x_orig=x_orig, mask=hard, blend=True, renoise=True, eps=eps, x_out=state, xin_out=twice)
    assert torch.equal(twice[:B], want_in) and torch.equal(twice[B:], want_in)
    # the range guard's word: raised by a non-finite result, left alone by a finite one
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = r.first.coef(DS_IN_FLOW, 1.0, nonfinite=word)
    ops.si_inpaint_step(x, f, kw, r.step(0.7), x_orig=x_orig, mask=hard, blend=True, eps=eps, x_out=state)
    assert int(word) == 0
    bad = f.clone()
    bad.view(-1)[-1] = float("inf")
    ops.si_inpaint_step(x, bad, kw, r.step(0.7), eps=eps, x_out=state)
    assert int(word) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_philox_launch_equals_injected_launch_at_the_documented_offsets(M, dev, shape):
    from diffsci_amd import ops
    from diffsci_amd._native import DS_IN_FLOW
    from diffsci_amd.models.karras import siloop
    g = torch.Generator().manual_seed(7 + sum(shape))
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)                               # noqa: E731
    B, one = shape[0], (1,) + shape[1:]
    n = 1
    for s in shape[1:]:
        n *= s
    x, f, x_orig = rnd(*shape), rnd(*shape), rnd(*one)
    mask = torch.rand(*shape[1:], generator=g).to(dev)
    state = torch.tensor([0x1234_5678_9ABC, 40], dtype=torch.int64, device=dev)
    base = 1000
    cB, c1 = ops.philox_counters(B * n), ops.philox_counters(n)
    eps = [ops.philox_normal(state, base + o, s) for o, s in ((0, shape), (cB, one), (cB + c1, shape), (2 * cB + c1, one))]
    assert rel_l2(eps[0].cpu(), torch.zeros(())) > 0 and not torch.equal(eps[0], eps[2])
    cfg = M.SIModuleConfig(scheduler="linear")
    for blend, jump in ((False, False), (True, False), (True, True)):
        r = siloop.si_row(cfg, torch.tensor(0.6), torch.tensor(0.4), False, blend, jump)
        k = r.first.coef(DS_IN_FLOW, 1.0)
        a, a_in, b, b_in = (torch.empty_like(x) for _ in range(4))
        kw = dict(x_orig=x_orig, mask=mask, blend=blend, renoise=jump)
        ops.si_inpaint_step(x, f, k, r.step(0.9), eps=eps, x_out=a, xin_out=a_in, **kw)
        ops.si_inpaint_step(x, f, k, r.step(0.9), philox=(state, base), x_out=b, xin_out=b_in, **kw)
        assert torch.equal(a, b) and torch.equal(a_in, b_in), (shape, blend, jump)
        assert ops.si_inpaint_counters(B, n, blend, jump) == (2 * (cB + c1) if jump else cB + c1 if blend else cB)


# ---------------------------------------------------------------- the fused, captured run
class FixedField(torch.nn.Module):
    """A 'network' with a condition: a fixed linear map of its input and time, shifted by the condition."""

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(0.3))                # a parameter: the module's device follows it

    def forward(self, x, t, y=None):
        out = self.gain * x + t.reshape(-1, *([1] * (x.dim() - 1))) * 0.1
        return out if y is None else out + 0.05 * y["c"]


@pytest.mark.parametrize("pre", ["identity", "edm"])
def test_fused_run_equals_the_eager_inpaint_draw_for_draw(M, dev, pre):
    """inpaint_fused against inpaint (the parent's step-by-step path) on the same injected draws: every option the rows carry."""
    cfgkw = dict(scheduler="linear") if pre == "identity" else dict(scheduler="cosine", precondition_fn="edm", initial_norm=2.0)
    mod = M.SIModule(M.SIModuleConfig(**cfgkw), FixedField()).to(dev).eval()
    g = torch.Generator().manual_seed(11)
    shape = (3, 5, 5, 5)                                                 # n = 375
    x_orig, mask = torch.randn(*shape, generator=g), (torch.rand(*shape, generator=g) < 0.4).float()
    noise0 = torch.randn(2, *shape, generator=g)
    y = {"c": torch.randn(1, *shape, generator=g).to(dev)}
    from diffsci_amd.models.karras import siloop
    for ios, (cond, guidance), kw in itertools.product((False, True), ((None, 1.0), (y, 2.5)), (
            dict(nsteps=4), dict(nsteps=5, mask_falloff=1, resample_steps=1, mask_start_t=0.6),
            dict(nsteps=5, resample_steps=2, jump_length=2))):
        rows = siloop.inpaint_table(mod.config, kw["nsteps"], ios, kw.get("resample_steps", 0), kw.get("jump_length", 1),
                                    kw.get("mask_start_t", 1.0)).rows
        draws = [torch.randn(2 if i % 2 == 0 else 1, *shape, generator=g) for r in rows for i in range(r.draws)]
        assert len({r.draws for r in rows}) > (1 if len(kw) > 1 else 0)  # the longer cases mix the row kinds
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            args = dict(nsamples=2, y=cond, guidance=guidance, integrate_on_sigma=ios, orig_noise=noise0, **kw)
            a, b = iter(draws), iter(draws)
            want = mod.inpaint(x_orig, mask, noise=a, **args)
            got = mod.inpaint_fused(x_orig, mask, noise=b, **args)
        assert list(a) == [] and list(b) == []                           # both consumed every draw
        assert rel_l2(got.cpu(), want.cpu()) < REL, (pre, ios, guidance, kw)
    # the plain Euler-Maruyama run (sample with noise_injection): the eager chain with the same draws
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        steps = [torch.randn(2, *shape, generator=g) for _ in range(4)]
        got = mod.sample_fused(2, list(shape), nsteps=5, noise_injection=True, orig_noise=noise0, noise=iter(steps))
        it = iter(steps)
        x = noise0.to(dev) * float(mod.config.sigma_fn(torch.tensor(1.0)))
        ts = torch.linspace(1, 0, 5)
        for i in range(4):
            x = mod._em_step(x.contiguous(), ts[i], ts[i + 1], None, 1.0, False, lambda t: next(it).to(t).contiguous())
        assert rel_l2(got.cpu(), mod.initial_norm.unnorm(x).cpu()) < REL


def test_run_offsets_follow_the_documented_layout(M, dev):
    """A whole run on in-kernel Philox equals the same run injected with SILoop.row_noise -- ops.philox_normal at each row's
    offset (what the rows before it consumed) plus the launch's documented layout -- bit for bit."""
    from diffsci_amd import ops
    from diffsci_amd.models.karras import siloop
    mod = M.SIModule(M.SIModuleConfig(scheduler="linear"), FixedField()).to(dev).eval()
    g = torch.Generator().manual_seed(23)
    shape = (2, 3, 5, 5, 5)                                              # n = 375: counters per draw are rounded up
    x = torch.randn(*shape, generator=g).to(dev)
    x_orig, mask = torch.randn(*shape[1:], generator=g).to(dev), torch.rand(*shape[1:], generator=g).to(dev)
    table = siloop.inpaint_table(mod.config, 5, False, resample_steps=1, jump_length=1, mask_start_t=0.6)
    assert {r.draws for r in table.rows} == {1, 2, 4}
    with torch.inference_mode():
        a = siloop.SILoop(table, mod._source(None, 1.0, x), x)
        cB, c1 = ops.philox_counters(x.numel()), ops.philox_counters(x.numel() // 2)
        per = {1: cB, 2: cB + c1, 4: 2 * (cB + c1)}
        assert a.offsets == [sum(per[r.draws] for r in table.rows[:j]) for j in range(len(table.rows))]
        assert a.counters == sum(per[r.draws] for r in table.rows)
        a.load(x, 0.9)
        a.set_inputs(x_orig, mask)
        a.set_noise(None, seed_offset=(0x5EED, 4000))
        a.launch()
        draws = [e for j in range(len(table.rows)) for e in a.row_noise(j)]
        assert len(draws) == sum(r.draws for r in table.rows)
        b = siloop.SILoop(table, mod._source(None, 1.0, x), x, injected_noise=True)
        b.load(x, 0.9)
        b.set_inputs(x_orig, mask)
        b.set_noise(draws)
        b.launch()
        assert torch.equal(a.result(), b.result()) and torch.isfinite(a.result()).all()
        assert torch.equal(b.row_noise(1)[0], draws[table.rows[0].draws])


@pytest.fixture(scope="module")
def net8(M, dev):
    _, sd = load("punetg8_forward")
    net = M.PUNetG(M.PUNetGConfig(model_channels=8))
    net.load_state_dict(sd)
    return net.to(dev).eval()


def test_fused_run_on_the_si8_inpaint_fixture(M, net8, dev):
    """Both cases of test_si_inpaint, on the fused captured run, at the tolerance the eager path meets there."""
    v, _ = load("si8_inpaint")
    cases = (("hard", dict(scheduler="linear"), dict(nsteps=5)),
             ("soft_jump", dict(scheduler="cosine", precondition_fn="edm", initial_norm=2.0),
              dict(nsteps=5, mask_falloff=2, resample_steps=1, mask_start_t=0.8)))
    for tag, cfgkw, kw in cases:
        mod = M.SIModule(M.SIModuleConfig(**cfgkw), net8).to(dev).eval()
        draws = [v[f"{tag}_eps{i:02d}"] for i in range(int(v[tag + "_ndraws"]))]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):                                           # the capture, then its replay
                it = iter(draws)
                out = mod.inpaint_fused(v["x_orig"], v["mask"], nsamples=2, orig_noise=v["orig_noise"], noise=it, **kw).cpu()
                e = rel_l2(out, v[tag + "_out"])
                print(f"si8_inpaint {tag}: fused run vs the reference {e:.2e}")
                assert e < REL and list(it) == []
            assert len(mod._plans.plans) == 1
            with pytest.raises(StopIteration):
                mod.inpaint_fused(v["x_orig"], v["mask"], nsamples=2, orig_noise=v["orig_noise"], noise=draws[:2], **kw)
            torch.manual_seed(5)
            a = mod.inpaint_fused(v["x_orig"], v["mask"], nsamples=2, **kw)      # in-kernel noise: a second plan
            b = mod.inpaint_fused(v["x_orig"], v["mask"], nsamples=2, **kw)
            torch.manual_seed(5)
            c = mod.inpaint_fused(v["x_orig"], v["mask"], nsamples=2, **kw)
            assert a.shape == (2, 1, 32, 32) and torch.isfinite(a).all() and torch.equal(a, c) and not torch.equal(a, b)
            assert len(mod._plans.plans) == 2


# ---------------------------------------------------------------- the periodic scatter
def setitem_ref(dst, box, start):
    """periodic_setitem (torchutils.py:238-309) restated with index arithmetic: cell (i, j, k) of the box lands at
    (start + (i, j, k)) mod the axis."""
    idx = [(int(s) + torch.arange(n)) % d for s, n, d in zip(start, box.shape[-3:], dst.shape[-3:])]
    out = dst.clone()
    out[..., idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]] = box
    return out


SCATTERS = [  # dst spatial, src spatial, src start, dst start, box
    ((8, 9, 10), (4, 5, 6), (0, 0, 0), (6, 1, 2), (4, 5, 6)),            # a wrap on the first axis alone
    ((8, 9, 10), (4, 5, 6), (0, 0, 0), (1, 7, 2), (4, 5, 6)),            # the second
    ((8, 9, 10), (4, 5, 6), (0, 0, 0), (1, 1, 7), (4, 5, 6)),            # the third (inside a 4-vector)
    ((8, 9, 10), (4, 5, 6), (0, 0, 0), (6, 7, 7), (4, 5, 6)),            # all three
    ((8, 9, 12), (8, 9, 12), (0, 0, 0), (3, 4, 5), (8, 9, 12)),          # a box as long as every axis
    ((8, 9, 12), (3, 3, 3), (0, 0, 0), (7, 8, 11), (3, 3, 3)),           # a start at the last cell
    ((1, 1, 1), (2, 2, 2), (1, 1, 1), (0, 0, 0), (1, 1, 1)),             # size 1 everywhere
    ((8, 9, 10), (6, 7, 9), (2, 1, 3), (-3, -1, -13), (3, 5, 6)),        # a box inside src; negative destination starts
    ((16, 16, 16), (12, 12, 12), (0, 0, 0), (14, 14, 14), (12, 12, 12)),  # the generator's own: aligned rows, 16-byte quads
    ((8, 9, 10), (4, 5, 6), (0, 0, 0), (1, 1, 1), (4, 0, 6)),            # an empty box: nothing happens
]


@pytest.mark.parametrize("case", range(len(SCATTERS)))
def test_box_scatter_equals_periodic_setitem(dev, case):
    from diffsci_amd import ops
    D, S, s, d, L = SCATTERS[case]
    g = torch.Generator().manual_seed(case)
    src, dst = torch.randn(3, *S, generator=g), torch.randn(3, *D, generator=g)
    box = src[:, s[0]:s[0] + L[0], s[1]:s[1] + L[1], s[2]:s[2] + L[2]]
    want = setitem_ref(dst, box, d) if min(L) else dst
    got = dst.clone().to(dev)
    assert ops.box_scatter3d(src.to(dev), s, got, d, L) is got
    assert torch.equal(got.cpu(), want)
    if min(L):                                                           # gather after scatter returns the box
        back = ops.box_copy3d(got, d, torch.empty(3, *L, device=dev), (0, 0, 0), L)
        assert torch.equal(back.cpu(), box)
    with pytest.raises(ValueError, match="longer than a destination axis"):
        ops.box_scatter3d(torch.zeros(3, D[0] + 1, 1, 1, device=dev), (0, 0, 0), got, (0, 0, 0), (D[0] + 1, 1, 1))
    with pytest.raises(ValueError, match="leaves src"):
        ops.box_scatter3d(src.to(dev), (0, 0, 1), got, (0, 0, 0), (1, 1, S[2]))
    assert torch.equal(got.cpu(), want)                                  # the refusals wrote nothing


# ---------------------------------------------------------------- the generators, end to end
@pytest.fixture(scope="module")
def tiled_module(M, dev):
    plan, _ = load("tiled_plan")
    _, sd = load("tiled_net_w1")
    net = M.PUNetG(M.PUNetGConfig(**json.loads(plan["info"])["net"]))
    r = net.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return M.SIModule(M.SIModuleConfig(scheduler="linear"), net.to(dev).eval()).to(dev).eval()


def replay(name, fn, module):
    v, _ = load("tiled_" + name)
    draws = iter([v[f"eps{i:03d}"] for i in range(int(v["ndraws"]))])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = fn(module, **json.loads(v["args"]), noise=draws)
    assert list(draws) == []                                             # every draw the reference made was consumed
    e = rel_l2(out.cpu(), v["out"])
    print(f"tiled_{name}: vs the reference {e:.2e}")
    assert tuple(out.shape) == tuple(v["out"].shape) and e < REL, (name, e)


@pytest.mark.parametrize("name", ["grid222_none", "grid222_ttf", "grid222_all", "grid321_none"])
def test_grid_volume_equals_the_reference(tiled_module, name):
    from diffsci_amd import extra
    replay(name, extra.sample_grid_volume, tiled_module)


@pytest.mark.parametrize("name", [f"seq{n}_{mode}" for n in (1, 2, 3) for mode in ("cosine", "latest")])
def test_sequential_volume_equals_the_reference(tiled_module, name):
    from diffsci_amd import extra
    replay(name, extra.sample_sequential_z, tiled_module)


def test_grid_volume_capture(tiled_module):
    """All axes periodic: every cube has one shape, so the run leaves two plans (the sampled corner, the inpainted cubes); a
    replayed run equals the same kernels launched eagerly bit for bit; a seed reproduces, consecutive calls differ."""
    from diffsci_amd import extra
    mod = tiled_module
    kw = dict(grid_map=[2, 2, 2], base_shape=[2, 8, 8, 8], overlap_size=4, nsteps=4, periodicity=[True, True, True])
    runs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for use_graph, seed in ((True, 3), (True, None), (True, 3), (False, 3)):
            mod.use_graph = use_graph
            if use_graph and not runs:
                mod._plans.clear()
            if seed is not None:
                torch.manual_seed(seed)
            runs.append(extra.sample_grid_volume(mod, **kw))
            if use_graph:
                assert len(mod._plans.plans) == 2
        mod.use_graph = True
    first, second, again, eager = runs
    assert first.shape == (1, 2, 16, 16, 16) and torch.isfinite(first).all()
    assert torch.equal(first, again) and torch.equal(first, eager) and not torch.equal(first, second)
