"""The DDPM / DDIM family on a real MI355X: ds_ddpm_step against the restatement tests/ddpm_ref.py (fp32 on the CPU, bit for
bit), its in-kernel noise against ops.philox_normal, the range guard's word, DDPMModule against the histories the reference
recorded (tests/golden/ddpm_runs.npz, its draws fed through eps=), and the captured path against the step-by-step one.

Bounds.  Kernel and every step whose F is computed by torch: torch.equal -- the step is one rounding per operation in the
reference's order and its scalars are the host's.  Runs through our networks: rel-L2 < 1e-5 against the reference's fp32 and,
against its fp64, within max(4 x the reference's own fp32-vs-fp64 distance, 2e-6): the referee of tests/test_gpu_ldm_decoder.py.

Sizes: n = 3 (scalar path only), 4099 (float4 body + 3-element tail), a view one float into a buffer (unaligned: all scalar), and
once tests/test_gpu_grid_caps.py's N_A, where the grid-stride loop runs more than once."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ddpm_ref as R  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

REL = 1e-5
N_A = 2752512
FORMS = ("classical", "generalized", "forward")
# c0..c4 of the size a mid-schedule row has (both sides round them to fp32 the same way); every used coefficient is non-trivial
COEFS = {"classical": (0.013952379114925861, 1.0049128532409668, 0.09828366339206696, 0.0, 0.0),
         "generalized": (0.9574294090270996, 0.28866896033287048, 0.29008716344833374, 0.9519214630126953, 0.09467311203479767),
         "forward": (0.9951111674308777, 0.009753942489624023, 0.0, 0.0, 0.0)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def V():
    import diffsci_amd.models as M
    return M.ddpmv2


@pytest.fixture(scope="module")
def runs():
    vals, sd = R.load("runs")
    sd.update(R.load("runs_w1")[1])
    return vals, sd


def referee(got, want32, want64, what=""):
    e32, e64, ref = rel_l2(got, want32), rel_l2(got, want64), rel_l2(want32, want64)
    print(f"{what}: vs fp32 {e32:.2e}; vs fp64 {e64:.2e}; reference fp32 vs fp64 {ref:.2e}")
    assert e32 < REL, (what, e32)
    assert e64 < max(4 * ref, 2e-6), (what, e64, ref)


def _coef(form, word=None):
    from diffsci_amd._native import DDPMCoef
    return DDPMCoef(*COEFS[form], None if word is None else word.data_ptr())


def _inputs(n, seed, unaligned=False):
    """x, f, eps of n elements on the host; unaligned: views that start one float into their buffers."""
    g = torch.Generator().manual_seed(seed)
    bufs = [torch.randn(n + 1, generator=g) for _ in range(3)]
    return [b[1:] if unaligned else b[:n].clone() for b in bufs]


def _on(dev, t, unaligned):
    if not unaligned:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, device=dev)
    buf[1:].copy_(t)
    assert buf[1:].data_ptr() % 16 == 4
    return buf[1:]


@pytest.mark.parametrize("size", ["3", "4099", "4099-unaligned", "N_A"])
@pytest.mark.parametrize("form", FORMS)
def test_step_kernel_equals_the_restatement(dev, form, size):
    from diffsci_amd import ops
    unaligned = size.endswith("unaligned")
    n = N_A if size == "N_A" else int(size.split("-")[0])
    if size == "N_A":
        from tests.test_gpu_grid_caps import N_A as cap
        assert n == cap and n // 4 > 2048 * 256
    x, f, e = _inputs(n, 7 + len(form), unaligned)
    xd, fd, ed = (_on(dev, t, unaligned) for t in (x, f, e))
    if form == "forward":
        f = fd = None
    k = _coef(form)
    for noise in ("none", "eps"):
        want = R.step(form, x, f, e if noise == "eps" else None, COEFS[form][:{"classical": 3, "generalized": 5, "forward": 2}[form]])
        got = ops.ddpm_step(xd, fd, k, form, eps=ed if noise == "eps" else None)                   # out of place, a new tensor
        assert got.data_ptr() != xd.data_ptr() and torch.equal(got.cpu(), want), (form, size, noise)
        assert torch.equal(xd.cpu(), x)                                                            # the input is left alone
        out = _on(dev, torch.zeros(n), unaligned)                                                  # into a given buffer
        assert ops.ddpm_step(xd, fd, k, form, eps=ed if noise == "eps" else None, out=out) is out and torch.equal(out.cpu(), want)
        xi = _on(dev, x, unaligned)                                                                # in place
        ops.ddpm_step(xi, fd, k, form, eps=ed if noise == "eps" else None, out=xi)
        assert torch.equal(xi.cpu(), want), (form, size, noise, "in place")


def _state(dev, seed, base):
    return torch.tensor([seed, base], dtype=torch.int64, device=dev)


@pytest.mark.parametrize("form", FORMS)
def test_in_kernel_noise_is_the_philox_stream(dev, form):
    """Philox mode equals injected mode fed with ops.philox_normal at the same counters -- on the float4 path, the tail and the
    all-scalar path (element e reads counter base + offset + e/4 whatever the path)."""
    from diffsci_amd import ops
    k = _coef(form)
    for n, unaligned, offset in ((3, False, 0), (4099, False, 5), (4099, True, 1 << 33)):
        x, f, _ = _inputs(n, 31, unaligned)
        xd, fd = _on(dev, x, unaligned), (None if form == "forward" else _on(dev, f, unaligned))
        st = _state(dev, 1234567, 40)
        eps = ops.philox_normal(st, offset, (n,))
        want = ops.ddpm_step(xd, fd, k, form, eps=eps)
        got = ops.ddpm_step(xd, fd, k, form, philox=(st, offset))
        assert torch.equal(got, want), (form, n, unaligned)
        assert not torch.equal(got, ops.ddpm_step(xd, fd, k, form, philox=(st, offset + 1)))
        assert float(eps.std()) > 0.5 if n > 100 else True


def test_nonfinite_result_raises_the_word(dev):
    from diffsci_amd import ops
    for form in FORMS:
        for n, at in ((3, 2), (4099, 17), (4099, 4098)):
            x, f, _ = _inputs(n, 5)
            xd, fd = x.to(dev), (None if form == "forward" else f.to(dev))
            word = torch.zeros(1, dtype=torch.int32, device=dev)
            ops.ddpm_step(xd, fd, _coef(form, word), form)
            assert int(word) == 0                                             # a finite result leaves it alone
            xd[at] = float("inf")
            ops.ddpm_step(xd, fd, _coef(form), form)                          # no word handed: nothing to raise
            assert int(word) == 0
            out = ops.ddpm_step(xd, fd, _coef(form, word), form)
            assert int(word) == 1 and not bool(torch.isfinite(out[at]))


def _analytic(x, t):
    return R.predictor(x, t)


@pytest.mark.parametrize("iname,kind", [("type1", "exp"), ("type2", "classical_b3"), ("ddpm", "cosine"), ("ddpm", "exp"), ("ddim", "exp")])
@pytest.mark.parametrize("shape", [(3, 5), (2, 1, 7, 9)])
def test_runs_with_a_torch_predictor_equal_the_restatement_step_by_step(dev, V, iname, kind, shape):
    """F by torch on the device (the analytic predictor): every state of the history is the restatement's step of the state
    before it, given the same F and the same draw -- bit for bit.  Also the single-step methods, and the forward walk."""
    from tests.test_ddpm import INTEGRATORS, KINDS
    integ = INTEGRATORS[iname](KINDS[kind]())
    T = 6
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, generator=g)
    eps = torch.randn(T, *shape, generator=g)
    seen = []

    def predictor(xx, t):
        seen.append((xx.clone(), t.clone(), _analytic(xx, t)))
        return seen[-1][2]
    hist = integ.propagate_backward(x.to(dev), predictor, nsteps=T, record_history=True, eps=eps.to(dev))
    assert tuple(hist.shape) == (T + 1,) + shape and torch.equal(hist[0].cpu(), x) and len(seen) == T
    rows = integ.backward_table(T).rows
    form = R.form_of(iname)
    for i in range(T):
        xx, t, f = seen[i]
        assert torch.equal(xx, hist[i]) and t.tolist() == [float(T - i)] * shape[0]
        want = R.step(form, hist[i].cpu(), f.cpu(), eps[i], rows[i].c[:3 if form == "classical" else 5])
        assert torch.equal(hist[i + 1].cpu(), want), (iname, kind, i)
    final = integ.propagate_backward(x.to(dev), _analytic, nsteps=T, eps=eps.to(dev))
    assert torch.equal(final, hist[-1])
    one = integ.step_backward(x.to(dev), torch.tensor(float(T)), _analytic, T, eps=eps[0].to(dev))
    assert torch.equal(one, hist[1])
    fwd = integ.propagate_forward(x.to(dev), **({"nsteps": T} if form == "generalized" else {"noise_predictor": None, "nsteps": T}),
                                  record_history=True, eps=eps.to(dev))
    frows = integ.forward_table(T).rows
    for i in range(T):
        assert torch.equal(fwd[i + 1].cpu(), R.step("forward", fwd[i].cpu(), None, eps[i], frows[i].c[:2])), (iname, kind, i, "forward")


def _punetg(M, sd, dev, cond=False):
    net = M.PUNetG(M.PUNetGConfig(model_channels=8), conditional_embedding=torch.nn.Linear(3, 8) if cond else None)
    own = {k[len("punetg/"):]: v for k, v in sd.items() if k.startswith("punetg/")}
    if cond:
        own.update({k[len("punetg_cond/"):]: v for k, v in sd.items() if k.startswith("punetg_cond/")})
    net.load_state_dict(own, strict=True)
    return net.to(dev).eval()


def _config(V, name):
    """The fixture's configuration by case name; the classical kind runs its 6 steps with beta1T = 3 (see tools/make_ddpm_golden.py)."""
    if name.startswith("classical"):
        cfg = V.DDPMModuleConfig.from_classical_ddpm(int(name[-1]))
    else:
        maker, kind = name.split("_")
        cfg = getattr(V.DDPMModuleConfig, "from_" + maker)(kind)
    if type(cfg.scheduler) is V.ClassicalDDPMScheduler:
        cfg.change_scheduler(V.ClassicalDDPMScheduler(beta1T=3.0))
    return cfg


RUN_CASES = ["ddpm_classical", "ddim_classical", "ddpm_exp", "ddim_exp", "ddpm_cosine", "ddim_cosine", "classical1", "classical2"]


@pytest.mark.parametrize("name", RUN_CASES)
def test_punetg_histories_against_the_reference(dev, V, runs, name):
    import diffsci_amd.models as M
    vals, sd = runs
    module = V.DDPMModule(_punetg(M, sd, dev), _config(V, name)).to(dev)
    x, eps = vals["x"].to(dev), vals[name + "/eps"].to(dev)
    assert eps.shape[0] == 6                                                   # one recorded draw per step, DDIM included
    hist = module.propagate_toward_sample(x, nsteps=6, record_history=True, eps=eps)
    assert tuple(hist.shape) == (7, 2, 1, 16, 16) and torch.equal(hist[0], x)
    h32, h64 = vals[name + "/hist_f32"], vals[name + "/hist_f64"]
    referee(hist.cpu(), h32, h64, name + " history")
    referee(hist[-1].cpu(), h32[-1], h64[-1], name + " final state")
    module.use_graph = False
    assert torch.equal(module.propagate_toward_sample(x, nsteps=6, record_history=True, eps=eps), hist)
    assert torch.equal(module.propagate_toward_sample(x, nsteps=6, eps=eps), hist[-1])


def test_conditional_history_against_the_reference(dev, V, runs):
    import diffsci_amd.models as M
    vals, sd = runs
    name = "cond_ddpm_cosine"
    module = V.DDPMModule(_punetg(M, sd, dev, cond=True), V.DDPMModuleConfig.from_ddpm("cosine"), conditional=True).to(dev)
    x, eps, y = vals["x"].to(dev), vals[name + "/eps"].to(dev), vals["y"].to(dev)
    hist = module.propagate_toward_sample(x, y, nsteps=6, record_history=True, eps=eps)
    referee(hist.cpu(), vals[name + "/hist_f32"], vals[name + "/hist_f64"], name + " history")
    referee(hist[-1].cpu(), vals[name + "/hist_f32"][-1], vals[name + "/hist_f64"][-1], name + " final state")


def test_mlp_history_against_the_reference_and_step_by_step(dev, V, runs):
    """MLPUncond on [5, 2] (an odd-sized state: the scalar path): through DDPMModule against the recorded history, and with F
    computed by torch on the device every step bit for bit."""
    import diffsci_amd.models as M
    vals, sd = runs
    name = "mlp_ddpm_exp"
    net = M.MLPUncond(2, hidden_dims=[16, 16])
    net.load_state_dict({k[len("mlp/"):]: v for k, v in sd.items() if k.startswith("mlp/")}, strict=True)
    module = V.DDPMModule(net, V.DDPMModuleConfig.from_ddpm("exp")).to(dev)
    x, eps = vals["x_mlp"].to(dev), vals[name + "/eps"].to(dev)
    hist = module.propagate_toward_sample(x, nsteps=6, record_history=True, eps=eps)
    referee(hist.cpu(), vals[name + "/hist_f32"], vals[name + "/hist_f64"], name + " history")
    lin = [(m.weight.detach(), m.bias.detach()) for m in net.net if isinstance(m, torch.nn.Linear)]
    seen = []

    def torch_mlp(xx, t):
        h = torch.cat([xx, t[:, None]], dim=-1)
        for i, (w, b) in enumerate(lin):
            h = torch.nn.functional.linear(h, w, b)
            h = torch.relu(h) if i < len(lin) - 1 else h
        seen.append(h)
        return h
    integ = module.config.integrator
    h2 = integ.propagate_backward(x, torch_mlp, nsteps=6, record_history=True, eps=eps)
    rows = integ.backward_table(6).rows
    for i in range(6):
        assert torch.equal(h2[i + 1].cpu(), R.step("generalized", h2[i].cpu(), seen[i].cpu(), eps[i].cpu(), rows[i].c)), i
    referee(h2.cpu(), vals[name + "/hist_f32"], vals[name + "/hist_f64"], name + " history, F by torch")


def test_toward_noise_history_against_the_reference(dev, V, runs):
    import diffsci_amd.models as M
    vals, sd = runs
    name = "noise_ddpm_exp"
    module = V.DDPMModule(_punetg(M, sd, dev), V.DDPMModuleConfig.from_ddpm("exp")).to(dev)
    x, eps = vals["x"].to(dev), vals[name + "/eps"].to(dev)
    hist = module.propagate_toward_noise(x, 6, record_history=True, eps=eps)
    assert tuple(hist.shape) == (7, 2, 1, 16, 16)
    rows = module.config.integrator.forward_table(6).rows
    for i in range(6):                                                         # no network in it: bit for bit
        assert torch.equal(hist[i + 1].cpu(), R.step("forward", hist[i].cpu(), None, eps[i].cpu(), rows[i].c[:2]))
    referee(hist.cpu(), vals[name + "/hist_f32"], vals[name + "/hist_f64"], name)
    assert torch.equal(module.propagate_toward_noise(x, 6, eps=eps), hist[-1])


# ---------------------------------------------------------------------------------------------------------- capture, generator
def test_captured_run_equals_the_step_by_step_one_and_reuses_its_plan(dev, V, runs):
    import diffsci_amd.models as M
    vals, sd = runs
    module = V.DDPMModule(_punetg(M, sd, dev), V.DDPMModuleConfig.from_ddpm("exp")).to(dev)
    x = vals["x"].to(dev)
    for kw in (dict(eps=vals["ddpm_exp/eps"].to(dev)), dict()):
        module._plans.clear()
        module.use_graph = True
        torch.manual_seed(21)
        a = module.propagate_toward_sample(x, nsteps=6, **kw)
        assert len(module._plans.plans) == 1
        torch.manual_seed(21)
        b = module.propagate_toward_sample(x + 0, nsteps=6, **kw)              # same shapes, another tensor: the plan is replayed
        assert len(module._plans.plans) == 1 and torch.equal(a, b)
        c = module.propagate_toward_sample(x, nsteps=6, **kw)                  # the generator moved on
        assert torch.equal(c, a) == bool(kw)
        hist = module.propagate_toward_sample(x, nsteps=6, record_history=True, **kw)
        assert tuple(hist.shape) == (7,) + tuple(x.shape) and torch.equal(hist[0], x) and len(module._plans.plans) == 2
        module.use_graph = False
        torch.manual_seed(21)
        d = module.propagate_toward_sample(x, nsteps=6, **kw)
        assert torch.equal(a, d) and len(module._plans.plans) == 2
        assert bool(torch.isfinite(a).all())
    torch.manual_seed(5)
    s1 = module.sample(3, [1, 16, 16], nsteps=4, maximum_batch_size=2)
    torch.manual_seed(5)
    s2 = module.sample(3, [1, 16, 16], nsteps=4, maximum_batch_size=2)
    assert tuple(s1.shape) == (3, 1, 16, 16) and torch.equal(s1, s2) and not torch.equal(s1, module.sample(3, [1, 16, 16], nsteps=4))


def test_new_condition_values_refresh_the_captured_plan(dev, V, runs):
    import diffsci_amd.models as M
    vals, sd = runs
    module = V.DDPMModule(_punetg(M, sd, dev, cond=True), V.DDPMModuleConfig.from_ddim("exp"), conditional=True).to(dev)
    x, y = vals["x"].to(dev), vals["y"].to(dev)
    y2 = torch.tensor([-1.1, 0.2, 0.6], device=dev)
    a = module.propagate_toward_sample(x, y, nsteps=5)
    a2 = module.propagate_toward_sample(x, y2, nsteps=5)                       # same structure: the plan's tables are refreshed
    assert len(module._plans.plans) == 1 and not torch.equal(a, a2)
    assert torch.equal(module.propagate_toward_sample(x, y, nsteps=5), a)
    module.use_graph = False
    assert torch.equal(module.propagate_toward_sample(x, y2, nsteps=5), a2)
    assert torch.equal(module.propagate_toward_sample(x, y, nsteps=5), a)


def test_sharded_half_batches_reproduce_the_whole_batch(dev, V, runs):
    """noise_shard: element e of step i reads counter base + i*ceil(total/4) + (first + e)/4, so two half-batches run from the
    same generator state are the whole batch's rows bit for bit."""
    import diffsci_amd.models as M
    vals, sd = runs
    module = V.DDPMModule(_punetg(M, sd, dev), V.DDPMModuleConfig.from_classical_ddpm(2, "exp")).to(dev)
    x = vals["x"].to(dev)
    per_row = x[0].numel()
    for use_graph in (False, True):
        module.use_graph = use_graph
        torch.manual_seed(11)
        full = module.propagate_toward_sample(x, nsteps=5)
        parts = []
        for lo, hi in ((0, 1), (1, 2)):
            torch.manual_seed(11)
            module.noise_shard = (lo * per_row, 2 * per_row)
            try:
                parts.append(module.propagate_toward_sample(x[lo:hi], nsteps=5))
            finally:
                module.noise_shard = None
        assert torch.equal(torch.cat(parts), full)
        torch.manual_seed(11)
        assert not torch.equal(module.propagate_toward_sample(x[1:2], nsteps=5), full[1:2])       # unsharded addressing: other noise
    # the same at the integrator's level, with F by torch
    integ = module.config.integrator
    torch.manual_seed(3)
    whole = integ._run(x, integ.backward_table(4), _analytic, False, None)
    torch.manual_seed(3)
    half = integ._run(x[1:2], integ.backward_table(4), _analytic, False, None, noise_shard=(per_row, 2 * per_row))
    assert torch.equal(half, whole[1:2])
