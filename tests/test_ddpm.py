"""The DDPM / DDIM family on the host: signatures, schedule tables and step coefficients against what the reference recorded
(tests/golden/ddpm_*.npz, written by tools/make_ddpm_golden.py), the restatement tests/ddpm_ref.py against its recorded steps, the
reference's quirks, and the refusals of ops.ddpm_step.  Nothing is launched: where a loop runs, the library is a recording
stand-in and host tensors pass for device tensors (the `_off_device` style of tests/test_abi_trace.py).

Tables are bit-exact on a host whose torch CPU kernels are the fixtures' (exp / log / cos differ in the last place between
vectorised kernel sets; golden_util.same_cpu_arithmetic is the project's test for that) and within 2 ulp elsewhere."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

from diffsci_amd import _native as N
from diffsci_amd import ops
import diffsci_amd.models as M

from . import ddpm_ref as R
from .golden_util import rel_l2

V = M.ddpmv2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"classical": V.ClassicalDDPMScheduler, "exp": V.ExpDDPMScheduler, "cosine": V.CosineDDPMScheduler,
         "classical_b3": lambda: V.ClassicalDDPMScheduler(beta1T=3.0)}
INTEGRATORS = {"type1": V.ClassicalDDPMIntegratorType1, "type2": V.ClassicalDDPMIntegratorType2, "ddpm": V.DDPMIntegrator,
               "ddim": V.DDIMIntegrator}
STEP_TIMES = {1000: (1000, 500, 1), 6: (6, 3, 1)}


@pytest.fixture(scope="module")
def tables():
    return R.load("tables")[0]


@pytest.fixture(scope="module")
def steps():
    return R.load("steps")[0]


def _same_isa(tables):
    from .golden_util import cpu_vendor
    return tables["cpu_capability"] == torch.backends.cpu.get_cpu_capability() and tables["cpu_vendor"] == cpu_vendor()


def _exact(got, want, tables, what):
    if _same_isa(tables):
        assert R.same(got, want), what
    else:
        assert torch.equal(got.isnan(), want.isnan()), what
        torch.testing.assert_close(got, want, rtol=3e-7, atol=0, equal_nan=True, msg=what)


def _signature(fn):
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name not in ("self", "cls"):
            out.append([name, p.kind.name, "<required>" if p.default is inspect.Parameter.empty else p.default])
    return out


def test_signatures_and_defaults_are_the_references(tables):
    ref = json.loads(tables["signature"])
    assert len(ref) == 13 and "sample" in ref["DDPMModule"] and "from_ddim" in ref["DDPMModuleConfig"]
    for cname, methods in ref.items():
        cls = getattr(V, cname, None) or getattr(V.integrators, cname)
        for mname, want in methods.items():
            if mname in ("loss_fn", "training_step"):
                continue
            obj = inspect.getattr_static(cls, mname)
            assert isinstance(obj, classmethod) == (mname.startswith("from_")), (cname, mname)
            got = json.loads(json.dumps(_signature(obj.__func__ if isinstance(obj, classmethod) else obj)))
            assert got[:len(want)] == want, f"{cname}.{mname}\n  reference: {want}\n  ours:      {got}"
            for name, kind, default in got[len(want):]:                  # extensions come last and have defaults
                assert name == "eps" and default is None and kind == "POSITIONAL_OR_KEYWORD", (cname, mname, name)
    for absent in ("loss_fn", "training_step", "sample_time_for_training", "configure_optimizers"):
        assert not hasattr(V.DDPMModule, absent)


def test_namespace_resolves_as_in_the_reference():
    assert M.ddpmv2.DDPMModule is V.DDPMModule and M.ddpmv2.DDPMModuleConfig.from_ddim
    import diffsci_amd.models.ddpm as D
    assert D.ddpmv2 is M.ddpmv2 and not hasattr(D, "ddpmv1")
    for name in ("DDPMScheduler", "ClassicalDDPMScheduler", "CosineDDPMScheduler", "ExpDDPMScheduler", "DDPMIntegrator",
                 "DDIMIntegrator", "DDPMModule", "DDPMModuleConfig"):                      # the reference's v2/__init__ list
        assert hasattr(M.ddpmv2, name)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("T", [1000, 6])
def test_schedule_tables_equal_the_references(tables, kind, T):
    sch = KINDS[kind]()
    t = torch.arange(T).to(torch.float32) + 1
    p = f"{kind}/T{T}/"
    _exact(sch.calpha(torch.arange(T + 1).to(torch.float32), T), tables[p + "calpha"], tables, p + "calpha")
    _exact(sch.alpha(t, T), tables[p + "alpha"], tables, p + "alpha")
    _exact(sch.beta(t, T), tables[p + "beta"], tables, p + "beta")
    ref = R.Schedule(kind)
    _exact(ref.calpha(torch.arange(T + 1).to(torch.float32), T), tables[p + "calpha"], tables, p + "calpha (ddpm_ref)")
    for iname, icls in INTEGRATORS.items():
        _exact(icls(sch).noise_injector(t, T), tables[p + "sigma_" + iname], tables, p + iname)
        _exact(R.sigma(iname, ref, t, T), tables[p + "sigma_" + iname], tables, p + iname + " (ddpm_ref)")
    if kind != "classical":
        assert bool(torch.isfinite(tables[p + "sigma_ddpm"]).all())
    elif T == 6:
        assert bool(tables[p + "beta"][2:].gt(1).all()) and bool(tables[p + "calpha"][3:].isnan().all())     # the reference's own NaN


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("iname", sorted(INTEGRATORS))
def test_step_tables_hold_the_references_scalars(kind, iname):
    """The per-step scalars handed to the kernel are the restatement's, element for element (same host, same torch: exact)."""
    sch, ref = KINDS[kind](), R.Schedule(kind)
    integ = INTEGRATORS[iname](sch)
    T = 6
    tab, fwd = integ.backward_table(T), integ.forward_table(T)
    assert tab.kind == "ddpm-" + R.form_of(iname) and fwd.kind == "ddpm-forward" and len(tab.rows) == len(fwd.rows) == T
    assert tab.needs_noise == (iname != "ddim") and fwd.needs_noise
    for i, t in enumerate(range(T, 0, -1)):
        tt = torch.tensor([float(t)])
        want = [float(v) for v in R.backward_coefs(iname, ref, tt, T)]
        got = tab.rows[i].c[:len(want)]
        assert tab.rows[i].time == tab.rows[i].c_noise == float(t)
        assert R.same(torch.tensor(got), torch.tensor(want)), (kind, iname, t, got, want)
        wf = [float(v) for v in R.forward_coefs(iname, ref, tt, T)]
        assert R.same(torch.tensor(fwd.rows[i].c[:2]), torch.tensor(wf)), (kind, iname, t)
    assert tab.digest() == integ.backward_table(T).digest() != integ.backward_table(T - 1).digest()


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("iname", sorted(INTEGRATORS))
def test_ddpm_ref_reproduces_the_references_steps(steps, tables, kind, iname):
    ref, worst = R.Schedule(kind), 0.0
    for T, times in STEP_TIMES.items():
        for t in times:
            for tag in ("a", "b"):
                key = f"{kind}/{iname}/T{T}/t{t}/{tag}/"
                for dt, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
                    x, e = steps[f"x_{tag}"].to(dt), steps[f"eps_{tag}"].to(dt)
                    tt = torch.full((x.shape[0],) + (1,) * (x.dim() - 1), float(t), dtype=dt)
                    f = R.predictor(x, tt.reshape(-1))
                    back = R.step(R.form_of(iname), x, f, e, R.backward_coefs(iname, ref, tt, T))
                    fwd = R.step("forward", x, None, e, R.forward_coefs(iname, ref, tt, T))
                    for got, want in ((back, steps[key + "back_" + suffix]), (fwd, steps[key + "fwd_" + suffix])):
                        assert got.dtype == want.dtype == dt
                        if dt == torch.float32:
                            _exact(got, want, tables, key)
                        elif bool(want.isnan().any()):
                            assert torch.equal(got.isnan(), want.isnan()), key
                        else:
                            worst = max(worst, rel_l2(got, want))
    print(f"{kind}/{iname}: worst fp64 rel-L2 {worst:.2e}")
    assert worst < 1e-12


def test_ddim_without_noise_equals_the_references_step_with_its_draw(steps):
    """sigma_t = 0*t: the reference adds 0 * eps; dropping the term changes no value."""
    ref = R.Schedule("exp")
    for tag in ("a", "b"):
        x = steps[f"x_{tag}"]
        tt = torch.full((x.shape[0],) + (1,) * (x.dim() - 1), 500.0)
        got = R.step("generalized", x, R.predictor(x, tt.reshape(-1)), None, R.backward_coefs("ddim", ref, tt, 1000))
        assert torch.equal(got, steps[f"exp/ddim/T1000/t500/{tag}/back_f32"])


# ---------------------------------------------------------------------------------------------------------- quirks
def test_every_subclass_ignores_its_T():
    for cls in (V.ClassicalDDPMScheduler, V.ExpDDPMScheduler, V.CosineDDPMScheduler):
        assert cls(T=50).T == 1000
    assert V.DDPMScheduler(T=50).T == 50
    s = V.ClassicalDDPMScheduler()
    assert float(s.calpha(torch.tensor([0.0]))) == 1.0                                     # the empty product
    assert s.calpha(torch.tensor([3.0], dtype=torch.float64)).dtype == torch.float32       # built from an int64 arange
    t = torch.tensor([3.0])
    assert torch.equal(s.calpha(t), torch.exp(torch.sum(torch.log(s.alpha(torch.arange(3) + 1)))).reshape(1))
    assert torch.equal(s.calpha(torch.tensor([2.6])), s.calpha(t))                         # round(t)
    cfg = V.DDPMModuleConfig.from_ddpm("exp")
    other = V.CosineDDPMScheduler()
    cfg.change_scheduler(other)
    assert cfg.scheduler is other and cfg.integrator.scheduler is other and cfg.loss_metric == "huber"
    with pytest.raises(NotImplementedError):
        V.DDPMModuleConfig.from_classical_ddpm(3)


class StandIn:
    """Stands where N.lib() stood: ds_ddpm_step is recorded, nothing else is reachable."""

    def __init__(self):
        self.calls = []

    def ds_ddpm_step(self, *args):
        self.calls.append(args)
        return 0


@pytest.fixture
def on_host(monkeypatch):
    rec = StandIn()
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(N, "lib", lambda: rec)
    return rec


def _flags(call):
    return call[-1] & 3, call[-1] & 12


def test_nsteps_replaces_T_in_the_schedule_and_in_the_networks_time(on_host):
    seen = []

    def predictor(x, t):
        seen.append(t.clone())
        return torch.zeros_like(x)
    x = torch.randn(3, 5)
    integ = V.DDPMIntegrator(V.ClassicalDDPMScheduler(beta1T=2.0))
    hist = integ.propagate_backward(x, predictor, nsteps=4, record_history=True, eps=torch.randn(4, 3, 5))
    assert tuple(hist.shape) == (5, 3, 5) and torch.equal(hist[0], x)
    assert [t.tolist() for t in seen] == [[float(v)] * 3 for v in (4, 3, 2, 1)] and seen[0].dtype == torch.float32
    assert len(on_host.calls) == 4
    # t = 1: alpha-bar_0 = 1 makes sigma_1 = 0 -- no draw is read there
    assert [_flags(c) for c in on_host.calls] == [(N.DS_DDPM_GENERALIZED, N.DS_DDPM_NOISE_EPS)] * 3 + [(N.DS_DDPM_GENERALIZED, 0)]
    assert integ.backward_table(4).rows[0].c == V.DDPMIntegrator(V.ClassicalDDPMScheduler(beta1T=2.0)).backward_table(4).rows[0].c != \
        integ.backward_table(1000).rows[0].c
    out = integ.propagate_backward(x, predictor, nsteps=4, eps=torch.randn(6, 3, 5))       # more rows than steps: the first four
    assert tuple(out.shape) == (3, 5)
    del on_host.calls[:]
    V.DDIMIntegrator(V.ExpDDPMScheduler()).propagate_backward(x, predictor, nsteps=3, eps=torch.randn(3, 3, 5))
    assert [_flags(c) for c in on_host.calls] == [(N.DS_DDPM_GENERALIZED, N.DS_DDPM_NOISE_NONE)] * 3
    with pytest.raises(ValueError):
        integ.propagate_backward(x, predictor, nsteps=4, eps=torch.randn(3, 3, 5))         # one draw per step
    with pytest.raises(ValueError):
        integ.propagate_backward(x, predictor, nsteps=4, eps=torch.randn(4, 3, 4))


def test_the_classical_forward_binding_is_kept(on_host):
    """propagate_toward_noise(x, nsteps) hands nsteps to the integrator's second parameter: `noise_predictor` on the classical
    integrators, which therefore walk scheduler.T steps; `nsteps` on the generalized ones."""
    x = torch.randn(1, 2)
    net = torch.nn.Linear(2, 2)
    m = V.DDPMModule(net, V.DDPMModuleConfig.from_classical_ddpm(1))
    out = m.propagate_toward_noise(x, 5, eps=torch.randn(1000, 1, 2))
    assert len(on_host.calls) == 1000 and tuple(out.shape) == (1, 2)
    assert all(_flags(c) == (N.DS_DDPM_FORWARD, N.DS_DDPM_NOISE_EPS) and c[2] is None for c in on_host.calls)
    del on_host.calls[:]
    m = V.DDPMModule(net, V.DDPMModuleConfig.from_ddim("exp"))
    hist = m.propagate_toward_noise(x, 5, record_history=True, eps=torch.randn(5, 1, 2))
    assert len(on_host.calls) == 5 and tuple(hist.shape) == (6, 1, 2) and torch.equal(hist[0], x)
    assert list(inspect.signature(V.ClassicalDDPMIntegrator.propagate_forward).parameters)[1:3] == ["x", "noise_predictor"]
    assert list(inspect.signature(V.GeneralizedDDPMIntegrator.propagate_forward).parameters)[1:3] == ["x", "nsteps"]


def test_single_steps_launch_one_kernel_each(on_host):
    x = torch.randn(2, 3)
    e = torch.randn(2, 3)
    pred = lambda xx, t: 0.5 * xx          # noqa: E731
    c = V.ClassicalDDPMIntegratorType2(V.ExpDDPMScheduler())
    g = V.DDPMIntegrator(V.CosineDDPMScheduler())
    c.step_backward(x, torch.tensor(7.0), pred, eps=e)
    c.step_forward(x, x, torch.tensor(7.0), pred, eps=e)
    g.step_backward(x, torch.tensor(7.0), pred, 20, eps=e)
    g.step_forward(x, torch.tensor(7.0), 20, eps=e)
    assert [_flags(k)[0] for k in on_host.calls] == [N.DS_DDPM_CLASSICAL, N.DS_DDPM_FORWARD, N.DS_DDPM_GENERALIZED, N.DS_DDPM_FORWARD]
    k = on_host.calls[2][3]._obj
    want = [float(v) for v in R.backward_coefs("ddpm", R.Schedule("cosine"), torch.tensor([7.0]), 20)]
    assert [k.c0, k.c1, k.c2, k.c3, k.c4] == want and k.nonfinite is None


# ---------------------------------------------------------------------------------------------------------- the wrapper
def test_coefficient_struct_matches_the_header():
    src = open(os.path.join(ROOT, "include", "diffsci_hip.h")).read()
    body = re.search(r"typedef struct ds_ddpm_coef \{(.*?)\} ds_ddpm_coef;", src, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "float c0, c1, c2, c3, c4; uint32_t* nonfinite;"
    assert [n for n, _ in N.DDPMCoef._fields_] == ["c0", "c1", "c2", "c3", "c4", "nonfinite"]
    assert ctypes.sizeof(N.DDPMCoef) == 32 and N.DDPMCoef.nonfinite.offset == 24
    res, args = N._PROTOS["ds_ddpm_step"]
    assert res is ctypes.c_int and args[-2] is ctypes.c_void_p and args[-1] is ctypes.c_int      # ..., void* stream, int flags
    for name in ("DS_DDPM_CLASSICAL", "DS_DDPM_GENERALIZED", "DS_DDPM_FORWARD", "DS_DDPM_NOISE_NONE", "DS_DDPM_NOISE_EPS",
                 "DS_DDPM_NOISE_PHILOX"):
        assert int(re.search(name + r" = (\d+)", src).group(1)) == getattr(N, name)
    assert N.ABI_VERSION == 4


def test_ddpm_step_refuses_what_a_kernel_would_overrun_or_misread(on_host):
    k = N.DDPMCoef(0.1, 1.0, 0.5, 0.0, 0.0, None)
    x, f, e = torch.randn(2, 3, 4), torch.randn(2, 3, 4), torch.randn(2, 3, 4)
    state = torch.zeros(2, dtype=torch.int64)
    ok = ops.ddpm_step(x, f, k, "classical", eps=e)
    assert tuple(ok.shape) == (2, 3, 4) and len(on_host.calls) == 1 and on_host.calls[0][-3] == 24
    assert ops.ddpm_step(x, f, k, "generalized", out=x) is x and ops.ddpm_step(x, None, k, "forward", philox=(state, 8)).shape == x.shape
    assert [c[-1] for c in on_host.calls] == [0 | 4, 1 | 0, 2 | 8] and on_host.calls[2][5:7] == (state.data_ptr(), 8)
    del on_host.calls[:]
    big = torch.randn(2, 2, 3, 4)
    refused = [
        (ValueError, lambda: ops.ddpm_step(x, f[:1], k, "classical")),                                  # f shorter than x
        (ValueError, lambda: ops.ddpm_step(x, f, k, "classical", eps=e[:, :2])),                        # eps shorter than x
        (ValueError, lambda: ops.ddpm_step(x, f, k, "classical", out=torch.empty(2, 3, 3))),            # out smaller
        (ValueError, lambda: ops.ddpm_step(x, f, k, "classical", out=torch.empty(24))),                 # out of another shape
        (ValueError, lambda: ops.ddpm_step(big[0], f, k, "classical", out=big.view(-1)[4:28].view(2, 3, 4))),   # out overlaps x, shifted
        (ValueError, lambda: ops.ddpm_step(x, f, k, "classical", out=f)),                               # out is an input
        (ValueError, lambda: ops.ddpm_step(x, f, k, "classical", eps=e, out=e)),
        (ValueError, lambda: ops.ddpm_step(x, None, k, "classical")),                                   # the backward forms read f
        (ValueError, lambda: ops.ddpm_step(x, f, k, "forward")),
        (ValueError, lambda: ops.ddpm_step(x, f, k, "heun")),
        (ValueError, lambda: ops.ddpm_step(x, f, k, "classical", eps=e, philox=(state, 0))),
        (ValueError, lambda: ops.ddpm_step(x.transpose(0, 1), f.transpose(0, 1), k, "classical")),      # not contiguous
        (TypeError, lambda: ops.ddpm_step(x.double(), f, k, "classical")),                              # dtypes
        (TypeError, lambda: ops.ddpm_step(x, f.half(), k, "classical")),
        (TypeError, lambda: ops.ddpm_step(x, f, k, "classical", eps=e.double())),
        (TypeError, lambda: ops.ddpm_step(x, f, ops.EvalCoef(), "classical")),                          # another struct
        (TypeError, lambda: ops.ddpm_step(x, f, k, "classical", philox=(state.int(), 0))),
        (TypeError, lambda: ops.ddpm_step(x, f, k, "classical", philox=(torch.zeros(3, dtype=torch.int64), 0))),
        (TypeError, lambda: ops.ddpm_step([1.0], f, k, "classical")),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
    assert on_host.calls == []


def test_ddpm_step_refuses_host_tensors(monkeypatch):
    """Without the stand-in's device predicate: a tensor in host memory never reaches a launch."""
    rec = StandIn()
    monkeypatch.setattr(N, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    k = N.DDPMCoef(0.1, 1.0, 0.5, 0.0, 0.0, None)
    x = torch.randn(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ddpm_step(x, x.clone(), k, "classical")
    monkeypatch.setattr(ops, "_off_device", lambda t: None if t.dtype == torch.float32 else "host")
    with pytest.raises(TypeError, match="philox state"):
        ops.ddpm_step(x, x.clone(), k, "classical", philox=(torch.zeros(2, dtype=torch.int64), 0))
    assert rec.calls == []
