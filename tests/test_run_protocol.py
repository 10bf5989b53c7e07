"""The run protocol the sampler families share, on the host: the plan key's common part and each family's extras,
the guarded run (capture decision, escalation), PlanCache's bookkeeping, and what a DDPMLoop allocates.  The components that must
matter to a key are the union of what the four drivers' hand-built tuples held before engine.plan_key: a condition, not a
measurement."""
import pytest
import torch

from diffsci_amd import ops
import diffsci_amd.models as M
from diffsci_amd.models.ddpm.v2 import ddpmmodule, steploop
from diffsci_amd.models.karras import engine, flowfield, integrators, karrasmodule, siloop
from diffsci_amd.models.nets import precision

from . import loop_trace

SHAPE = (2, 3, 4, 4)


class Src:
    """What plan_key and guarded_run read of a source."""
    planned, batched_cfg, guidance, nonfinite_word, static_condition = True, False, 1.0, None, False


def _tables():
    ddpm = M.ddpmv2.DDPMIntegrator(M.ddpmv2.ClassicalDDPMScheduler(beta1T=2.0))
    cfg = M.SIModuleConfig(scheduler="linear")
    return {"karras": lambda: loop_trace.karras_table("karras", preconditioned=True),
            "si": lambda: siloop.inpaint_table(cfg, 4, mask_start_t=0.6),
            "ddpm": lambda: ddpm.backward_table(3)}


def _perturb_one_scalar(family, table):
    row = table.rows[1]
    if family == "ddpm":
        row.c = row.c[:3] + (row.c[3] + 0.25,) + row.c[4:]
    else:
        row.dt += 0.25


@pytest.mark.parametrize("family", ["karras", "si", "ddpm"])
def test_every_common_component_of_a_plan_key_matters(family):
    make = _tables()[family]
    model = torch.nn.Linear(2, 2)
    y = {"c": torch.zeros(1, 3), "mode": "a"}

    def key(table=None, src=None, x=torch.zeros(SHAPE), y=y, injected=False, loop_args=None, extras=(7,)):
        return engine.plan_key(table or make(), src or Src(), x, y, model, injected, loop_args or {}, extras)

    base = key()
    assert key() == base and hash(base) == hash(key())                       # equal inputs: one plan
    assert base[0] == make().kind
    src = lambda **kw: type("S", (Src,), kw)()                                # noqa: E731
    changed = {
        "shape": key(x=torch.zeros(2, 3, 4, 5)),
        "device": key(x=torch.zeros(SHAPE, device="meta")),
        "history": key(loop_args=dict(record_history=True)),
        "injected": key(injected=True),
        "guidance": key(src=src(guidance=2.0)),
        "planned": key(src=src(planned=False)),
        "batched guidance": key(src=src(batched_cfg=True)),
        "condition tensor shape": key(y=dict(y, c=torch.zeros(1, 4))),
        "condition leaf value": key(y=dict(y, mode="b")),
        "condition or none": key(y=None),
        "noise_shard": key(loop_args=dict(noise_shard=(8, 200))),
        "extras": key(extras=(8,)),
    }
    table = make()
    _perturb_one_scalar(family, table)
    changed["one scalar of the table"] = key(table=table)
    for what, k in changed.items():
        assert k != base, what
    assert key(y=dict(y, c=torch.ones(1, 3))) == base                         # a condition tensor's VALUES are refreshed, not keyed
    with torch.no_grad():
        model.weight.mul_(1.0)                                                # a parameter's version
    bumped = key()
    assert bumped != base
    model.conv_precision = "fp32"                                            # one of engine.MODEL_SWITCHES
    assert key() != bumped


class Spy:
    """Stands where a driver's guarded_run stood: keeps the call, hands x back."""

    def __call__(self, plans, model, make_source, loop_cls, table, x, **kw):
        self.plans, self.model, self.loop_cls, self.table, self.kw = plans, model, loop_cls, table, kw
        return x


@pytest.fixture
def spy(monkeypatch):
    s = Spy()
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    for mod in (karrasmodule, flowfield, ddpmmodule):
        monkeypatch.setattr(mod, "guarded_run", s)
    return s


def test_karras_hands_its_extras_and_its_loop_arguments(spy):
    mod = M.KarrasModule(torch.nn.Linear(2, 2), M.KarrasModuleConfig.from_edm())
    sch, x = mod.config.noisescheduler, torch.zeros(SHAPE)

    def extras(call=lambda: mod.propagate_toward_sample(x, nsteps=3), **kw):
        call(**kw)
        return spy.kw["extras"]
    base = extras()
    assert extras() == base and spy.loop_cls is engine.Loop and spy.plans is mod._plans and spy.model is mod.model
    assert spy.kw["use_graph"] is mod.use_graph and spy.kw["capture_eager"] is mod.capture_eager
    assert spy.kw["record_history"] is False and spy.kw["noise_shard"] is None and spy.kw["eps"] is None
    assert extras(lambda: mod.propagate_toward_sample(x, nsteps=4)) != base                                     # nsteps
    part = extras(lambda: mod.propagate_partial_toward_sample(x, 0, 3, nsteps=3))
    assert extras(lambda: mod.propagate_partial_toward_sample(x, 1, 3, nsteps=3)) != part                       # i0
    assert extras(lambda: mod.propagate_partial_toward_sample(x, 0, 2, nsteps=3)) != part                       # i1
    churn = lambda **kw: extras(lambda: mod.propagate_toward_sample(x, nsteps=3, integrator=integrators.KarrasIntegrator(**kw)))  # noqa: E731
    ch = churn()
    assert ch != base and spy.table.kind == "karras"
    for kw in (dict(s_schurn=10), dict(s_tmin=0.1), dict(s_tmax=40), dict(s_noise=1.01)):
        assert churn(**kw) != ch, kw                                                                            # the churn parameters
    sch.langevin_const = 2.0
    assert extras() != base
    sch.langevin_const = 1.0
    sch.langevin_interval = (0.1, 1.0)
    assert extras() != base
    sch.langevin_interval = None
    mod.noise_shard = (8, 200)
    mod.propagate_toward_sample(x, nsteps=3, record_history=True, eps=torch.zeros(3, *SHAPE))
    assert spy.kw["record_history"] is True and spy.kw["noise_shard"] == (8, 200) and spy.kw["eps"] is not None


def test_the_interpolant_drivers_hand_integrate_on_sigma(spy):
    mod = M.SIModule(M.SIModuleConfig(scheduler="linear"), torch.nn.Linear(2, 2)).eval()
    x, ts = torch.zeros(SHAPE), torch.linspace(1, 0, 4)
    for ios in (False, True):
        mod.integrate_flow_field(x, ts, integrate_on_sigma=ios, return_history=False)
        assert spy.kw["extras"] == (ios,) and spy.loop_cls is engine.Loop and spy.kw["record_history"] is False
        assert spy.kw["use_graph"] is mod.use_graph and spy.kw["capture_eager"] is mod.capture_eager
        table = siloop.em_table(mod.config, ts, ios)
        draws = [torch.zeros(SHAPE)] * 3
        mod._run_si_table(table, x, None, 1.0, ios, 0.9, ("x_orig", "mask"), draws)
        assert spy.kw["extras"] == (ios,) and spy.loop_cls is siloop.SILoop and spy.table is table
        assert spy.kw["eps"] is draws and spy.kw["inputs"] == ("x_orig", "mask") and spy.kw["scale"] == 0.9


def test_ddpm_hands_T_and_never_captures_a_run_of_no_steps(spy):
    mod = M.ddpmv2.DDPMModule(torch.nn.Linear(2, 2), M.ddpmv2.DDPMModuleConfig.from_ddpm())
    x = torch.zeros(SHAPE)
    mod.propagate_toward_sample(x, nsteps=3)
    assert spy.kw["extras"] == (3,) and spy.loop_cls is steploop.DDPMLoop and spy.kw["use_graph"] is True
    assert "capture_eager" not in spy.kw                                      # its default: only a planned network is captured
    mod.propagate_toward_sample(x, nsteps=4, record_history=True)
    assert spy.kw["extras"] == (4,) and spy.kw["record_history"] is True
    mod.propagate_toward_sample(x, nsteps=0)
    assert len(spy.table.rows) == 0 and spy.kw["use_graph"] is False
    mod.use_graph = False
    mod.propagate_toward_sample(x, nsteps=3)
    assert spy.kw["use_graph"] is False


# ---------------------------------------------------------------------------------------------------------- the guarded run
class StubTable:
    kind = "stub"

    def __init__(self, rows=2):
        self.rows = [None] * rows

    def digest(self):
        return (self.kind, len(self.rows))


class StubLoop:
    made = []

    def __init__(self, table, source, like, injected_noise=False, **loop_args):
        self.source, self.injected, self.loop_args, self.runs = source, injected_noise, loop_args, []
        StubLoop.made.append(self)

    def run(self, x, scale=None, eps=None, inputs=()):
        self.runs.append((scale, eps, inputs))
        return x


class StubPlans:
    def __init__(self):
        self.calls = []

    def run(self, key, make_loop, x, **kw):
        self.calls.append((key, make_loop(), kw))
        return x


class Cuda:
    """A state that says it is on the GPU."""
    is_cuda, shape, device = True, SHAPE, "cuda:0"


@pytest.fixture
def guard(monkeypatch):
    """precision's two entry points under count: flagged[0] runs are flagged before the guard gives in."""
    seen = dict(flagged=0, checked=[], escalated=0)

    def needs_escalation(model, out, *inputs, result_checked=False):
        seen["checked"].append(result_checked)
        seen["flagged"] -= 1
        return seen["flagged"] >= 0

    def escalate(model):
        seen["escalated"] += 1
    monkeypatch.setattr(precision, "needs_escalation", needs_escalation)
    monkeypatch.setattr(precision, "escalate", escalate)
    StubLoop.made = []
    return seen


def _guarded(x, plans, sources, word=None, planned=True, rows=2, **kw):
    def make_source():
        sources.append(type("S", (Src,), dict(nonfinite_word=word, planned=planned))())
        return sources[-1]
    return engine.guarded_run(plans, torch.nn.Linear(2, 2), make_source, StubLoop, StubTable(rows), x, **kw)


def test_a_finite_result_runs_once_and_a_flagged_one_exactly_twice(guard):
    x, plans, sources = torch.zeros(SHAPE), StubPlans(), []
    assert _guarded(x, plans, sources, scale=0.5, eps="e", inputs=(1, 2), record_history=True) is x
    assert len(sources) == 1 and guard["escalated"] == 0 and len(StubLoop.made) == 1
    loop = StubLoop.made[0]
    assert loop.runs == [(0.5, "e", (1, 2))] and loop.injected and loop.loop_args == dict(record_history=True)
    assert plans.calls == []                                                  # a host x never touches the PlanCache
    guard["flagged"] = 1
    assert _guarded(x, plans, sources) is x
    assert guard["escalated"] == 1 and len(sources) == 3 and sources[1] is not sources[2]      # the second run: a new source
    assert [len(lp.runs) for lp in StubLoop.made] == [1, 1, 1] and StubLoop.made[2].source is sources[2]
    guard["flagged"] = 5                                                      # still flagged after the escalation: no third run
    _guarded(x, plans, sources)
    assert guard["escalated"] == 2 and len(sources) == 5


@pytest.mark.parametrize("word,rows,want", [(None, 2, False), ("word", 0, False), ("word", 2, True)])
def test_result_checked_needs_the_guard_word_and_a_last_step(guard, word, rows, want):
    _guarded(torch.zeros(SHAPE), StubPlans(), [], word=word, rows=rows)
    assert guard["checked"] == [want]


def test_which_runs_go_through_the_plan_cache(guard):
    x, plans, sources = Cuda(), StubPlans(), []
    _guarded(x, plans, sources, use_graph=False)
    _guarded(x, plans, sources, planned=False)                                # evaluated as given, capture_eager off
    _guarded(torch.zeros(SHAPE), plans, sources, capture_eager=True)          # on the host
    assert plans.calls == [] and len(StubLoop.made) == 3 and all(len(lp.runs) == 1 for lp in StubLoop.made)
    _guarded(x, plans, sources, y=None, scale=0.5, inputs=(1,), extras=(9,), noise_shard=(8, 200))
    (key, loop, kw), = plans.calls
    assert loop.runs == [] and kw == dict(y=None, scale=0.5, eps=None, torch_graph=False, inputs=(1,))
    assert key[-1] == 9 and (8, 200) in key and sources[-1].static_condition is False
    _guarded(x, plans, sources, planned=False, capture_eager=True, rows=0)    # an empty run is captured like any other here
    key2, _, kw2 = plans.calls[1]
    assert kw2["torch_graph"] is True and sources[-1].static_condition is True and key2 != key


# ---------------------------------------------------------------------------------------------------------- DDPMLoop's buffers
@pytest.mark.parametrize("history,injected", [(False, False), (True, False), (False, True), (True, True)])
def test_ddpm_loop_allocates_the_state_and_the_draws_only(monkeypatch, history, injected):
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    table = _tables()["ddpm"]()
    x = torch.zeros(SHAPE)
    src = engine.ModuleSource(loop_trace.Owner(loop_trace.StubNet(x, x), False), None, 1.0, SHAPE[0], x)
    made, empty = [], torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(empty(*a, **k)) or made[-1])
    loop = steploop.DDPMLoop(table, src, x, history, injected_noise=injected)
    monkeypatch.undo()
    assert loop.xin is None and loop.tmp is None and loop.tmp2 is None
    state_sized = [t for t in made if t.numel() >= x.numel()]
    want = ([] if history else [loop.x]) + ([loop.eps] if injected else [])   # the history is torch.zeros'
    assert len(state_sized) == len(want) and all(a is b for a, b in zip(state_sized, want))
    assert (loop.history is not None) == history and loop.x.shape == x.shape and (loop.rng is None) == injected
