"""The launch sequences of the sampler loops -- engine.Loop, siloop.SILoop, ddpm.v2.steploop.DDPMLoop -- through the recording
stand-in of tests/abi_trace.py (net_trace.Recorder), on the host, and the table of runs whose records are pinned (tests/golden/loop_trace.json,
written by tools/make_loop_trace_golden.py from the PARENT commit's diffsci_amd/).  Per case the record holds every launch (entry
point, scalars with every field of EvalCoef / SIStep / DDPMCoef, pointers as [label, byte offset]), the contents of the Philox
state after set_noise(None, seed_offset=SEED_OFFSET), and where the result lives.  A loop's buffers are labelled by attribute
name once it is built; memory nobody labelled (the source's lazily made outputs, a wrapper's own output) is numbered by first
appearance in a launch ("new0", "new1", ...): every torch.empty / empty_like of a trace is kept alive, so no two share an address.
Host tensors pass for device tensors (the on_host style of tests/test_ddpm.py) and no kernel runs.  diffsci_amd is imported
inside the functions: the golden tool runs this module with the parent's package first on sys.path."""
import ctypes
import math

import torch

from . import net_trace

B = 2
SHAPE = (B, 3, 4, 4)
SEED_OFFSET = (0x5EED, 4000)
STEP_LAUNCHES = ("ds_si_inpaint_step", "ds_ddpm_step")          # launches whose stream is not the last argument
LOOP_BUFFERS = ("history", "x", "xin", "tmp", "tmp2", "eps", "rng", "x_orig", "mask")
# what the issue of the run protocol names: the step kernels and the scale / div launches of the first network input
REQUIRED = {"ds_karras_euler", "ds_karras_heun", "ds_karras_churn", "ds_si_inpaint_step", "ds_ddpm_step", "ds_karras_scale",
            "ds_div_scalar"}


def _number(v):
    """inf and NaN (a schedule with beta_t > 1 has such coefficients) as text: a NaN must equal itself in the golden."""
    return repr(v) if isinstance(v, float) and not math.isfinite(v) else v


class Recorder(net_trace.Recorder):
    def __init__(self, real):
        super().__init__(real, True)
        self._anon, self._seen = [], {}

    def allocated(self, t):
        """A tensor torch.empty / empty_like made during the trace: kept, numbered when a launch first points into it."""
        if isinstance(t, torch.Tensor) and t.numel():
            self._keep.append(t)
            self._anon.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
        return t

    def _pointer(self, p):
        out = super()._pointer(p)
        if out != "fresh":
            return out
        for lo, hi in self._anon:
            if lo <= p < hi:
                return [self._seen.setdefault(lo, f"new{len(self._seen)}"), p - lo]
        return "fresh"

    def _arg(self, v, ctype):
        struct = getattr(ctype, "_type_", None)
        if isinstance(struct, type) and issubclass(struct, ctypes.Structure):
            return [self._pointer(getattr(v._obj, f)) if t is ctypes.c_void_p else _number(getattr(v._obj, f)) for f, t in struct._fields_]
        return _number(super()._arg(v, ctype))

    def __getattr__(self, name):
        if name not in STEP_LAUNCHES:
            return super().__getattr__(name)
        N = net_trace._native()
        types = N._PROTOS[name][1]

        def launch(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            self.calls.append([name] + [self._arg(v, t) for v, t in zip(args, types)])
            return 0
        return launch


class Ctx:
    """What a case builds its run from: named tensors of fixed contents (net_trace.pattern) and `drive`."""

    def __init__(self, rec):
        self.rec, self.k, self.out = rec, 0, {}

    def f(self, label, *shape):
        self.k += 1
        return self.rec.name(label, net_trace.pattern(self.k, *shape))

    def label(self, loop):
        """The loop's buffers by attribute name (x is row 0 of the history when there is one)."""
        for attr in LOOP_BUFFERS:
            t = getattr(loop, attr, None)
            if attr == "x" and getattr(loop, "history", None) is not None:
                continue
            if isinstance(t, torch.Tensor):
                self.rec.name(attr, t)
            elif isinstance(t, list):                                            # SILoop.eps: per row, per draw
                for j, row in enumerate(t):
                    for i, e in enumerate(row):
                        self.rec.name(f"{attr}.{j}.{i}", e)

    def drive(self, loop, x0, scale=None, eps=None, inputs=None, max_rows=None):
        """The protocol, spelled out (the parent's loops have no `run`); generator mode gets SEED_OFFSET, never torch's generator."""
        self.label(loop)
        loop.load(x0, scale)
        if inputs is not None:
            loop.set_inputs(*inputs)
        if loop.rng is not None:
            loop.set_noise(None, seed_offset=SEED_OFFSET)
        else:
            loop.set_noise(eps)
        loop.launch(max_rows)
        self.out = {"rng": None if loop.rng is None else [int(v) for v in loop.rng], "result": self.rec._pointer(loop.result().data_ptr()),
                    "result_shape": list(loop.result().shape)}


class StubNet(torch.nn.Module):
    """A network evaluated as given: a fixed tensor with a condition, another without."""

    def __init__(self, f, fu):
        super().__init__()
        self.f, self.fu = f, fu

    def forward(self, x, t, y=None):
        return self.fu if y is None else self.f


class Owner:
    """What engine.ModuleSource reads of a module."""

    def __init__(self, model, conditional):
        self.model, self.conditional = model, conditional


def karras_table(kind, vp=False, nsteps=3, preconditioned=False):
    from diffsci_amd.models.karras import integrators as I
    from diffsci_amd.models.karras import karrasmodule as K
    from diffsci_amd.models.karras.steptable import build_step_table
    cfg = K.KarrasModuleConfig.from_vp(M=2) if vp else K.KarrasModuleConfig.from_edm()
    integ = {"euler": I.EulerIntegrator, "heun": I.HeunIntegrator, "euler-maruyama": I.EulerMaruyamaIntegrator,
             "karras": I.KarrasIntegrator}[kind]()
    return build_step_table(cfg.noisescheduler, integ, nsteps, preconditioner=cfg.preconditioner if preconditioned else None)


def _karras(c, source, kind="heun", vp=False, history=False, injected=False, shard=False, max_rows=None, state=SHAPE):
    from diffsci_amd.models.karras import engine
    table = karras_table(kind, vp, preconditioned=source is not _score_source)
    x0 = c.f("x0", *state)
    loop = engine.Loop(table, source(c, x0), x0, history, injected_noise=injected,
                       noise_shard=(8, x0.numel() + 16) if shard else None)
    eps = c.f("eps0", len(table.rows), *state) if injected and table.needs_noise else None
    c.drive(loop, x0, scale=None if source is _score_source else 80.0, eps=eps, max_rows=max_rows)


def _score_source(c, x0):
    from diffsci_amd.models.karras import engine
    score = c.f("score", *x0.shape)
    return engine.ScoreFnSource(lambda x, sigma: score, x0.shape[0], x0)


def stub_source(conditional=False, guidance=1.0):
    def source(c, x0):
        from diffsci_amd.models.karras import engine
        net = StubNet(c.f("f", *x0.shape), c.f("fu", *x0.shape))
        y = {"c": c.f("y", 1, 3)} if conditional else None
        return engine.ModuleSource(Owner(net, conditional), y, guidance, x0.shape[0], x0)
    return source


def punetg_source(guidance, per_sample):
    """The smallest PUNetG of net_trace.py, planned: its time path tabulated by prepare, its forward launched per evaluation."""
    def source(c, x0):
        from diffsci_amd.models.karras import engine
        net = net_trace.Net(c.rec, net_trace.Pool(c.rec), output_channels=2).net
        y = c.f("y", B if per_sample else 1, net.config.model_channels)
        src = engine.ModuleSource(Owner(net, True), y, guidance, x0.shape[0], x0)
        assert src.planned and src.batched_cfg == (guidance != 1.0)
        return src
    return source


def _si(c, table="em", pre="identity", injected=False):
    import diffsci_amd.models as M
    from diffsci_amd import _native as N
    from diffsci_amd.models.karras import siloop
    cfg = M.SIModuleConfig(scheduler="linear") if pre == "identity" else M.SIModuleConfig(scheduler="cosine", precondition_fn="edm")
    x0 = c.f("x0", *SHAPE)
    mod = M.SIModule(cfg, StubNet(c.f("f", *SHAPE), c.f("fu", *SHAPE))).eval()
    tab = {"em": lambda: siloop.em_table(mod.config, torch.linspace(1, 0, 4)),
           "blend": lambda: siloop.inpaint_table(mod.config, 4, mask_start_t=0.6),
           "jump": lambda: siloop.inpaint_table(mod.config, 4, resample_steps=1, jump_length=1)}[table]()
    src = mod._source(None, 1.0, x0)
    assert src.input_kind == (N.DS_IN_FLOW if pre == "identity" else N.DS_IN_NETWORK)
    loop = siloop.SILoop(tab, src, x0, injected_noise=injected)
    draws = None
    if injected:
        draws = [c.f(f"draw{j}.{i}", *(SHAPE if i % 2 == 0 else (1,) + SHAPE[1:])) for j, r in enumerate(tab.rows) for i in range(r.draws)]
    c.drive(loop, x0, scale=0.9, eps=draws, inputs=(c.f("x_orig0", *SHAPE[1:]), c.f("mask0", 1, *SHAPE[1:])))


def _ddpm(c, integrator="type1", forward=False, history=False, injected=False, module=False):
    import diffsci_amd.models as M
    from diffsci_amd.models.ddpm.v2 import steploop
    V = M.ddpmv2
    integ = {"type1": V.ClassicalDDPMIntegratorType1, "ddpm": V.DDPMIntegrator, "ddim": V.DDIMIntegrator}[integrator](
        V.ClassicalDDPMScheduler(beta1T=2.0))
    table = integ.forward_table(3) if forward else integ.backward_table(3)
    x0 = c.f("x0", *SHAPE)
    src = stub_source()(c, x0) if module else _score_source(c, x0)
    loop = steploop.DDPMLoop(table, src, x0, history, injected_noise=injected)
    assert loop.xin is None and loop.tmp is None and loop.tmp2 is None
    assert (loop.eps is None and loop.rng is None) == (not table.needs_noise)
    c.drive(loop, x0, eps=c.f("eps0", 3, *SHAPE) if injected else None)          # DDIM is handed eps too: it reads none


def case(run, *args, **kw):
    return run, args, kw


CASES = {
    "score_euler": case(_karras, _score_source, kind="euler"),
    "score_heun": case(_karras, _score_source),
    "score_heun_history": case(_karras, _score_source, history=True),
    "score_heun_max_rows2": case(_karras, _score_source, max_rows=2),
    "score_em_injected": case(_karras, _score_source, kind="euler-maruyama", injected=True),
    "score_em_generator": case(_karras, _score_source, kind="euler-maruyama"),
    "score_em_generator_history": case(_karras, _score_source, kind="euler-maruyama", history=True),
    "score_em_generator_shard": case(_karras, _score_source, kind="euler-maruyama", shard=True),
    "score_karras_injected": case(_karras, _score_source, kind="karras", injected=True),
    "score_karras_generator": case(_karras, _score_source, kind="karras"),
    "score_karras_generator_shard_history": case(_karras, _score_source, kind="karras", shard=True, history=True),
    "score_vp_heun": case(_karras, _score_source, vp=True),
    "score_vp_karras_generator": case(_karras, _score_source, kind="karras", vp=True),
    "stub_unconditional": case(_karras, stub_source()),
    "stub_conditional_g1": case(_karras, stub_source(True, 1.0)),
    "stub_conditional_g2": case(_karras, stub_source(True, 2.0)),
    "stub_conditional_g0": case(_karras, stub_source(True, 0.0)),
    "stub_euler_history": case(_karras, stub_source(), kind="euler", history=True),
    "stub_vp_heun": case(_karras, stub_source(), vp=True),                        # the first network input: div, then scale
    "stub_karras_generator": case(_karras, stub_source(True, 2.0), kind="karras"),
    "stub_em_injected_max_rows2": case(_karras, stub_source(), kind="euler-maruyama", injected=True, max_rows=2),
    "punetg_heun_g2": case(_karras, punetg_source(2.0, False), state=(B, 2, 8, 8)),      # [2B, ...] input, xin_copies = 2
    "punetg_euler_per_sample": case(_karras, punetg_source(1.0, True), kind="euler", state=(B, 2, 8, 8)),
    **{f"si_{t}_{p}_{'injected' if i else 'generator'}": case(_si, table=t, pre=p, injected=i)
       for t in ("em", "blend", "jump") for p in ("identity", "edm") for i in (False, True)},
    "ddpm_classical_injected": case(_ddpm, injected=True),
    "ddpm_classical_generator": case(_ddpm),
    "ddpm_classical_generator_history": case(_ddpm, history=True),
    "ddpm_classical_module_generator": case(_ddpm, module=True),
    "ddpm_generalized_generator": case(_ddpm, integrator="ddpm"),
    "ddpm_generalized_injected_history": case(_ddpm, integrator="ddpm", injected=True, history=True),
    "ddpm_ddim": case(_ddpm, integrator="ddim", injected=True),
    "ddpm_ddim_history": case(_ddpm, integrator="ddim", history=True),
    "ddpm_forward_injected": case(_ddpm, forward=True, injected=True),
    "ddpm_forward_generator_history": case(_ddpm, forward=True, history=True),
}


def trace_of(name):
    """The pinned record of one case."""
    from diffsci_amd import ops
    N = net_trace._native()
    run, args, kw = CASES[name]
    rec = Recorder(N.lib())
    c = Ctx(rec)
    empty, empty_like = torch.empty, torch.empty_like
    saved = [(N, "lib", N.lib), (ops, "_stream", ops._stream), (ops, "_off_device", ops._off_device), (torch, "empty", empty),
             (torch, "empty_like", empty_like)]
    try:
        N.lib, ops._stream, ops._off_device = (lambda: rec), (lambda: 0), (lambda t: None)
        torch.empty = lambda *a, **k: rec.allocated(empty(*a, **k))
        torch.empty_like = lambda *a, **k: rec.allocated(empty_like(*a, **k))
        with torch.inference_mode():
            run(c, *args, **kw)
    finally:
        for mod, attr, v in saved:
            setattr(mod, attr, v)
    return {"calls": rec.calls, **c.out}
