"""Generate tests/golden/ddpm_{tables,steps,runs,runs_w1}.npz: the reference's DDPM / DDIM family (diffsci/models/ddpm/v2) run on the CPU in
fp32 and as an fp64 copy (imported through oracle/tools/refshim.py; needs the reference checkout that shim points at).  The
fixtures are data only: schedule tables, inputs, the recorded draws, the reference's outputs, state_dicts and -- as a JSON
string -- the classes' signatures.  Every file stays under 900 KiB.

The draws are recorded by patching torch.randn_like (the integrators' per-step noise) while a case runs: row i of `eps` is the
i-th call's result.  An fp64 case replays the fp32 case's draws (cast up), so both see the same noise.

    tables  calpha (t = 0..T), alpha, beta (t = 1..T) of the three schedulers and every integrator's sigma_t, T = 1000 and T = 6
    steps   single step_backward / step_forward outputs for the analytic predictor 0.3*x + 0.01*t on [3, 5] and [2, 1, 7, 9]
    runs    6-step histories of DDPMModule over PUNetG(model_channels=8) on [2, 1, 16, 16] (from_ddpm and from_ddim per scheduler
            kind, from_classical_ddpm(1 | 2), one conditional case with a Linear(3, 8) embedding and a tensor y), over
            MLPUncond(2) on [5, 2], and one propagate_toward_noise history of a generalized integrator with nsteps = 6

    python tools/make_ddpm_golden.py"""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
from tests.golden_util import cpu_vendor  # noqa: E402  (before the reference's checkout, which has a `tests` of its own, joins the path)
import refshim  # noqa: E402

refshim.install()
import diffsci.models as M  # noqa: E402
from diffsci.models.ddpm.v2 import integrators as RI, schedulers as RS, ddpmmodule as RM  # noqa: E402

torch.set_num_threads(8)
GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT = 900 << 10
# "classical_b3": beta1T = 3.  The default beta1T = 20 makes beta_t > 1 from t = 3 on when T = 6 (beta_T = beta1T / T), so the
# reference's own 6-step tables, steps and histories are NaN there; they are recorded as they are (tables, steps), and the 6-step
# runs of the classical kind swap this scheduler in through DDPMModuleConfig.change_scheduler
KINDS = {"classical": RS.ClassicalDDPMScheduler, "exp": RS.ExpDDPMScheduler, "cosine": RS.CosineDDPMScheduler,
         "classical_b3": lambda: RS.ClassicalDDPMScheduler(beta1T=3.0)}
INTEGRATORS = {"type1": RI.ClassicalDDPMIntegratorType1, "type2": RI.ClassicalDDPMIntegratorType2, "ddpm": RI.DDPMIntegrator,
               "ddim": RI.DDIMIntegrator}
STEP_TIMES = {1000: (1000, 500, 1), 6: (6, 3, 1)}
STEP_SHAPES = {"a": (3, 5), "b": (2, 1, 7, 9)}


def signature(fn):
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name != "self" and name != "cls":
            d = p.default
            out.append([name, p.kind.name, "<required>" if d is inspect.Parameter.empty else d])
    return out


def signatures():
    classes = {"DDPMScheduler": RS.DDPMScheduler, "ClassicalDDPMScheduler": RS.ClassicalDDPMScheduler,
               "ExpDDPMScheduler": RS.ExpDDPMScheduler, "CosineDDPMScheduler": RS.CosineDDPMScheduler,
               "Integrator": RI.Integrator, "ClassicalDDPMIntegrator": RI.ClassicalDDPMIntegrator,
               "ClassicalDDPMIntegratorType1": RI.ClassicalDDPMIntegratorType1,
               "ClassicalDDPMIntegratorType2": RI.ClassicalDDPMIntegratorType2,
               "GeneralizedDDPMIntegrator": RI.GeneralizedDDPMIntegrator, "DDPMIntegrator": RI.DDPMIntegrator,
               "DDIMIntegrator": RI.DDIMIntegrator, "DDPMModuleConfig": RM.DDPMModuleConfig, "DDPMModule": RM.DDPMModule}
    methods = ("__init__", "calpha", "alpha", "beta", "calpha_norm", "propagate_backward", "propagate_forward", "step_backward",
               "step_forward", "noise_injector", "from_classical_ddpm", "from_ddpm", "from_ddim", "change_scheduler", "sample",
               "propagate_toward_sample", "propagate_toward_noise")
    out = {}
    for cname, cls in classes.items():
        out[cname] = {}
        for m in methods:
            obj = inspect.getattr_static(cls, m, None)
            if obj is None:
                continue
            out[cname][m] = signature(obj.__func__ if isinstance(obj, (classmethod, staticmethod)) else obj)
    return out


class Draws:
    """Patch torch.randn_like (the only generator call of the runs made here; torch.randn is reached from DDPMModule.sample alone):
    record what it returns, or replay a recorded list (cast to the asked dtype)."""

    def __init__(self, replay=None):
        self.replay, self.seen, self.i = replay, [], 0

    def __enter__(self):
        self._rl = torch.randn_like

        def randn_like(x, **kw):
            if self.replay is not None:
                out = self.replay[self.i].to(x.dtype)
                self.i += 1
            else:
                out = self._rl(x, **kw)
            self.seen.append(out)
            return out
        torch.randn_like = randn_like
        return self

    def __exit__(self, *a):
        torch.randn_like = self._rl


def save(name, arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (np.asarray(v.detach().cpu().numpy()) if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrs.items()})
    assert os.path.getsize(path) < LIMIT, (path, os.path.getsize(path))
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} entries", flush=True)


def tables():
    arrs = {"signature": json.dumps(signatures()), "cpu_capability": torch.backends.cpu.get_cpu_capability(),
            "cpu_vendor": cpu_vendor()}
    for kind, cls in KINDS.items():
        sch = cls()
        assert sch.T == 1000 and cls(T=50).T == 1000 if kind != "classical_b3" else True
        for T in (1000, 6):
            t = torch.arange(T).to(torch.float32) + 1
            t0 = torch.arange(T + 1).to(torch.float32)
            p = f"{kind}/T{T}/"
            arrs[p + "calpha"] = sch.calpha(t0, T)
            arrs[p + "alpha"] = sch.alpha(t, T)
            arrs[p + "beta"] = sch.beta(t, T)
            for iname, icls in INTEGRATORS.items():
                arrs[p + "sigma_" + iname] = icls(sch).noise_injector(t, T)
    save("ddpm_tables", arrs)


def predictor(x, t):
    return 0.3 * x + 0.01 * t.reshape((-1,) + (1,) * (x.dim() - 1))


def steps():
    arrs = {}
    torch.manual_seed(510)
    for tag, shape in STEP_SHAPES.items():
        arrs[f"x_{tag}"] = torch.randn(*shape)
        arrs[f"eps_{tag}"] = torch.randn(*shape)
    for kind, cls in KINDS.items():
        sch = cls()
        for iname, icls in INTEGRATORS.items():
            integ = icls(sch)
            for T, times in STEP_TIMES.items():
                for t in times:
                    for tag in STEP_SHAPES:
                        for dt, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
                            x, e = arrs[f"x_{tag}"].to(dt), arrs[f"eps_{tag}"]
                            tt = torch.tensor(float(t), dtype=dt)
                            key = f"{kind}/{iname}/T{T}/t{t}/{tag}/"
                            with Draws(replay=[e]):
                                arrs[key + "back_" + suffix] = integ.step_backward(x, tt, predictor, T)
                            with Draws(replay=[e]):
                                if iname in ("type1", "type2"):
                                    arrs[key + "fwd_" + suffix] = integ.step_forward(x, x, tt, predictor, T)
                                else:
                                    arrs[key + "fwd_" + suffix] = integ.step_forward(x, tt, T)
    save("ddpm_steps", arrs)


def run_pair(make, call, arrs, name):
    """make(dtype) -> module; call(module, dtype) -> history.  Records the fp32 draws and replays them in the fp64 copy."""
    m32 = make(torch.float32)
    with Draws() as d, torch.inference_mode():
        arrs[name + "/hist_f32"] = call(m32, torch.float32)
    arrs[name + "/eps"] = torch.stack(d.seen, 0)
    m64 = make(torch.float64)
    with Draws(replay=d.seen), torch.inference_mode():
        arrs[name + "/hist_f64"] = call(m64, torch.float64)
    assert arrs[name + "/hist_f64"].dtype == torch.float64
    h32, h64 = arrs[name + "/hist_f32"].double(), arrs[name + "/hist_f64"]
    print(f"  {name}: fp32 vs fp64 per state", [f"{float((a - b).norm() / b.norm()):.1e}" for a, b in zip(h32, h64)], flush=True)


def runs():
    arrs, weights = {}, {}
    N = 6
    torch.manual_seed(520)
    net = M.nets.PUNetG(M.nets.PUNetGConfig(model_channels=8)).eval()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                v.add_(0.25 * torch.randn_like(v))
    sd = net.state_dict()
    weights.update({"sd/punetg/" + k: v for k, v in sd.items()})
    cnet = M.nets.PUNetG(M.nets.PUNetGConfig(model_channels=8), conditional_embedding=torch.nn.Linear(3, 8)).eval()
    cnet.load_state_dict({**sd, **{k: v for k, v in cnet.state_dict().items() if k.startswith("conditional_embedding")}})
    csd = cnet.state_dict()
    weights.update({"sd/punetg_cond/" + k: v for k, v in csd.items() if k.startswith("conditional_embedding")})
    mlp = M.nets.MLPUncond(2, hidden_dims=[16, 16]).eval()
    msd = mlp.state_dict()
    weights.update({"sd/mlp/" + k: v for k, v in msd.items()})
    arrs["punetg_keys"] = json.dumps([[k, list(v.shape)] for k, v in sd.items()])
    x = arrs["x"] = torch.randn(2, 1, 16, 16)
    xm = arrs["x_mlp"] = torch.randn(5, 2)
    y = arrs["y"] = torch.tensor([0.7, -0.4, 1.3])

    def punetg(dtype, cond=False):
        if cond:
            n = M.nets.PUNetG(M.nets.PUNetGConfig(model_channels=8), conditional_embedding=torch.nn.Linear(3, 8))
            n.load_state_dict(csd)
        else:
            n = M.nets.PUNetG(M.nets.PUNetGConfig(model_channels=8))
            n.load_state_dict(sd)
        return n.to(dtype).eval()

    def module(net_fn, config, conditional=False):
        def make(dtype):
            cfg = config()
            if type(cfg.scheduler) is RS.ClassicalDDPMScheduler:
                cfg.change_scheduler(KINDS["classical_b3"]())
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return RM.DDPMModule(net_fn(dtype), cfg, conditional=conditional).eval()
        return make

    def sample(xx, yy=None):
        return lambda m, dt: m.propagate_toward_sample(xx.to(dt), None if yy is None else yy.to(dt), nsteps=N, record_history=True)

    for kind in ("classical", "exp", "cosine"):
        run_pair(module(punetg, lambda k=kind: RM.DDPMModuleConfig.from_ddpm(k)), sample(x), arrs, f"ddpm_{kind}")
        run_pair(module(punetg, lambda k=kind: RM.DDPMModuleConfig.from_ddim(k)), sample(x), arrs, f"ddim_{kind}")
    for it in (1, 2):
        run_pair(module(punetg, lambda i=it: RM.DDPMModuleConfig.from_classical_ddpm(i)), sample(x), arrs, f"classical{it}")
    run_pair(module(lambda dt: punetg(dt, True), lambda: RM.DDPMModuleConfig.from_ddpm("cosine"), conditional=True), sample(x, y), arrs,
             "cond_ddpm_cosine")

    def mlpnet(dtype):
        n = M.nets.MLPUncond(2, hidden_dims=[16, 16])
        n.load_state_dict(msd)
        return n.to(dtype).eval()
    run_pair(module(mlpnet, lambda: RM.DDPMModuleConfig.from_ddpm("exp")), sample(xm), arrs, "mlp_ddpm_exp")
    run_pair(module(punetg, lambda: RM.DDPMModuleConfig.from_ddpm("exp")),
             lambda m, dt: m.propagate_toward_noise(x.to(dt), N, record_history=True), arrs, "noise_ddpm_exp")
    save("ddpm_runs", arrs)
    save("ddpm_runs_w1", weights)


if __name__ == "__main__":
    tables()
    steps()
    runs()
