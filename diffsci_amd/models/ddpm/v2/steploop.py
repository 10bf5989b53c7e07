"""Host-built step tables of the DDPM / DDIM integrators and the loop that launches them on ds_ddpm_step.

During a run every sample sits at the same integer time t, so a step's coefficients are scalars.  They are computed here once
per run on the CPU, in fp32, by calling the scheduler and the integrator's ``noise_injector`` on one-element tensors with the
reference's own operation sequence (integrators.py:91-107, 116-122, 197-225), so the numbers handed to the kernel are
bit-identical to the ones the reference's CPU path broadcasts over the state.

The loop is an engine.StepNoiseLoop -- the state or the history, one draw per step, ``noise_shard`` addressing and the run
protocol are the base's -- with its own launch sequence and no buffer of its own; engine.PlanCache captures and replays it.  Per step: one
evaluation through the source -- the network reads the state itself, there is no c_in*x copy -- and one ds_ddpm_step:
read x, read F, write x'.  A row speaks the sources' vocabulary: ``sigma`` and ``c_noise`` are the time handed to the
network (engine.ScoreFnSource passes sigma*ones(B), engine.ModuleSource tabulates embed_time(c_noise))."""
from dataclasses import dataclass
from typing import List, Tuple

import torch

from .... import ops
from ...._native import DDPMCoef
from ...karras.engine import StepNoiseLoop

NOISE_SLOT = {"classical": 2, "generalized": 4, "forward": 1}       # which coefficient multiplies the draw


@dataclass
class DDPMRow:
    time: float                    # t as the network sees it: T, T-1, ..., 1
    form: str                      # "classical" | "generalized" | "forward"
    c: Tuple[float, ...]           # ds_ddpm_coef's c0..c4 (unused ones 0)
    scaled = False

    @property
    def sigma(self):
        return self.time

    @property
    def c_noise(self):
        return self.time

    @property
    def noise_coef(self):
        return self.c[NOISE_SLOT[self.form]]

    def coef(self, nonfinite=None):
        return DDPMCoef(*self.c, None if nonfinite is None else nonfinite.data_ptr())


@dataclass
class DDPMTable:
    kind: str                      # "ddpm-classical" | "ddpm-generalized" | "ddpm-forward"
    rows: List[DDPMRow]

    @property
    def evals(self):
        return self.rows

    @property
    def needs_noise(self):
        """False when no step of the run injects noise (DDIM: sigma_t = 0*t): no eps buffer, no Philox state, no draw."""
        return any(r.noise_coef != 0.0 for r in self.rows)

    def digest(self):
        """Every scalar a captured launch sequence bakes in: the plan key's view of the scheduler and the integrator.  As hex
        strings: a NaN coefficient (a schedule with beta_t > 1) must equal itself, or the key would never hit."""
        return (self.kind,) + tuple((r.time,) + tuple(float(v).hex() for v in r.c) for r in self.rows)


def _f(v):
    return float(torch.as_tensor(v).reshape(-1)[0])


def _times(T):
    """t = T, T-1, ..., 1 as one-element fp32 tensors: the values of arange(T).to(x) + 1, flipped."""
    return [torch.tensor([float(t)], dtype=torch.float32) for t in range(int(T), 0, -1)]


def backward_table(integrator, T, form, times=None):
    """times: the steps' t as one-element fp32 tensors (default T..1; a single step hands its own)."""
    sch, rows = integrator.scheduler, []
    for t in (_times(T) if times is None else times):
        sigma = integrator.noise_injector(t, T)
        calpha = sch.calpha(t, T)
        if form == "classical":                               # integrators.py:93-105
            alpha = sch.alpha(t, T)
            beta = 1 - alpha
            c = (_f(beta / torch.sqrt(1 - calpha)), _f(1 / torch.sqrt(alpha)), _f(sigma), 0.0, 0.0)
        else:                                                 # integrators.py:199-208
            calpha_prev = sch.calpha(t - 1, T)
            c = (_f(torch.sqrt(1 - calpha)), _f(torch.sqrt(calpha)), _f(torch.sqrt(calpha_prev)),
                 _f(torch.sqrt(torch.relu(1 - calpha_prev - sigma ** 2))), _f(sigma))
        rows.append(DDPMRow(_f(t), form, c))
    return DDPMTable("ddpm-" + form, rows)


def forward_table(integrator, T, form, times=None):
    """x -> a*x + b*eps for t = T..1 (the reference's forward loops walk the flipped list too)."""
    sch, rows = integrator.scheduler, []
    for t in (_times(T) if times is None else times):
        if form == "classical":                               # integrators.py:119-121
            beta = sch.beta(t, T)
            a, b = torch.sqrt(1 - beta), torch.sqrt(beta)
        else:                                                 # integrators.py:219-224 (the noise factor is not a square root there)
            calpha, calpha_prev = sch.calpha(t, T), sch.calpha(t - 1, T)
            a, b = torch.sqrt(calpha / calpha_prev), 1 - calpha / calpha_prev
        rows.append(DDPMRow(_f(t), "forward", (_f(a), _f(b), 0.0, 0.0, 0.0)))
    return DDPMTable("ddpm-forward", rows)


class DDPMLoop(StepNoiseLoop):
    """DDPMLoop(table, source, like, record_history=False, injected_noise=False, noise_shard=None); load(x0); set_noise(eps);
    launch(); result().  eps [nsteps, *shape] holds one draw per step in the order of the reference's randn_like calls (it
    draws at every step, also where sigma_t = 0)."""
    xin = tmp = tmp2 = None                               # the evaluation reads the state; the step needs no scratch

    def launch(self, max_rows=None):
        rows, source = self.table.rows, self.source
        n = len(rows)
        cur = self.x
        for i, row in enumerate(rows):
            if max_rows is not None and i >= max_rows:
                break
            nxt = self.history[i + 1] if self.record_history else cur
            f = None if row.form == "forward" else source.evaluate(cur, cur, row, i, 0)[0]
            noisy = row.noise_coef != 0.0
            ops.ddpm_step(cur, f, row.coef(self.nonfinite_word if i == n - 1 else None), row.form,
                          eps=self.eps[i] if (noisy and self.eps is not None) else None,
                          philox=(self.rng, i * self.counters_per_step + self.noise_base) if (noisy and self.rng is not None) else None,
                          out=nxt)
            cur = nxt
        self._final = cur
