"""The Euler-Maruyama runs of the stochastic-interpolant sampler on the fused inpainting step (ds_inpaint.hip): the rows of
SIModule.inpaint (flowfield.py:546-641 of the reference) and of integrate_flow_field(noise_injection=True) (flowfield.py:783-793)
resolved on the host, and the loop that launches them: an engine.LoopBase, which owns the state, the protocol (load, set_inputs,
set_noise, launch, result) and the Philox state, so engine.PlanCache captures and replays it like any other run.

Per row: one network evaluation through the source, one ds_si_inpaint_step.  The state is updated in place; x_orig, the mask,
the start noise and the Philox state (or the injected draws) live in buffers the loop owns, rewritten before every replay.
"""
from dataclasses import dataclass
from typing import List

import torch

from ... import ops
from ..._native import SIStep
from .engine import LoopBase
from .steptable import EvalRow


@dataclass
class SIRow:
    """One inner iteration: the evaluation at the step's start, the step's scalars, and what follows the step."""
    first: EvalRow
    score_a: float
    score_b: float
    score_den: float
    neg_half_omega: float
    dt: float
    noise_coef: float
    patch_alpha: float
    patch_sigma: float
    jump_alpha: float
    jump_sigma: float
    blend: bool = False         # re-impose the known region at the step's end
    jump: bool = False          # then jump back to the step's start and re-impose it there (RePaint)

    def step(self, c_in_next):
        return SIStep(self.score_a, self.score_b, self.score_den, self.neg_half_omega, self.dt, self.noise_coef, self.patch_alpha,
                      self.patch_sigma, self.jump_alpha, self.jump_sigma, float(c_in_next))

    @property
    def draws(self):
        return 4 if self.jump else (2 if self.blend else 1)


@dataclass
class SITable:
    """What engine.ModuleSource and engine.PlanCache read of a step table, for the rows above."""
    t: torch.Tensor
    rows: List[SIRow]
    kind: str = "si-euler-maruyama"
    needs_noise = True

    @property
    def evals(self):
        return [r.first for r in self.rows]

    def digest(self):
        e = lambda v: (v.sigma, v.sigma_sq, v.neg_mult, v.c_skip, v.c_out, v.c_in, v.c_noise)     # noqa: E731
        return (self.kind,) + tuple((e(r.first), r.score_a, r.score_b, r.score_den, r.neg_half_omega, r.dt, r.noise_coef,
                                     r.patch_alpha, r.patch_sigma, r.jump_alpha, r.jump_sigma, r.blend, r.jump) for r in self.rows)


def si_row(config, t_curr, t_next, integrate_on_sigma, blend=False, jump=False):
    """The scalars of SIModule._em_step and of the blend, as 0-dim fp32 CPU tensor arithmetic in the eager chain's order."""
    c = config
    dt = float((c.sigma_fn(t_next) - c.sigma_fn(t_curr)) if integrate_on_sigma else (t_next - t_curr))
    alpha, sigma, alpha_dot, sigma_dot = c.alpha_fn(t_curr), c.sigma_fn(t_curr), c.alpha_fn_dot(t_curr), c.sigma_fn_dot(t_curr)
    den = sigma * (alpha_dot * sigma - alpha * sigma_dot)
    omega = c.sigma_fn(t_curr)
    return SIRow(first=c.preconditioner.eval_row(t_curr, integrate_on_sigma), score_a=float(alpha), score_b=-float(alpha_dot),
                 score_den=float(den), neg_half_omega=-float(0.5 * omega), dt=dt, noise_coef=float(torch.sqrt(omega * abs(dt))),
                 patch_alpha=float(c.alpha_fn(t_next)), patch_sigma=float(c.sigma_fn(t_next)), jump_alpha=float(alpha),
                 jump_sigma=float(sigma), blend=bool(blend), jump=bool(jump))


def inpaint_table(config, nsteps, integrate_on_sigma=False, resample_steps=0, jump_length=1, mask_start_t=1.0):
    """The nsteps-1 x (resample_steps+1) inner iterations of SIModule.inpaint, mask_start_t and jump_length resolved."""
    ts = torch.linspace(1, 0, nsteps)
    rows = []
    for i in range(nsteps - 1):
        t_curr, t_next = ts[i], ts[i + 1]
        for r in range(resample_steps + 1):
            blend = t_next.item() <= mask_start_t
            jump = blend and r < resample_steps and i + jump_length < nsteps - 1
            rows.append(si_row(config, t_curr, t_next, integrate_on_sigma, blend, jump))
    return SITable(t=ts, rows=rows)


def em_table(config, time_schedule, integrate_on_sigma=False):
    """The steps of integrate_flow_field(noise_injection=True): no known region."""
    ts = torch.as_tensor(time_schedule, dtype=torch.float32).detach().cpu()
    return SITable(t=ts, rows=[si_row(config, ts[i], ts[i + 1], integrate_on_sigma) for i in range(ts.numel() - 1)])


class SILoop(LoopBase):
    """The launch sequence of an SITable and the buffers it reads.  Usage: load(x0[, scale]); set_inputs(x_orig, mask);
    set_noise(...); launch(); result() -- or run(x0, scale, draws, (x_orig, mask)).

    Noise: injected_noise=True -- the draws, in the reference's order (per row: the step's [B, *shape], with a blend the patch's
    [1, *shape], with a jump the re-noising [B, *shape] and its patch [1, *shape]), are copied into loop-owned buffers;
    injected_noise=False -- generated in the kernel from the device state, row j at the offset the rows before it consumed
    (ds_inpaint.hip)."""

    def __init__(self, table: SITable, source, like, injected_noise=False):
        super().__init__(table, source, like)
        shape = self.shape
        self.xin = self._new_xin()
        self.masked = any(r.blend for r in table.rows)
        self.x_orig = self._new(shape[1:]) if self.masked else None
        self.mask = self._new(shape[1:]) if self.masked else None
        B, n = shape[0], like.numel() // max(shape[0], 1)
        self.offsets, o = [], 0
        for r in table.rows:
            self.offsets.append(o)
            o += ops.si_inpaint_counters(B, n, r.blend, r.jump)
        self.counters = self.noise_counters = o
        if injected_noise:
            self.eps = [[self._new(shape if i % 2 == 0 else (1,) + shape[1:]) for i in range(r.draws)] for r in table.rows]
        else:
            self._make_rng()

    def set_inputs(self, x_orig=None, mask=None):
        """The known data (network space) and the (soft) mask, [*shape] or [1, *shape]."""
        if not self.masked:
            return
        for dst, src, what in ((self.x_orig, x_orig, "x_orig"), (self.mask, mask, "mask")):
            if src is None or src.numel() != dst.numel():
                raise ValueError(f"{what} must hold one sample of shape {tuple(dst.shape)}")
            dst.copy_(src.reshape(dst.shape))

    def _copy_eps(self, eps):
        flat = [b for row in self.eps for b in row]
        eps = list(eps)
        if len(eps) < len(flat):
            raise ValueError(f"the run consumes {len(flat)} draws; got {len(eps)}")
        for b, e in zip(flat, eps):
            if tuple(e.shape) != tuple(b.shape):
                raise ValueError(f"injected noise has shape {tuple(e.shape)}, expected {tuple(b.shape)}")
            b.copy_(e)

    def row_noise(self, j):
        """The draws of row j as tensors (generator mode regenerates them from the counters: tests / diagnostics)."""
        if self.eps is not None:
            return list(self.eps[j])
        r, shape = self.table.rows[j], tuple(self.x.shape)
        B, n = shape[0], self.x.numel() // shape[0]
        cB, c1 = ops.philox_counters(B * n), ops.philox_counters(n)
        offs = (0, cB, cB + c1, 2 * cB + c1)
        return [ops.philox_normal(self.rng, self.offsets[j] + offs[i], shape if i % 2 == 0 else (1,) + shape[1:])
                for i in range(r.draws)]

    def launch(self, max_rows=None):
        table, source = self.table, self.source
        rows, n = table.rows, len(table.rows)
        kind, g = source.input_kind, source.guidance
        x, xin = self.x, self.xin
        copies = getattr(source, "xin_copies", 1)
        if n > 0:
            for half in self._xin_copies(xin):
                ops.scale(x, rows[0].first.c_in, out=half)
        for j, row in enumerate(rows):
            if max_rows is not None and j >= max_rows:
                break
            nxt = rows[j + 1] if j + 1 < n else None
            k = row.first.coef(kind, g, xin_copies=copies, nonfinite=self.nonfinite_word if j == n - 1 else None)
            f, fu = source.evaluate(x, xin, row.first, j, 0)
            ops.si_inpaint_step(x, f, k, row.step(nxt.first.c_in if nxt is not None else 1.0), fu=fu, x_orig=self.x_orig,
                                mask=self.mask, blend=row.blend, renoise=row.jump,
                                eps=None if self.eps is None else self.eps[j],
                                philox=None if self.rng is None else (self.rng, self.offsets[j]),
                                x_out=x, xin_out=xin if nxt is not None else None)
