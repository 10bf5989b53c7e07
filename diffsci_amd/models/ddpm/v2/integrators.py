"""The DDPM / DDIM integrators (reference: diffsci/models/ddpm/v2/integrators.py) on the fused step kernel.

Names, constructor and method signatures and defaults are the reference's; ``eps`` is the one extension (keyword, last, default
None): the draws of the run, ``[nsteps, *x.shape]`` in the order of the reference's ``randn_like`` calls -- it draws once per
step, also in steps whose sigma_t is 0 (DDIM), so row i always belongs to step i.  Without ``eps`` the draws are generated
inside the kernel by Philox, seeded from ``torch.manual_seed`` through the device generator.

A ``noise_predictor`` is any callable ``(x, t[B]) -> eps_hat`` on device tensors: each evaluation runs as given, each step is
one launch of ds_ddpm_step.  ``t`` counts T, T-1, ..., 1 with T = ``scheduler.T`` or, when given, ``nsteps`` -- which then also
replaces T inside the schedule and is the time the network is handed (the reference's behaviour, kept).

Also kept: the classical ``propagate_forward`` takes ``(x, noise_predictor, nsteps, record_history)`` while the generalized one
takes ``(x, nsteps, record_history)``; ``DDPMModule.propagate_toward_noise`` passes its ``nsteps`` second, so with a classical
integrator it binds to ``noise_predictor`` and the run has ``scheduler.T`` steps.  Both forward loops walk t = T..1.

A subclass may override ``noise_injector`` (it is evaluated on the host, on one-element fp32 tensors, once per step of a run)."""
import torch

from .... import ops
from ...karras.engine import ScoreFnSource
from . import schedulers
from .steploop import DDPMLoop, backward_table, forward_table


class Integrator(torch.nn.Module):
    form = None                      # the kernel form of step_backward: "classical" | "generalized"

    def __init__(self, scheduler: schedulers.DDPMScheduler):
        super().__init__()
        self.scheduler = scheduler

    def propagate_backward(self, x, noise_predictor, nsteps: None | int = None, record_history: bool = False, eps=None):
        raise NotImplementedError

    def propagate_forward(self, x, noise_predictor=None, nsteps: None | int = None, record_history: bool = False, eps=None):
        raise NotImplementedError

    # ------------------------------------------------------------------ what the subclasses share
    def _steps(self, nsteps):
        return self.scheduler.T if nsteps is None else nsteps

    def backward_table(self, T):
        return backward_table(self, T, self.form)

    def forward_table(self, T):
        return forward_table(self, T, self.form)

    @staticmethod
    @ops.device_guard
    @torch.inference_mode()
    def _run(x, table, noise_predictor, record_history, eps, noise_shard=None):
        """One eager pass of `table` over x: the final state (a new tensor) or the history [len(rows)+1, *x.shape]."""
        ops.require_device(x, "x")
        if eps is not None and (eps.shape[0] < len(table.rows) or tuple(eps.shape[1:]) != tuple(x.shape)):
            raise ValueError(f"eps must be [nsteps = {len(table.rows)}, *x.shape]; got {tuple(eps.shape)}")
        return DDPMLoop(table, ScoreFnSource(noise_predictor, x.shape[0], x), x, record_history,
                        injected_noise=eps is not None, noise_shard=noise_shard).run(x, eps=eps)

    def _one(self, x, table, noise_predictor, eps):
        return self._run(x, table, noise_predictor, False, None if eps is None else eps[None])

    def _backward(self, x, noise_predictor, nsteps, record_history, eps):
        return self._run(x, self.backward_table(self._steps(nsteps)), noise_predictor, record_history, eps)

    def _step_table(self, build, t, T):
        """The one-row table of a single step at time t (a 0-dim tensor or a number) under T."""
        tt = torch.as_tensor(t, dtype=torch.float32).detach().cpu().reshape(1)
        return build(self, self._steps(T), self.form, times=[tt])


# ---------------------------------------------------------------------- the formulation of the DDPM paper
class ClassicalDDPMIntegrator(Integrator):
    form = "classical"

    def propagate_backward(self, x, noise_predictor, nsteps: None | int = None, record_history: bool = False, eps=None):
        return self._backward(x, noise_predictor, nsteps, record_history, eps)

    def propagate_forward(self, x, noise_predictor=None, nsteps: None | int = None, record_history: bool = False, eps=None):
        return self._run(x, self.forward_table(self._steps(nsteps)), None, record_history, eps)

    def step_backward(self, x, t, noise_predictor, T: None | int = None, eps=None):
        """x_(t-1) = 1/sqrt(alpha_t) * (x - beta_t/sqrt(1 - alpha-bar_t) * eps_hat(x, t)) + sigma_t * eps."""
        return self._one(x, self._step_table(backward_table, t, T), noise_predictor, eps)

    def step_forward(self, x, x0, t, noise_predictor, T: None | int = None, eps=None):
        """sqrt(1 - beta_t) * x + sqrt(beta_t) * eps (x0 and noise_predictor are not read, as in the reference)."""
        return self._one(x, self._step_table(forward_table, t, T), None, eps)

    def noise_injector(self, t, T: None | int = None):
        raise NotImplementedError


class ClassicalDDPMIntegratorType1(ClassicalDDPMIntegrator):
    def noise_injector(self, t, T: None | int = None):
        return torch.sqrt(self.scheduler.beta(t, T))


class ClassicalDDPMIntegratorType2(ClassicalDDPMIntegrator):
    def noise_injector(self, t, T: None | int = None):
        calpha_prev = self.scheduler.calpha(t - 1, T)
        calpha = self.scheduler.calpha(t, T)
        beta = self.scheduler.beta(t, T)
        return torch.sqrt((1 - calpha_prev) / (1 - calpha) * beta)


# ---------------------------------------------------------------------- the formulation of the DDIM paper
class GeneralizedDDPMIntegrator(Integrator):
    form = "generalized"

    def propagate_backward(self, x, noise_predictor, nsteps: None | int = None, record_history: bool = False, eps=None):
        return self._backward(x, noise_predictor, nsteps, record_history, eps)

    def propagate_forward(self, x, nsteps: None | int = None, record_history: bool = False, eps=None):
        return self._run(x, self.forward_table(self._steps(nsteps)), None, record_history, eps)

    def step_backward(self, x, t, noise_predictor, T: None | int = None, eps=None):
        """x0_hat = (x - sqrt(1 - alpha-bar_t) * eps_hat) / sqrt(alpha-bar_t);
        x_(t-1) = sqrt(alpha-bar_(t-1)) * x0_hat + sqrt(relu(1 - alpha-bar_(t-1) - sigma_t^2)) * eps_hat + sigma_t * eps."""
        return self._one(x, self._step_table(backward_table, t, T), noise_predictor, eps)

    def step_forward(self, x, t, T: None | int = None, eps=None):
        """sqrt(alpha_t) * x + (1 - alpha_t) * eps, alpha_t = alpha-bar_t / alpha-bar_(t-1)."""
        return self._one(x, self._step_table(forward_table, t, T), None, eps)

    def noise_injector(self, t, T: None | int = None):
        raise NotImplementedError


class DDPMIntegrator(GeneralizedDDPMIntegrator):
    def noise_injector(self, t, T: None | int = None):
        calpha_t = self.scheduler.calpha(t, T)
        calpha_t_prev = self.scheduler.calpha(t - 1, T)
        term1sq = (1 - calpha_t_prev) / (1 - calpha_t)
        term2sq = 1 - calpha_t / calpha_t_prev
        return torch.sqrt(term1sq * term2sq)


class DDIMIntegrator(GeneralizedDDPMIntegrator):
    def noise_injector(self, t, T: None | int = None):
        return 0 * t
