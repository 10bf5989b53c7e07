"""DDPMModuleConfig / DDPMModule: the sampling surface of the reference (diffsci/models/ddpm/v2/ddpmmodule.py) on the fused
DDPM step (ds_ddpm.hip).

Kept: ``DDPMModuleConfig`` with ``from_classical_ddpm`` / ``from_ddpm`` / ``from_ddim`` / ``change_scheduler``, and
``DDPMModule(model, config, conditional=False)`` with ``sample``, ``propagate_toward_sample``, ``propagate_toward_noise``,
``device``.  ``model`` is a noise predictor ``model(x, t[, y])`` with the state_dict of the reference's.  Training (loss_fn,
training_step, sample_time_for_training, the optimiser hooks) is outside this path, as for KarrasModule.

For a HIP-native network (``forward_with_shifts``: PUNetG, ADM, ...) the per-step time path is tabulated once per run --
embed_time of t = T..1 and the conditional embedding of ``y.unsqueeze(0)`` -- and the whole T-step loop is captured into a
hipGraph and replayed (engine.PlanCache); a new ``y`` of the same structure refreshes the plan's tables before the replay.
Any other ``model`` runs eagerly, step by step, through the same step kernel.  ``use_graph``, ``noise_shard`` and the
precision escalation of nets/precision.py behave as on KarrasModule.

Quirks of the reference that are kept: ``sample`` concatenates its minibatches along axis 0 also when it records histories;
``propagate_toward_noise`` hands ``nsteps`` to the integrator's second parameter, which the classical integrators name
``noise_predictor`` -- with them the forward run has ``scheduler.T`` steps whatever ``nsteps`` says (integrators.py)."""
import torch

from .... import ops
from ...karras.engine import ModuleSource, PlanCache, guarded_run
from ...karras.karrasmodule import dict_unsqueeze, get_minibatch_sizes
from . import integrators, schedulers
from .steploop import DDPMLoop

_SCHEDULERS = {"classical": schedulers.ClassicalDDPMScheduler, "exp": schedulers.ExpDDPMScheduler,
               "cosine": schedulers.CosineDDPMScheduler}


def _scheduler(scheduler):
    """A scheduler by name; anything else (an instance) is taken as it is, as the reference's if-chain does."""
    return _SCHEDULERS[scheduler]() if isinstance(scheduler, str) and scheduler in _SCHEDULERS else scheduler


class DDPMModuleConfig(object):
    def __init__(self, scheduler: schedulers.DDPMScheduler, integrator: integrators.Integrator, loss_metric: str = "huber"):
        self.scheduler = scheduler
        self.integrator = integrator
        self.loss_metric = loss_metric              # stored for drop-in scripts; the sampling path does not read it

    @classmethod
    def from_classical_ddpm(cls, integrator_type: int = 1, scheduler: str = 'classical'):
        scheduler = _scheduler(scheduler)
        if integrator_type == 1:
            integrator = integrators.ClassicalDDPMIntegratorType1(scheduler)
        elif integrator_type == 2:
            integrator = integrators.ClassicalDDPMIntegratorType2(scheduler)
        else:
            raise NotImplementedError
        return cls(scheduler=scheduler, integrator=integrator, loss_metric="huber")

    @classmethod
    def from_ddpm(cls, scheduler: str = 'classical'):
        scheduler = _scheduler(scheduler)
        return cls(scheduler=scheduler, integrator=integrators.DDPMIntegrator(scheduler), loss_metric="huber")

    @classmethod
    def from_ddim(cls, scheduler: str = 'classical'):
        scheduler = _scheduler(scheduler)
        return cls(scheduler=scheduler, integrator=integrators.DDIMIntegrator(scheduler), loss_metric="huber")

    def change_scheduler(self, scheduler):
        self.scheduler = scheduler
        self.integrator.scheduler = scheduler


def _fused(integrator):
    """The built-in step forms: an integrator whose step_backward / propagate_backward are the library's own (noise_injector
    may be a subclass's).  Anything else runs through its own propagate_backward."""
    for base in (integrators.ClassicalDDPMIntegrator, integrators.GeneralizedDDPMIntegrator):
        if isinstance(integrator, base):
            return all(getattr(type(integrator), m) is getattr(base, m) for m in ("step_backward", "propagate_backward"))
    return False


class DDPMModule(torch.nn.Module):
    def __init__(self, model: torch.nn.Module, config: DDPMModuleConfig, conditional: bool = False):
        super().__init__()
        self.model = model
        self.config = config
        self.conditional = conditional
        self.use_graph = True          # capture the loop as a hipGraph for HIP-native networks
        # (first element, total elements) of this process' rows inside a batch sampled by several ranks: see KarrasModule
        self.noise_shard = None
        self._plans = PlanCache()

    @property
    def device(self):
        try:
            return next(self.parameters()).device
        except StopIteration:
            return torch.device("cpu")

    def _apply(self, fn, *a, **k):
        self._plans.clear()
        return super()._apply(fn, *a, **k)

    # ---------------------------------------------------------------- sampling
    def sample(self, nsamples: int, shape: list[int], y=None, nsteps: None | int = None, record_history: bool = False,
               maximum_batch_size: None | int = None):
        """ddpmmodule.py:179-207: CPU-generator white noise, optional minibatching."""
        with torch.inference_mode():
            if maximum_batch_size is not None:
                result = [self.sample(b, shape, y, nsteps, record_history, maximum_batch_size=None)
                          for b in get_minibatch_sizes(nsamples, maximum_batch_size)]
                return torch.cat(result, dim=0)
            white_noise = torch.randn(*([nsamples] + list(shape))).to(self.device)
            return self.propagate_toward_sample(white_noise, y, nsteps, record_history)

    def propagate_toward_sample(self, x, y=None, nsteps: None | int = None, record_history: bool = False, eps=None):
        """ddpmmodule.py:209-231.  eps (extension): injected per-step noise [nsteps, *x.shape]."""
        return self._propagate(x, y, nsteps, record_history, eps)

    def propagate_toward_noise(self, x, nsteps: int = 100, record_history: bool = False, eps=None):
        """ddpmmodule.py:233-246: nsteps goes to the integrator's second parameter (see the module docstring)."""
        kw = {} if eps is None else dict(eps=eps)                  # a user's integrator need not know the extension
        return self.config.integrator.propagate_forward(x, nsteps, record_history=record_history, **kw)

    @ops.device_guard                              # launches go to x's GPU whatever the caller's current device is
    @torch.inference_mode()                        # sampling never differentiates; plan buffers live in one mode
    def _propagate(self, x, y, nsteps, record_history, eps):
        ops.require_device(x, "x")
        if y is not None:
            y = dict_unsqueeze(y, 0)                                     # ddpmmodule.py:216-217: one condition for the batch
        integ = self.config.integrator
        if not _fused(integ):                          # a user's integrator: its own loop, each evaluation as given
            def rhs(xx, t):
                return self.model(xx, t, y) if self.conditional else self.model(xx, t)
            kw = {} if eps is None else dict(eps=eps)
            return integ.propagate_backward(x, rhs, nsteps=nsteps, record_history=record_history, **kw)
        T = integ.scheduler.T if nsteps is None else nsteps
        table = integ.backward_table(T)
        if eps is not None and (eps.shape[0] < len(table.rows) or tuple(eps.shape[1:]) != tuple(x.shape)):
            raise ValueError(f"eps must be [nsteps = {len(table.rows)}, *x.shape]; got {tuple(eps.shape)}")
        # only a planned network is captured (no capture_eager here), and never a run of no steps
        return guarded_run(self._plans, self.model, lambda: ModuleSource(self, y, 1.0, x.shape[0], x), DDPMLoop, table, x, y=y,
                           eps=eps, use_graph=self.use_graph and len(table.rows) > 0, extras=(T,),
                           record_history=record_history, noise_shard=self.noise_shard)
