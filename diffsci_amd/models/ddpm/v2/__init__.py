"""``diffsci.models.ddpmv2``: schedulers, integrators and the module of the DDPM / DDIM family on the HIP sampling path."""
from . import integrators, schedulers  # noqa: F401
from .schedulers import DDPMScheduler, ClassicalDDPMScheduler, CosineDDPMScheduler, ExpDDPMScheduler  # noqa: F401
from .integrators import (Integrator, ClassicalDDPMIntegrator, ClassicalDDPMIntegratorType1, ClassicalDDPMIntegratorType2,  # noqa: F401
                          GeneralizedDDPMIntegrator, DDPMIntegrator, DDIMIntegrator)
from .ddpmmodule import DDPMModule, DDPMModuleConfig  # noqa: F401
