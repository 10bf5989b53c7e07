"""The discrete noise schedules of the DDPM family (reference: diffsci/models/ddpm/v2/schedulers.py).

Host code: every method is plain torch on whatever tensors it is handed, written in the reference's operation order, so the
fp32 tables the integrators build from it (steploop.backward_table) are bit-identical to what the reference's CPU path
computes.  Nothing here touches the GPU.

Quirks of the reference that are kept, because checkpoints and scripts depend on what they compute:
  * every subclass accepts ``T`` and ignores it (it never reaches ``DDPMScheduler.__init__``): ``self.T`` is always 1000;
  * ``ClassicalDDPMScheduler.calpha(t)`` is exp(sum(log(alpha(1..round(t))))) -- a product over the integer steps, computed in
    the default dtype whatever dtype ``t`` has; ``calpha(0)`` is an empty product, 1;
  * an explicit ``T`` argument (the integrators pass ``nsteps``) replaces ``self.T`` in the schedule itself.
"""
import math

import torch


class DDPMScheduler(torch.nn.Module):
    def __init__(self, T: int = 1000):
        super().__init__()
        self.T = T

    def calpha_norm(self, s):
        """alpha-bar as a function of normalised time s = t / T."""
        raise NotImplementedError

    def calpha(self, t, T: None | int = None):
        """alpha-bar_t = calpha_norm(t / T)."""
        if T is None:
            T = self.T
        return self.calpha_norm(t / T)

    def alpha(self, t, T: None | int = None):
        """alpha_t = alpha-bar_t / alpha-bar_(t-1)."""
        return self.calpha(t, T) / self.calpha(t - 1, T)

    def beta(self, t, T: None | int = None):
        return 1 - self.alpha(t, T)


class ClassicalDDPMScheduler(DDPMScheduler):
    """The linear beta schedule of the DDPM paper: beta_t runs from beta0 (t = 1) to beta1T / T (t = T)."""

    def __init__(self, beta1T: float = 20.0, beta0: float = 1e-4, T: int = 1000):
        super().__init__()                                   # T is not handed on (the reference's quirk): self.T = 1000
        self.beta1T = beta1T
        self.beta0 = beta0

    def calpha_norm(self, s):
        raise NotImplementedError

    def calpha(self, t, T: None | int = None):
        """One entry per element of t (iterated along its first axis, so t has at least one): the product of alpha over the
        integer steps 1..round(t), as exp of the summed logs."""
        out = []
        for tt in t:
            steps = torch.round(tt).int().item()
            s = torch.arange(steps).to(t.device) + 1          # int64: the division inside beta() lands in the default dtype
            out.append(torch.exp(torch.sum(torch.log(self.alpha(s, T)))))
        return torch.stack(out, axis=0).reshape(t.shape)

    def alpha(self, t, T: None | int = None):
        return 1.0 - self.beta(t, T)

    def beta(self, t, T: None | int = None):
        T = self.T if T is None else T
        s = (t - 1) / (T - 1)
        return self.beta0 * (1 - s) + self.beta1T / T * s


class ExpDDPMScheduler(DDPMScheduler):
    def __init__(self, beta_data: float = 19.9, beta0: float = 1e-4, T: int = 1000):
        super().__init__()
        self.beta_data = beta_data
        self.beta0 = beta0

    def calpha_norm(self, s):
        return torch.exp(-0.5 * (self.beta_data * s ** 2 + self.beta0))


class CosineDDPMScheduler(DDPMScheduler):
    def __init__(self, stabilizer: float = 0.008, T: int = 1000):
        super().__init__()
        self.stabilizer = stabilizer
        self.f0 = math.cos((stabilizer / (1 + stabilizer) * math.pi / 2)) ** 2

    def calpha_norm(self, s):
        ft = torch.cos(((self.stabilizer + s) / (1 + self.stabilizer) * math.pi / 2)) ** 2
        return ft / self.f0
