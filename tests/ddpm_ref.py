"""The DDPM / DDIM family restated as plain torch (own code; no import of diffsci_amd or of the reference): the three schedules,
every integrator's sigma_t, the step coefficients and the three step forms, each in the operation order of
diffsci/models/ddpm/v2 -- so that in fp32 it is bit-identical to the reference's CPU path and in fp64 to its fp64 copy
(tests/test_ddpm.py checks both against tests/golden/ddpm_steps.npz).  The GPU tests compare the kernel with `step` on the CPU.

Times are tensors of the working dtype (the reference's `arange(T).to(x) + 1`).  The classical schedule's alpha-bar is a product
over integer steps, computed in fp32 whatever the working dtype (the reference builds it from an int64 arange, whose division
lands in the default dtype); everything else follows the dtype of t."""
import math

import torch

SCHEDULES = {"classical": dict(beta1T=20.0, beta0=1e-4), "exp": dict(beta_data=19.9, beta0=1e-4), "cosine": dict(stabilizer=0.008),
             "classical_b3": dict(beta1T=3.0, beta0=1e-4)}


class Schedule:
    def __init__(self, kind, T=1000):
        self.kind, self.p, self.T = kind.split("_")[0], SCHEDULES[kind], T

    def _norm(self, s):
        if self.kind == "exp":
            return torch.exp(-0.5 * (self.p["beta_data"] * s ** 2 + self.p["beta0"]))
        st = self.p["stabilizer"]
        f0 = math.cos((st / (1 + st) * math.pi / 2)) ** 2
        return torch.cos(((st + s) / (1 + st) * math.pi / 2)) ** 2 / f0

    def beta(self, t, T):
        if self.kind == "classical":
            s = (t - 1) / (T - 1)
            return self.p["beta0"] * (1 - s) + self.p["beta1T"] / T * s
        return 1 - self.alpha(t, T)

    def alpha(self, t, T):
        if self.kind == "classical":
            return 1.0 - self.beta(t, T)
        return self.calpha(t, T) / self.calpha(t - 1, T)

    def calpha(self, t, T):
        if self.kind != "classical":
            return self._norm(t / T)
        out = []
        for v in t.reshape(-1):
            k = torch.arange(int(torch.round(v))) + 1                     # int64 -> alpha in fp32
            out.append(torch.exp(torch.sum(torch.log(self.alpha(k, T)))))
        return torch.stack(out).reshape(t.shape)


def sigma(integrator, sch, t, T):
    """noise_injector of "type1" | "type2" | "ddpm" | "ddim"."""
    if integrator == "ddim":
        return 0 * t
    if integrator == "type1":
        return torch.sqrt(sch.beta(t, T))
    prev, cur = sch.calpha(t - 1, T), sch.calpha(t, T)
    if integrator == "type2":
        return torch.sqrt((1 - prev) / (1 - cur) * sch.beta(t, T))
    return torch.sqrt(((1 - prev) / (1 - cur)) * (1 - cur / prev))


def form_of(integrator):
    return "classical" if integrator in ("type1", "type2") else "generalized"


def backward_coefs(integrator, sch, t, T):
    """c0.. of the backward step at time t (a tensor), as tensors of t's shape."""
    sg, ca = sigma(integrator, sch, t, T), sch.calpha(t, T)
    if form_of(integrator) == "classical":
        al = sch.alpha(t, T)
        return ((1 - al) / torch.sqrt(1 - ca), 1 / torch.sqrt(al), sg)
    cp = sch.calpha(t - 1, T)
    return (torch.sqrt(1 - ca), torch.sqrt(ca), torch.sqrt(cp), torch.sqrt(torch.relu(1 - cp - sg ** 2)), sg)


def forward_coefs(integrator, sch, t, T):
    if form_of(integrator) == "classical":
        b = sch.beta(t, T)
        return (torch.sqrt(1 - b), torch.sqrt(b))
    r = sch.calpha(t, T) / sch.calpha(t - 1, T)
    return (torch.sqrt(r), 1 - r)


def step(form, x, f, e, c):
    """One step; c: the form's coefficients (tensors that broadcast against x, or numbers -- taken in x's dtype); e None: no noise."""
    c = [v if torch.is_tensor(v) else torch.tensor(v, dtype=x.dtype) for v in c]
    if form == "classical":
        r = c[1] * (x - c[0] * f)
        return r if e is None else r + c[2] * e
    if form == "generalized":
        x0 = (x - f * c[0]) / c[1]
        r = c[2] * x0 + c[3] * f
        return r if e is None else r + c[4] * e
    r = c[0] * x
    return r if e is None else r + c[1] * e


def predictor(x, t):
    """The analytic noise predictor of the fixtures: 0.3*x + 0.01*t, t [B]."""
    return 0.3 * x + 0.01 * t.reshape((-1,) + (1,) * (x.dim() - 1))


def same(a, b):
    """torch.equal that lets NaN equal NaN (a 6-step run of the default classical schedule has beta_t > 1: the reference's NaN)."""
    zero = torch.zeros((), dtype=a.dtype)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(torch.where(a.isnan(), zero, a), torch.where(b.isnan(), zero, b))


def load(name):
    from tests.golden_util import load as _load
    return _load("ddpm_" + name)
