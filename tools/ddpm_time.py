"""Time the DDPM / DDIM step kernel (ds_ddpm.hip) and a 50-step DDPMModule run on one MI355X; writes profiles/ddpm.log.

1. The step kernel in place on flat tensors of config 2's state [64,1,128,128] (4 MiB: it lives in the caches) and of
   [64,64,128,128] (256 MiB: larger than the 256 MiB Infinity Cache together with F), per form and noise mode.  Device events
   around a window of launches after a warm-up (as many as fill about 30 ms, at least 20), three rounds, the median round.  The
   achieved HBM rate is the bytes the step has to move -- x read, F read (not in the forward form), eps read in injected mode, x'
   written: 12 bytes per element for a backward step without injected noise -- over the time, against the 8 TB/s of the
   specification.  ds_add (two reads, one write: the same 12 bytes per element, no arithmetic to speak of) is timed on the same
   tensors as the same-box yardstick.
2. A 50-step from_ddpm run (classical schedule, in-kernel noise) over PUNetG(model_channels=64) on [64,1,128,128]: captured
   (use_graph=True, the replay of an existing plan), step by step (use_graph=False), and the eager torch composition of the
   reference's step around the same network (per step: the scheduler on [B,1,1,1] device tensors -- the classical schedule's
   alpha-bar loop reads the step count back on the host --, net(x, t), about ten elementwise passes and a randn_like).  Host
   clock around a whole run that ends in a device synchronise; one warm-up run, then three, the median, per step.

    python tools/ddpm_time.py [--out profiles/ddpm.log] [--steps 50] [--batch 64]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from diffsci_amd import ops  # noqa: E402
from diffsci_amd._native import DDPMCoef  # noqa: E402
import diffsci_amd.models as M  # noqa: E402

PEAK_GBS = 8000.0
dev = torch.device("cuda:0")
LOG = None


def say(line):
    print(line, flush=True)
    LOG.write(line + "\n")
    LOG.flush()


def timed(f):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        f()
    e1.record()
    torch.cuda.synchronize()
    n = int(min(2000, max(20, 30.0 / max(e0.elapsed_time(e1) / 5, 1e-3))))
    rounds = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / n * 1e3)
    return sorted(rounds)[1], n


def report(name, f, nbytes):
    us, n = timed(f)
    gbs = nbytes / us / 1e3
    say(f"{name:46s} {us:9.1f} us  {nbytes / 2**20:8.1f} MiB  {gbs:7.0f} GB/s  {gbs / PEAK_GBS:5.2f} of spec   ({n} launches per round)")


def kernels(shape):
    n = 1
    for s in shape:
        n *= s
    say(f"--- step kernel in place on {list(shape)} ({4 * n / 2**20:.0f} MiB per tensor)")
    x = torch.randn(n, device=dev) * 0.5
    f = torch.randn(n, device=dev)
    state = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    # coefficients that keep the state bounded over thousands of in-place launches: |c1| < 1 (classical), c2/c1 < 1 (generalized)
    coefs = {"classical": DDPMCoef(0.01, 0.9, 0.1, 0.0, 0.0, None), "generalized": DDPMCoef(0.1, 1.0, 0.9, 0.1, 0.1, None),
             "forward": DDPMCoef(0.9, 0.1, 0.0, 0.0, 0.0, None)}
    report("ds_add (yardstick: 12 B per element)", lambda: ops.add(x, f, out=x), 12 * n)
    x.normal_()
    for form in ("classical", "generalized", "forward"):
        ff = None if form == "forward" else f
        base = 8 if form == "forward" else 12
        report(f"{form}, no noise", lambda: ops.ddpm_step(x, ff, coefs[form], form, out=x), base * n)
        report(f"{form}, in-kernel Philox", lambda: ops.ddpm_step(x, ff, coefs[form], form, philox=(state, 0), out=x), base * n)
        eps = torch.randn(n, device=dev)
        report(f"{form}, injected eps", lambda: ops.ddpm_step(x, ff, coefs[form], form, eps=eps, out=x), (base + 4) * n)
        del eps
        assert bool(torch.isfinite(x).all())
        x.normal_()


def reference_composition(net, integ, x, T):
    """The reference's generalized step_backward / propagate_backward in eager torch around `net` (integrators.py:152-210)."""
    sch = integ.scheduler
    for t in (torch.arange(T).to(x) + 1).flip(0):
        tb = t.unsqueeze(0).expand(x.shape[0])
        t_ = tb.reshape((-1,) + (1,) * (x.dim() - 1))
        sigma = integ.noise_injector(t_, T)
        calpha, calpha_prev = sch.calpha(t_, T), sch.calpha(t_ - 1, T)
        f = net(x, tb)
        x0 = (x - f * torch.sqrt(1 - calpha)) / torch.sqrt(calpha)
        x = torch.sqrt(calpha_prev) * x0 + torch.sqrt(torch.relu(1 - calpha_prev - sigma ** 2)) * f + sigma * torch.randn_like(x)
    return x


def wall(f, runs=3):
    f()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return sorted(out)[len(out) // 2], out


def run(steps, batch):
    shape = (batch, 1, 128, 128)
    say(f"--- {steps}-step from_ddpm run (classical schedule, in-kernel noise), PUNetG(model_channels=64) on {list(shape)}")
    torch.manual_seed(0)
    net = M.PUNetG(M.PUNetGConfig(model_channels=64)).to(dev).eval()
    module = M.ddpmv2.DDPMModule(net, M.ddpmv2.DDPMModuleConfig.from_ddpm()).to(dev)
    x = torch.randn(*shape, device=dev)
    t0 = time.perf_counter()
    module.propagate_toward_sample(x, nsteps=steps)
    torch.cuda.synchronize()
    say(f"first call (tables, warm-up, capture, one replay)  {time.perf_counter() - t0:8.2f} s")
    results = []

    def measure(name, f):
        med, all_ = wall(f)
        results.append(med)
        say(f"{name:50s} {1e3 * med / steps:8.3f} ms per step   (runs: {', '.join(f'{1e3 * v:.1f}' for v in all_)} ms)")

    measure("captured (use_graph=True)", lambda: module.propagate_toward_sample(x, nsteps=steps))
    module.use_graph = False
    measure("step by step (use_graph=False)", lambda: module.propagate_toward_sample(x, nsteps=steps))
    eager = torch.inference_mode()(lambda: reference_composition(net, module.config.integrator, x, steps))
    measure("eager torch composition of the reference's step", eager)
    say(f"step by step takes {results[1] / results[0]:.3f}x the captured run's time, the eager composition {results[2] / results[0]:.3f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "ddpm.log"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ddpm_time.py measures on a GPU; none is available")
    global LOG
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as LOG:
        say(f"python tools/ddpm_time.py   ({torch.cuda.get_device_name(0)}; torch {torch.__version__})")
        kernels((64, 1, 128, 128))
        kernels((64, 64, 128, 128))
        run(a.steps, a.batch)


if __name__ == "__main__":
    main()
