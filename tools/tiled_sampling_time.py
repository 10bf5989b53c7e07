"""Time the tiled volume sampling on the GPU (a report, not a test): extra.sample_grid_volume and extra.sample_sequential_z on
the fused, captured Euler-Maruyama run (SIModule.sample_fused / inpaint_fused, ds_inpaint.hip) against the same generators
driving the step-by-step SIModule.sample / inpaint, which they use for any module without the fused methods.

    network      3-D PUNetG, model_channels 64, 4 channels in and out
    grid         base [4, 32, 32, 32], overlap 16, grid (2, 2, 2), 30 steps; every axis periodic unless --open (then the cubes
                 have sides 40 and 48: eight shapes, eight plans)
    sequential   3 blocks of the same base, overlap 16, 30 steps, noise_injection (its default)

Wall time around a call and a device synchronisation, in alternating rounds; the step-by-step variant is listed twice, and the
spread between its two listings is the noise floor of the comparison.  `host` is the time the call itself took before the
synchronisation, per cube (a run ends in the range guard's host read, so this is close to the whole time).  Then the step
kernel alone: ds_si_inpaint_step (blend, in-kernel Philox) next to ds_karras_euler (Euler-Maruyama, in-kernel Philox: the fused Karras step) at one cube's state and at a state large
enough to be bound by memory; bytes = 16 per element (x and F read, x and the network input written).

    python tools/tiled_sampling_time.py [--rounds 3] [--nsteps 30] [--open]"""
import argparse
import os
import sys
import time
import warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import diffsci_amd.models as M
from diffsci_amd import extra, ops
from diffsci_amd._native import DS_IN_FLOW
from diffsci_amd.models.karras import siloop

dev = torch.device("cuda:0")


class StepByStep:
    """The module as the generators see one without the fused methods."""

    def __init__(self, module):
        self.device, self.sample, self.inpaint = module.device, module.sample, module.inpaint


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert bool(torch.isfinite(out).all())
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3


def rounds(variants, n, cubes):
    got = {k: [] for k in variants}
    for k, f in variants.items():
        f()                                                               # the first call: captures, workspaces, packed weights
    for _ in range(n):
        for k, f in variants.items():
            got[k].append(wall(f))
    for k, r in got.items():
        total = sorted(t for t, _ in r)
        host = sorted(h for _, h in r)
        mid = total[len(total) // 2]
        print(f"  {k:34s} {mid:9.1f} ms   host {host[len(host) // 2] / cubes:7.2f} ms per cube   "
              f"(rounds: {', '.join(f'{t:.1f}' for t, _ in r)})", flush=True)
    return {k: sorted(t for t, _ in r)[len(r) // 2] for k, r in got.items()}


def generators(args):
    torch.manual_seed(0)
    net = M.PUNetG(M.PUNetGConfig(input_channels=4, output_channels=4, dimension=3, model_channels=64)).to(dev).eval()
    module = M.SIModule(M.SIModuleConfig(scheduler="linear"), net).to(dev).eval()
    eager = StepByStep(module)
    base, overlap = [4, 32, 32, 32], 16
    per = [not args.open] * 3
    grid = dict(grid_map=[2, 2, 2], base_shape=base, overlap_size=overlap, nsteps=args.nsteps, periodicity=per)
    seq = dict(num_blocks=3, base_shape=base, overlap_size=overlap, nsteps=args.nsteps)
    for title, fn, kw, cubes in ((f"sample_grid_volume grid (2,2,2) periodicity {per}", extra.sample_grid_volume, grid, 8),
                                 ("sample_sequential_z 3 blocks", extra.sample_sequential_z, seq, 3)):
        print(f"--- {title}, base {base}, overlap {overlap}, {args.nsteps} steps", flush=True)
        mid = rounds({"fused, captured": lambda: fn(module, **kw), "step by step (a)": lambda: fn(eager, **kw),
                      "step by step (b)": lambda: fn(eager, **kw)}, args.rounds, cubes)
        a, b, f = mid["step by step (a)"], mid["step by step (b)"], mid["fused, captured"]
        print(f"  step by step / fused = {min(a, b) / f:.3f}; noise floor (the two step-by-step listings) {abs(a - b) / min(a, b):.3%}",
              flush=True)


def kernels(iters):
    cfg = M.SIModuleConfig(scheduler="linear")
    row = siloop.si_row(cfg, torch.tensor(0.6), torch.tensor(0.4), False, blend=True)
    k = row.first.coef(DS_IN_FLOW, 1.0)
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    for shape in ((1, 4, 48, 48, 48), (16, 4, 64, 64, 64)):
        x, f = torch.randn(*shape, device=dev), torch.randn(*shape, device=dev)
        xin = torch.empty_like(x)
        x_orig, mask = torch.randn(*shape[1:], device=dev), torch.rand(*shape[1:], device=dev)
        variants = {
            "ds_si_inpaint_step (blend, Philox)": lambda: ops.si_inpaint_step(x, f, k, row.step(1.0), x_orig=x_orig, mask=mask,
                                                                               blend=True, philox=(rng, 0), x_out=x, xin_out=xin),
            "ds_karras_euler (EM, Philox)": lambda: ops.euler(x, f, k, row.dt, x_out=x, xin_out=xin, philox=(rng, 0),
                                                              noise_coef=1e-3, sqrt_abs_dt=0.4),
        }
        print(f"--- the step kernel alone, state {list(shape)} ({x.numel() * 4 / 2 ** 20:.1f} MiB)", flush=True)
        res = {kk: [] for kk in variants}
        for _ in range(3):
            for kk, fn in variants.items():
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                    x.copy_(f)                                            # keep the state bounded (charged to both variants)
                e1.record()
                torch.cuda.synchronize()
                res[kk].append(e0.elapsed_time(e1) / iters)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            x.copy_(f)
        e1.record()
        torch.cuda.synchronize()
        copy = e0.elapsed_time(e1) / iters
        for kk, r in res.items():
            mid = sorted(r)[1] - copy
            print(f"  {kk:40s} {mid * 1e3:9.1f} us  {16 * x.numel() / mid / 1e6:8.1f} GB/s   (rounds, with the {copy * 1e3:.1f} us copy: "
                  f"{', '.join(f'{v * 1e3:.1f}' for v in r)})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nsteps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--open", action="store_true", help="no periodic axis (cubes of sides 40 and 48)")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    with torch.inference_mode(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kernels(args.iters)
        generators(args)


if __name__ == "__main__":
    main()
