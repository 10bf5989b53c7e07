"""Time DiffusionPeriodizer's fused crop-and-blend (ds_periodize.hip) and a 50-step KarrasModule run through the periodizer on one
MI355X; writes profiles/periodizer.log.

1. ops.crop_blend on [16,1,256,256] cropped from pad 32 and on [1,4,64,64,64] cropped from pad 16 (blend width 8), against
   (a) ops.box_copy3d of the same crop -- the floor: the same bytes, no arithmetic -- and
   (b) the reference's composition in eager torch on the device: the centre slice, clone, and per axis two flipped strips blended
       and assigned (periodizer.py:103-199).
   Device events around a window of launches after a warm-up (as many as fill about 100 ms, at least 20), five rounds, the
   median round with the fastest and the slowest beside it; the three alternate inside every round.  The tensors are 4 MiB out
   and 6 - 13 MiB in and every launch of a window works on the same ones, so they are warm in the 256 MiB Infinity Cache: the
   times are launch times of cache-resident data and the rate printed is bytes over time, NOT an HBM rate.  The outputs are
   compared bit for bit first.  The kernel must not be slower than
   (b) -- it moves strictly fewer bytes in one launch -- and the tool fails if it is; its ratio to (a) is recorded, no threshold.
2. A 50-step captured KarrasModule run (Heun) over PUNetG(model_channels=64) on [64,1,128,128] through
   DiffusionPeriodizer(pad=32, blend_width=8), against the same run evaluated as given step by step (the planned protocol hidden,
   use_graph=False) and against the bare network at 192x192, captured -- what the expansion itself costs.  Host clock around a
   whole run that ends in a device synchronise; one warm-up run, then three, the median.

    python tools/periodizer_time.py [--out profiles/periodizer.log] [--steps 50] [--batch 64]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from diffsci_amd import ops  # noqa: E402
from diffsci_amd.extra import DiffusionPeriodizer  # noqa: E402
import diffsci_amd.models as M  # noqa: E402

dev = torch.device("cuda:0")
LOG = None


def say(line):
    print(line, flush=True)
    LOG.write(line + "\n")
    LOG.flush()


def eager_composition(y, pad, widths, tables):
    """crop_center then cosine_blend_boundaries as the reference issues them (periodizer.py:103-199), weights given."""
    x = y[(slice(None), slice(None)) + tuple(slice(p, y.shape[a + 2] - p) for a, p in enumerate(pad))].clone()
    for a, bw in enumerate(widths):
        dim, size = a + 2, x.shape[a + 2]
        if bw <= 0 or 2 * bw >= size:
            continue
        shape = [1] * x.dim()
        shape[dim] = bw
        w = tables[a].reshape(shape)
        start, end = x.narrow(dim, 0, bw), x.narrow(dim, size - bw, bw)
        new_start = w * start + (1 - w) * end.flip(dims=[dim])
        new_end = w.flip(dims=[dim]) * end + (1 - w.flip(dims=[dim])) * start.flip(dims=[dim])
        start.copy_(new_start)
        end.copy_(new_end)
    return x


ROUNDS, WINDOW_MS = 5, 100.0


def window(fs):
    """Per function of fs the (median, fastest, slowest) round's time per call in microseconds, alternating inside every round."""
    for f in fs:
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fs[0]()
    e1.record()
    torch.cuda.synchronize()
    n = int(min(10000, max(20, WINDOW_MS / max(e0.elapsed_time(e1) / 5, 1e-3))))
    rounds = [[] for _ in fs]
    for _ in range(ROUNDS):
        for k, f in enumerate(fs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                f()
            e1.record()
            torch.cuda.synchronize()
            rounds[k].append(e0.elapsed_time(e1) / n * 1e3)
    return [(sorted(r)[len(r) // 2], min(r), max(r)) for r in rounds], n


def kernel(shape, pad, bw):
    nd = len(shape) - 2
    pad, widths = (pad,) * nd, (bw,) * nd
    big = tuple(shape[:2]) + tuple(s + 2 * p for s, p in zip(shape[2:], pad))
    y = torch.randn(big, device=dev)
    out = torch.empty(shape, device=dev)
    tables = ops.blend_weights(widths, dev)
    lead = 3 - nd
    start, size = (0,) * lead + pad, (1,) * lead + tuple(shape[2:])
    y3, out3 = y.view(-1, *((1,) * lead + big[2:])), out.view(-1, *size)
    fused = lambda: ops.crop_blend(y, pad, widths, out=out, weights=tables)              # noqa: E731
    copy = lambda: ops.box_copy3d(y3, start, out3, (0, 0, 0), size)                      # noqa: E731
    eager = lambda: eager_composition(y, pad, widths, tables)                            # noqa: E731
    same = torch.equal(fused(), eager())
    (fused_t, copy_t, eager_t), n = window([fused, copy, eager])
    t_fused, t_copy, t_eager = fused_t[0], copy_t[0], eager_t[0]
    nbytes = 8 * out.numel()
    spread = lambda t: f"{t[0]:9.1f} us  (rounds {t[1]:.1f} - {t[2]:.1f})"                 # noqa: E731
    say(f"--- crop_blend {list(shape)} from pad {pad[0]}, blend width {bw} ({4 * out.numel() / 2**20:.0f} MiB out, {4 * y.numel() / 2**20:.1f} MiB in, "
        f"warm in the Infinity Cache; {ROUNDS} rounds of {n} launches); bit-identical to the eager composition: {same}")
    say(f"ops.crop_blend (one launch)                     {spread(fused_t)}  {nbytes / t_fused / 1e3:7.0f} GB/s of the crop's read + write (cache-resident)")
    say(f"(a) ops.box_copy3d of the same crop             {spread(copy_t)}  {nbytes / t_copy / 1e3:7.0f} GB/s (cache-resident)")
    say(f"(b) eager torch: slice, clone, strip updates    {spread(eager_t)}")
    say(f"crop_blend / (a) = {t_fused / t_copy:.3f} (between {fused_t[1] / copy_t[2]:.3f} and {fused_t[2] / copy_t[1]:.3f} over the rounds);  "
        f"(b) / crop_blend = {t_eager / t_fused:.2f} (at least {eager_t[1] / fused_t[2]:.2f})")
    return same and fused_t[2] <= eager_t[1]


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


def run(steps, batch, side=128, pad=32, bw=8):
    say(f"--- {steps}-step KarrasModule run (from_edm, Heun), PUNetG(model_channels=64) on {[batch, 1, side, side]}, pad {pad}, blend width {bw}")
    torch.manual_seed(0)
    net = M.PUNetG(M.PUNetGConfig(model_channels=64)).to(dev).eval()
    per = DiffusionPeriodizer(net, pad, bw, dimension=2)
    module = M.KarrasModule(per, M.KarrasModuleConfig.from_edm()).to(dev).eval()
    bare = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).to(dev).eval()
    x = torch.randn(batch, 1, side, side, device=dev)
    xb = torch.randn(batch, 1, side + 2 * pad, side + 2 * pad, device=dev)
    results = []

    def measure(name, f):
        med, all_ = wall(f)
        results.append(med)
        say(f"{name:62s} {1e3 * med / steps:8.3f} ms per step   (runs: {', '.join(f'{1e3 * v:.1f}' for v in all_)} ms)")

    go = lambda m, v: m.propagate_white_noise(v, nsteps=steps, integrator="heun")        # noqa: E731
    measure("periodizer, planned and captured (use_graph=True)", lambda: go(module, x))
    assert len(module._plans.plans) == 1
    measure(f"bare network at {side + 2 * pad}x{side + 2 * pad}, captured", lambda: go(bare, xb))
    module.use_graph = False
    per.__dict__["forward_with_shifts"] = None                     # the planned protocol hidden: evaluated as given
    measure("periodizer evaluated as given, step by step", lambda: go(module, x))
    say(f"the periodizer costs {results[0] / results[1]:.3f}x the bare network at the expanded size; evaluated as given step by step takes "
        f"{results[2] / results[0]:.3f}x the captured run's time")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "periodizer.log"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("periodizer_time.py measures on a GPU; none is available")
    global LOG
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as LOG:
        say(f"python tools/periodizer_time.py   ({torch.cuda.get_device_name(0)}; torch {torch.__version__})")
        ok = kernel((16, 1, 256, 256), 32, 8)
        ok = kernel((1, 4, 64, 64, 64), 16, 8) and ok
        run(a.steps, a.batch)
        say("crop_blend is bit-identical to and no slower than the eager composition: " + ("yes" if ok else "NO"))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
