"""Time the resampling kernels of the image_sample_factor != 2 route at config-3-like sizes (B = 8, 128-256 channels,
64^2-256^2 fields, 3-D volumes), with the factor-2 kernels beside them, and one ADM-128 evaluation at 256^2 with
transition_scale_factor 2 and 4.  Device events around 20 launches after a warm-up, three rounds; the median round is printed
with the achieved HBM rate (bytes read once + bytes written, against the 8 TB/s peak).  The max-pool rows time PUNetG's
transition_scale_factor != 2 route (ds_maxpool_f), next to eager PUNetG-64 evaluations with factors 2 and 4 in 2-D and 3-D.

    python tools/resample_time.py            # everything
    python tools/resample_time.py maxpool    # the max-pool rows and the PUNetG evaluations only
    python tools/resample_time.py field-eval # the PUNetG-64 64^3 evaluations alone (for a rocprofv3 kernel trace of the split)
    python tools/resample_time.py cornerpool # ds_cornerpool_f next to ds_upsample_f / ds_maxpool_f at the same output sizes, and one
                                             # PUNetG-64 evaluation at 64^3, B = 8 with a field against a vector embedding"""
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops

dev = torch.device("cuda:0")
PEAK_GBS = 8000.0


def timed(f, n=20):
    f()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / n * 1e3)
    return sorted(rounds)[1]


def report(name, f, nbytes):
    us = timed(f)
    gbs = nbytes / us / 1e3
    print(f"{name:58s} {us:9.1f} us  {nbytes / 2**20:8.1f} MiB  {gbs:7.0f} GB/s  {100 * gbs / PEAK_GBS:5.1f}% of peak", flush=True)


torch.manual_seed(0)
ONLY_MAXPOOL = sys.argv[1:] == ["maxpool"]


def maxpool_rows():
    """ds_maxpool_f on shapes above the 256 MiB Infinity Cache, with torch's own kernel beside it."""
    for shape in ((8, 128, 256, 256), (8, 256, 128, 128), (8, 128, 48, 48, 48)):
        x = torch.randn(shape, device=dev)
        tag = "x".join(map(str, shape))
        for f in (2, 3, 4):
            o = torch.empty(shape[:2] + tuple(v // f for v in shape[2:]), device=dev)
            nbytes = 4 * (x.numel() + o.numel())
            report(f"maxpool_f [{tag}] /{f}", lambda: ops.maxpool_f(x, f, out=o), nbytes)
            pool = torch.nn.functional.max_pool3d if x.dim() == 5 else torch.nn.functional.max_pool2d
            report(f"  torch max_pool [{tag}] /{f}", lambda: pool(x, f), nbytes)
        del x, o
    torch.cuda.empty_cache()


def punetg_rows():
    """One eager PUNetG-64 evaluation (channel_expansion [2, 4], as config 2): 2-D at B = 64, 128^2 and 3-D at B = 2, 64^3,
    transition_scale_factor 2 against 4."""
    import diffsci_amd.models as M
    for dim, shape in ((2, (64, 1, 128, 128)), (3, (2, 1, 64, 64, 64))):
        for f in (2, 4):
            torch.manual_seed(0)
            net = M.PUNetG(M.PUNetGConfig(dimension=dim, transition_scale_factor=f)).to(dev).eval()
            x, t = torch.randn(shape, device=dev), torch.rand(shape[0], device=dev)
            with torch.no_grad():
                us = timed(lambda: net(x, t), n=5)
            print(f"PUNetG-64 [2, 4] eval, [{','.join(map(str, shape))}], transition_scale_factor={f}: {us / 1e3:8.2f} ms", flush=True)
            del net
            torch.cuda.empty_cache()


def cornerpool_rows():
    """ds_cornerpool_f (te + ye at a block's resolution, with the amax row) counted as 8 bytes per output element -- 4 read, 4
    written; for f >= 2 the reads use 1/f of every cache line along W -- next to ds_upsample_f and ds_maxpool_f writing the same
    output, each counted by the bytes it reads once plus the bytes it writes."""
    for out_shape in ((8, 64, 64, 64, 64), (8, 128, 32, 32, 32), (8, 128, 256, 256)):
        B, C = out_shape[:2]
        o = torch.empty(out_shape, device=dev)
        te = torch.randn(B, C, device=dev)
        amax = torch.zeros(B, dtype=torch.int32, device=dev)
        tag = "x".join(map(str, out_shape))
        for f in (1, 2, 3, 4):
            x = torch.randn((1, C) + tuple(v * f for v in out_shape[2:]), device=dev)       # the sampler's shared field
            report(f"cornerpool_f -> [{tag}] /{f} (+te, amax, shared x)", lambda: ops.cornerpool_f(x, f, te=te, out=o, out_amax=amax),
                   8 * o.numel())
            del x
            if f > 1 and all(v % f == 0 for v in out_shape[2:]):
                xu = torch.randn(out_shape[:2] + tuple(v // f for v in out_shape[2:]), device=dev)
                report(f"  upsample_f -> [{tag}] x{f}", lambda: ops.upsample_f(xu, f, out=o), 4 * (xu.numel() + o.numel()))
                del xu
            if f > 1 and f * f * (f if len(out_shape) == 5 else 1) * o.numel() * 4 <= 8 << 30:
                xm = torch.randn(out_shape[:2] + tuple(v * f for v in out_shape[2:]), device=dev)
                report(f"  maxpool_f  -> [{tag}] /{f}", lambda: ops.maxpool_f(xm, f, out=o), 4 * (xm.numel() + o.numel()))
                del xm
        del o
    torch.cuda.empty_cache()


def punetg_field_rows():
    """One eager PUNetG-64 evaluation (channel_expansion [2, 4]) at 64^3, B = 8: no condition, a vector embedding, a field
    embedding (the per-voxel time MLPs, and the standalone norms in place of resblock3d_fused)."""
    import diffsci_amd.models as M
    torch.manual_seed(0)
    net = M.PUNetG(M.PUNetGConfig(dimension=3), conditional_embedding=torch.nn.Identity()).to(dev).eval()
    x, t = torch.randn(8, 1, 64, 64, 64, device=dev), torch.rand(8, device=dev)
    conds = (("unconditional", None), ("vector embedding", torch.randn(8, 64, device=dev)),
             ("field embedding 64^3", torch.randn(1, 64, 64, 64, 64, device=dev)))
    for name, y in conds:
        with torch.no_grad():
            us = timed(lambda: net(x, t, y), n=5)
        print(f"PUNetG-64 [2, 4] eval, [8,1,64,64,64], {name}: {us / 1e3:8.2f} ms", flush=True)


if sys.argv[1:] == ["cornerpool"]:
    cornerpool_rows()
    punetg_field_rows()
    sys.exit(0)
if sys.argv[1:] == ["field-eval"]:
    punetg_field_rows()
    sys.exit(0)
if ONLY_MAXPOOL:
    maxpool_rows()
    punetg_rows()
    sys.exit(0)
# fields: upsampling (store-bound) and norm + SiLU + pooling (read-bound)
for B, C, H in ((8, 128, 64), (8, 256, 64), (8, 128, 32)):
    for f in (2, 3, 4):
        x = torch.randn(B, C, H, H, device=dev)
        out = torch.empty(B, C, f * H, f * H, device=dev)
        report(f"upsample_f   [{B},{C},{H},{H}] x{f}", lambda: ops.upsample_f(x, f, out=out), 4 * (x.numel() + out.numel()))
for B, C, H in ((8, 128, 256), (8, 256, 128)):
    x = torch.randn(B, C, H, H, device=dev)
    st = ops.gnorm1_stats(x, 0)
    w, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
    o2 = torch.empty(B, C, H // 2, H // 2, device=dev)
    report(f"gnorm1_apply pool=2 (f=2 route) [{B},{C},{H},{H}]",
           lambda: ops.gnorm1_apply(x, st, w, b, 0, pool=True, out=o2), 4 * (x.numel() + o2.numel()))
    for f in (2, 3, 4):
        o = torch.empty(B, C, H // f, H // f, device=dev)
        report(f"gnorm1_apply_poolf kind 0 [{B},{C},{H},{H}] /{f}",
               lambda: ops.gnorm1_apply_poolf(x, st, w, b, 0, f, out=o), 4 * (x.numel() + o.numel()))
        report(f"gnorm1_apply_poolf kind 2 [{B},{C},{H},{H}] /{f}",
               lambda: ops.gnorm1_apply_poolf(x, None, None, None, 2, f, out=o), 4 * (x.numel() + o.numel()))
    del x, o, o2
# volumes
for B, C, D in ((8, 128, 48),):
    x = torch.randn(B, C, D, D, D, device=dev)
    report(f"avgpool3d (f=2 route) [{B},{C},{D}^3]", lambda: ops.avgpool3d(x), 4 * x.numel() * 9 // 8)
    for f in (2, 3, 4):
        o = torch.empty(B, C, D // f, D // f, D // f, device=dev)
        report(f"avgpool_f 3-D [{B},{C},{D}^3] /{f}", lambda: ops.avgpool_f(x, f, out=o), 4 * (x.numel() + o.numel()))
    del x, o
for B, C, D in ((8, 128, 16),):
    x = torch.randn(B, C, D, D, D, device=dev)
    report(f"upsample3d (f=2 route) [{B},{C},{D}^3]", lambda: ops.upsample3d(x), 4 * x.numel() * 9)
    for f in (2, 3, 4):
        o = torch.empty(B, C, f * D, f * D, f * D, device=dev)
        report(f"upsample_f 3-D [{B},{C},{D}^3] x{f}", lambda: ops.upsample_f(x, f, out=o), 4 * (x.numel() + o.numel()))
    del x, o
torch.cuda.empty_cache()

# one ADM-128 evaluation ([1, 2, 4] channel expansion, two transitions) at 256^2, B = 8: factor 2 against factor 4
import diffsci_amd.models as M
for f in (2, 4):
    torch.manual_seed(0)
    net = M.ADM(M.ADMConfig(input_channels=3, output_channels=3, model_channels=128, time_embed_dim=128, output_embed_dim=512,
                            channel_expansion=[2, 4], transition_scale_factor=f)).to(dev)
    x, t = torch.randn(8, 3, 256, 256, device=dev), torch.rand(8, device=dev)
    with torch.no_grad():
        us = timed(lambda: net(x, t), n=5)
    print(f"ADM-128 [2, 4] eval, [8,3,256,256], transition_scale_factor={f}: {us / 1e3:8.2f} ms", flush=True)
    del net
    torch.cuda.empty_cache()
maxpool_rows()
punetg_rows()
cornerpool_rows()
punetg_field_rows()
