"""The volume path (ops.conv3d_mfma, ops.resblock3d_fused) at 64-256 channels against fp64, on every kernel route it takes there.

The volume path drives the 2-D fp16x3 kernels in ways no 2-D test does: side depth taps accumulate IN PLACE (res1 = out = acc), every
slice is a 2-D sample with its own activation exponent or its own norm-table row, pad slices carry all-zero table rows with a zero
fourth column (no activation exponent), outputs at the pad slices between two samples are garbage that is read back through those
zero rows, and the statistics come from the last tap alone.  At 8-32 channels all of that runs on one kernel configuration; the cases
here put it on the multi-chunk 16x16x32 kernels, the 16-byte patch loads, the persistent producer / consumer kernel (k_conv3p, plain
and periodic), the two-channel-tile kernel (round-3 arm) and the parity kernel k_convup at width.

Every case is computed three times: on the GPU, by torch in fp64 on the CPU (the reference) and by the same torch composition in
fp32 on the CPU (the yardstick: what plain fp32 arithmetic loses on this input).  A case is ok when
    rel_l2(got, fp64) <= max(3 * rel_l2(torch_fp32, fp64), floor)   and   max|got - fp64| <= max(4 * max|torch_fp32 - fp64|, 1e-5)
with floor = 5e-7 for conv3d_mfma and 3e-6 for the fused block (the bounds the 8-channel tests of the same operations assert).
c64_slices gives every depth slice its own magnitude (2^-30 ... 2^27) and is held to both bounds on EVERY output slice (b, z): a
global norm would only see the largest slices.  Its residuals follow the slice ramp and it has no bias / shift: a per-channel constant
of order one would be the whole output of the small slices and make their bound vacuous.
The fused cases (run with norm2 = GroupNorm(C, C) and GroupRMSNorm, kind2 = 0 and 1) also check that out_stats recombines to the fp64
sums of the returned output (rtol 1e-6, atol 1e-4; n == D*H*W exactly) and that ops.inorm_table on them gives the output's fp64 mean
and weight / sqrt(var + eps) to rtol 1e-5.

The library reads its DS_CONV_* switches once per process.  Unless --no-ab is given the cases also run in a child process on the
round-3 routes (DS_CONV_PC=0 DS_CONV_VEC=0 DS_CONV_TWO_EARLY=0: one-shot kernels, one-pixel staging -- the same summation order,
DESIGN 4.5), and outputs and statistics of the two arms must agree BIT FOR BIT; the first differing indices are printed otherwise.

    python tools/volume_check.py                         # every case, default routes against the round-3 routes and fp64
    python tools/volume_check.py --only f64,f128 --no-ab # a subset, default routes only (what the kernel-trace test runs)
    python tools/volume_check.py --child FILE            # (internal) run the cases, save outputs and statistics
"""
import argparse
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN, MAXPOOL2, UPSAMPLE2 = 0, 1, 2
CHILD_SWITCHES = dict(DS_CONV_PC="0", DS_CONV_VEC="0", DS_CONV_TWO_EARLY="0")
CONV_FLOOR, FUSED_FLOOR = 5e-7, 3e-6

# ops.conv3d_mfma: name, B, Cin, Cout, (D, H, W) of the OUTPUT, kernel size, load mode, circular, what it is there for
CONV_CASES = [
    ("c64_128", 2, 64, 128, (8, 16, 32), 3, PLAIN, False, "4 chunks, two channel tiles, 16-byte loads, in-place taps"),
    ("c128_256_pool", 1, 128, 256, (4, 16, 32), 3, MAXPOOL2, False, "pooling loader at 8 chunks, depth pairs in the slice copy"),
    ("c256_128_up", 1, 256, 128, (8, 16, 64), 3, UPSAMPLE2, False, "parity kernel k_convup at 16 chunks (8 x 32 input planes)"),
    ("c256_128_up16", 1, 256, 128, (8, 16, 32), 3, UPSAMPLE2, False, "8 x 16 input planes: the upsampling loader of k_conv3h instead"),
    ("c192_64_circ", 1, 192, 64, (5, 12, 20), 3, PLAIN, True, "12 chunks, ragged tiles, periodic wrap in plane and depth"),
    ("c72_136", 2, 72, 136, (4, 16, 32), 3, PLAIN, False, "a half-filled last chunk (odd chunk count) and a ragged channel tile"),
    ("c64_k5", 1, 64, 64, (6, 16, 32), 5, PLAIN, False, "five depth taps x four shifted blocks, all accumulated in place"),
    ("c64_slices", 2, 64, 64, (20, 16, 32), 3, PLAIN, False, "one activation exponent per slice; bounds per output slice"),
]

# ops.resblock3d_fused: name, B, C, (D, H, W), circular, what it is there for
FUSED_CASES = [
    ("f64", 2, 64, (16, 32, 64), False, "272 items: conv2 on k_conv3p<PRE>, zero rows, fourth column 0; conv1 on the one-shot VEC kernel"),
    ("f128", 2, 128, (16, 32, 64), False, "544 items, two channel tiles (round-3 arm: two tiles per workgroup)"),
    ("f64_circ", 3, 64, (10, 24, 96), True, "306 items (uneven per workgroup), periodic k_conv3p, wrapped pad slices"),
    ("f128_small", 1, 128, (6, 16, 32), False, "below the persistent minimum: one-shot fused loader, VEC, two channel tiles"),
    ("f64_ragged", 2, 64, (5, 20, 40), False, "wide channels on ragged planes: one-pixel staging"),
]
NAMES = [c[0] for c in CONV_CASES] + [c[0] for c in FUSED_CASES]


def _seed(name):
    return 1000 + NAMES.index(name)


def _in_shape(dhw, mode):
    D, H, W = dhw
    return {PLAIN: (D, H, W), MAXPOOL2: (2 * D, 2 * H, 2 * W), UPSAMPLE2: (D // 2, H // 2, W // 2)}[mode]


def conv_inputs(case):
    import torch
    name, B, Cin, Cout, dhw, k, mode, circ, _ = case
    g = torch.Generator().manual_seed(_seed(name))
    x = torch.randn(B, Cin, *_in_shape(dhw, mode), generator=g) * 1.5 + 0.3
    w = torch.randn(Cout, Cin, k, k, k, generator=g) / math.sqrt(Cin * 27)
    bias, shift = torch.randn(Cout, generator=g), torch.randn(B, Cout, generator=g)
    r1, r2 = torch.randn(B, Cout, *dhw, generator=g), torch.randn(B, Cout, *dhw, generator=g) * 0.7 + 0.1
    if name == "c64_slices":
        D = dhw[0]
        ramp = 2.0 ** (3.0 * torch.arange(D, dtype=torch.float64) - 30.0)
        scale = torch.stack([ramp, ramp.flip(0) * 2.0 ** -7]).float()[:, None, :, None, None]        # [B, 1, D, 1, 1]: powers of two
        x, r1, r2, bias, shift = x * scale, r1 * scale, r2 * scale, None, None
    return dict(x=x, w=w, bias=bias, shift=shift, r1=r1, r2=r2)


def conv_reference(case, t, dtype):
    import torch.nn.functional as F
    name, B, Cin, Cout, dhw, k, mode, circ, _ = case
    c = lambda v: None if v is None else v.to(dtype)      # noqa: E731
    src = c(t["x"])
    if mode == MAXPOOL2:
        src = F.max_pool3d(src, 2)
    elif mode == UPSAMPLE2:
        src = F.interpolate(src, scale_factor=2.0, mode="nearest")
    p = k // 2
    if circ:
        want = F.conv3d(F.pad(src, (p,) * 6, mode="circular"), c(t["w"]), c(t["bias"]))
    else:
        want = F.conv3d(src, c(t["w"]), c(t["bias"]), padding=p)
    if t["shift"] is not None:
        want = want + c(t["shift"])[:, :, None, None, None]
    return want + c(t["r1"]) + c(t["r2"])


def conv_gpu(case, t, dev):
    import torch
    from diffsci_amd import ops
    name, B, Cin, Cout, dhw, k, mode, circ, _ = case
    d = lambda v: None if v is None else v.to(dev)        # noqa: E731
    D, H, W = dhw
    st = torch.full((B, Cout, ops.volume_stat_tiles(D, H * W), 4), float("nan"), device=dev)
    packs = ops.pack_conv3d(t["w"].to(dev), upsampled=mode == UPSAMPLE2)
    if mode == UPSAMPLE2:
        Din, Hin, Win = _in_shape(dhw, mode)
        on_parity_kernel = bool(ops.N.lib().ds_conv2d_h3_up_supported(Hin, Win))
        assert on_parity_kernel == (name == "c256_128_up"), (name, Hin, Win)
    out = ops.conv3d_mfma(t["x"].to(dev), packs, bias=d(t["bias"]), shift=d(t["shift"]), res1=d(t["r1"]), res2=d(t["r2"]),
                          load_mode=mode, circular=circ, out_stats=st)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), stats=st.cpu())


def fused_inputs(case):
    import torch
    name, B, C, dhw, circ, _ = case
    g = torch.Generator().manual_seed(_seed(name))
    r = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
    t = dict(h=r(B, C, *dhw) * 1.5 + 0.3, w1=1.0 + 0.3 * r(C), b1=0.4 * r(C), w2=1.0 + 0.3 * r(C), b2=0.4 * r(C),
             wa=r(C, C, 3, 3, 3) / math.sqrt(C * 27), ba=0.3 * r(C), wb=r(C, C, 3, 3, 3) / math.sqrt(C * 27), bb=0.3 * r(C),
             shift=r(B, C), res2=r(B, C, *dhw) * 0.8 - 0.1, wn=1.0 + 0.3 * r(C), bn=0.4 * r(C))
    return t


def fused_reference(case, t, kind2, dtype):
    import torch.nn.functional as F
    from oracle.punetg_ref import group_rms_norm
    name, B, C, dhw, circ, _ = case
    c = lambda v: v.to(dtype)                             # noqa: E731

    def conv(a, w, b):
        if circ:
            return F.conv3d(F.pad(a, (1,) * 6, mode="circular"), c(w), c(b))
        return F.conv3d(a, c(w), c(b), padding=1)
    h = c(t["h"])
    a = F.silu(F.group_norm(h, C, c(t["w1"]), c(t["b1"]), 1e-5))
    y = conv(a, t["wa"], t["ba"]) + c(t["shift"])[:, :, None, None, None]
    n2 = F.group_norm(y, C, c(t["w2"]), c(t["b2"]), 1e-5) if kind2 == 0 else group_rms_norm(y, c(t["w2"]), c(t["b2"]), 1e-5)
    return conv(F.silu(n2), t["wb"], t["bb"]) + h + c(t["res2"])


def fused_gpu(case, t, dev):
    """-> per kind2: out, out_stats, and the table ops.inorm_table builds from out_stats."""
    import torch
    from diffsci_amd import ops
    name, B, C, dhw, circ, _ = case
    D, H, W = dhw
    h = t["h"].to(dev)
    # the statistics of the input as a producer's slice -> volume copy leaves them, and norm1's table from those
    s = torch.empty(B * (D + 2), C, H, W, device=dev)
    ops.N.check(ops.N.lib().ds_volume_to_slices(ops._p(s), ops._p(h), B, C, D, H * W, 0, 0, 1, ops._stream()), "ds_volume_to_slices")
    back = torch.empty_like(h)
    hs = torch.full((B, C, ops.volume_stat_tiles(D, H * W), 4), float("nan"), device=dev)
    ops._from_slices(back, s, None, None, B, C, D, H * W, hs)
    assert torch.equal(back, h)
    tab1 = ops.inorm_table(hs, t["w1"].to(dev), t["b1"].to(dev), 0, D * H * W)
    p1, p2 = ops.pack_conv3d(t["wa"].to(dev)), ops.pack_conv3d(t["wb"].to(dev))
    res = {}
    for kind2 in (0, 1):
        st = torch.full((B, C, ops.volume_stat_tiles(D, H * W), 4), float("nan"), device=dev)
        out = ops.resblock3d_fused(h, tab1, p1, t["ba"].to(dev), t["shift"].to(dev), p2, t["bb"].to(dev), t["w2"].to(dev),
                                   t["b2"].to(dev), kind2, res2=t["res2"].to(dev), out_stats=st, circular=circ)
        tab = ops.inorm_table(st, t["wn"].to(dev), t["bn"].to(dev), 0, D * H * W)
        torch.cuda.synchronize()
        res[f"out{kind2}"], res[f"stats{kind2}"], res[f"tab{kind2}"] = out.cpu(), st.cpu(), tab.cpu()
    assert torch.equal(h.cpu(), t["h"]), "resblock3d_fused changed its input"
    return res


def run_gpu(names, dev):
    res = {}
    for case in CONV_CASES:
        if case[0] in names:
            res[case[0]] = conv_gpu(case, conv_inputs(case), dev)
    for case in FUSED_CASES:
        if case[0] in names:
            res[case[0]] = fused_gpu(case, fused_inputs(case), dev)
    return res


def errors(got, f32, f64, per_slice):
    """-> rel-L2 and max-abs of got and of torch fp32 against fp64, and whether the two output bounds hold up to `floor` (a closure
    over the floor would hide it: returned as a function).  per_slice: every (b, z) of [B, C, D, H, W] is held to the bounds; the
    figures reported are those of the slice with the largest rel-L2 of got."""
    import torch
    g, a, w = got.double(), f32.double(), f64
    dims = (1, 3, 4) if per_slice else tuple(range(got.dim()))
    den = w.pow(2).sum(dims).sqrt().clamp_min(1e-300)
    rel_g, rel_a = (g - w).pow(2).sum(dims).sqrt() / den, (a - w).pow(2).sum(dims).sqrt() / den
    max_g, max_a = (g - w).abs().amax(dims), (a - w).abs().amax(dims)

    def holds(floor):
        return bool(torch.isfinite(g).all() and (rel_g <= torch.clamp_min(3 * rel_a, floor)).all()
                    and (max_g <= torch.clamp_min(4 * max_a, 1e-5)).all())
    i = int(rel_g.flatten().argmax())
    pick = lambda v: float(v.flatten()[i])                # noqa: E731
    extra = ""
    if per_slice:
        ratio = rel_g / torch.clamp_min(3 * rel_a, 1e-300)
        extra = (f"  [per slice: rel-L2 {float(rel_g.min()):.2e}..{float(rel_g.max()):.2e}, torch fp32 {float(rel_a.min()):.2e}.."
                 f"{float(rel_a.max()):.2e}, worst got / (3 x fp32) {float(ratio.max()):.2f} at (b, z) = "
                 f"{tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])}]")
    return pick(rel_g), pick(rel_a), pick(max_g), pick(max_a), holds, extra


def stats_ok(st, tab, out, wn, count):
    """out_stats (K, S, Q, n per tile) against the fp64 sums of the returned output, and the table built from them -> the checks
    that failed, and per check the largest |error| / allowed."""
    import torch
    K, S, Q, n = st.double().unbind(-1)
    o = out.double()
    sx, sxx, nn = (n * K + S).sum(-1), (Q + 2 * K * S + n * K * K).sum(-1), n.sum(-1)
    C = out.shape[1]
    mean, var = o.mean(dim=(2, 3, 4)), o.var(dim=(2, 3, 4), unbiased=False)
    failed = [] if bool(torch.isfinite(st).all()) and torch.equal(nn, torch.full_like(nn, count)) else ["n != D*H*W"]
    used = {}
    for what, a, b, rtol, atol in (("sum", sx, o.sum(dim=(2, 3, 4)), 1e-6, 1e-4), ("sumsq", sxx, (o * o).sum(dim=(2, 3, 4)), 1e-6, 1e-4),
                                   ("mean", tab[:, :C, 0].double(), mean, 1e-5, 1e-6),
                                   ("rstd", tab[:, :C, 1].double(), wn.double() / torch.sqrt(var + 1e-5), 1e-5, 1e-8)):
        err, allowed = (a - b).abs(), atol + rtol * b.abs()
        used[what] = float((err / allowed).max())
        if not bool((err <= allowed).all()):
            i = int((err / allowed).flatten().argmax())
            failed.append(f"{what}: {int((err > allowed).sum())} of {err.numel()} (b, c) outside atol {atol:g} + rtol {rtol:g}; worst |err| "
                          f"{float(err.flatten()[i]):.3e} against {float(allowed.flatten()[i]):.3e} allowed at a value of "
                          f"{float(b.flatten()[i]):.4e} (max |err| {float(err.max()):.3e}, n = {count})")
    return failed, used


def first_mismatch(a, b):
    d = a != b
    return (f"first mismatches {d.nonzero()[:5].tolist()}, {int(d.sum())} of {d.numel()}, max abs diff "
            f"{float((a.double() - b.double()).abs().max()):.3e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="comma-separated case names")
    ap.add_argument("--no-ab", action="store_true", help="default routes only: no child process on the round-3 routes")
    ap.add_argument("--child", default="", metavar="FILE", help="(internal) run the cases and save outputs and statistics")
    a = ap.parse_args()
    names = [n for n in a.only.split(",") if n] or NAMES
    unknown = [n for n in names if n not in NAMES]
    if unknown:
        sys.exit(f"volume_check: unknown case(s) {unknown}; choose from {NAMES}")
    import torch
    dev = torch.device("cuda:0")
    if a.child:
        torch.save(run_gpu(names, dev), a.child)
        return
    ref = None
    if not a.no_ab:
        env = {k: v for k, v in os.environ.items() if not k.startswith("DS_CONV_")}
        env.update(CHILD_SWITCHES)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "arm.pt")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--only", ",".join(names), "--child", path], env=env)
            ref = torch.load(path)
    got = run_gpu(names, dev)
    bad = 0
    for case in CONV_CASES + FUSED_CASES:
        name = case[0]
        if name not in names:
            continue
        fused = len(case) == 6
        notes, ok, stat_use = [], True, {}
        if fused:
            t, floor, keys = fused_inputs(case), FUSED_FLOOR, [("out0", "stats0", 0), ("out1", "stats1", 1)]
        else:
            t, floor, keys = conv_inputs(case), CONV_FLOOR, [("out", "stats", None)]
        worst = None
        for ko, ks, kind2 in keys:
            with torch.inference_mode():
                if fused:
                    f64, f32 = fused_reference(case, t, kind2, torch.float64), fused_reference(case, t, kind2, torch.float32)
                else:
                    f64, f32 = conv_reference(case, t, torch.float64), conv_reference(case, t, torch.float32)
            o = got[name][ko]
            rg, ra, mg, ma, holds, extra = errors(o, f32, f64, per_slice=name == "c64_slices")
            tag = "" if kind2 is None else f"kind2={kind2} "
            if not holds(floor):
                ok = False
                notes.append(f"{tag}outside the output bounds")
            if fused:
                failed, used = stats_ok(got[name][ks], got[name][f"tab{kind2}"], o, t["wn"], math.prod(case[3]))
                for k, v in used.items():
                    stat_use[k] = v if v != v else max(stat_use.get(k, 0.0), v)            # a NaN stays visible
                if failed:
                    ok = False
                    notes.extend(f"{tag}statistics: {f}" for f in failed)
            if ref is not None:
                for k in (ko, ks) + ((f"tab{kind2}",) if fused else ()):
                    if not torch.equal(got[name][k], ref[name][k]):
                        ok = False
                        notes.append(f"{tag}{k} differs from the round-3 routes: {first_mismatch(got[name][k], ref[name][k])}")
                rr = errors(ref[name][ko], f32, f64, per_slice=name == "c64_slices")
                extra += f"  (round-3 routes: rel-L2 {rr[0]:.2e}, max-abs {rr[2]:.2e}{'' if rr[4](floor) else ', OUTSIDE the bounds'})"
            if worst is None or rg > worst[0]:
                worst = (rg, ra, mg, ma, extra)
        rg, ra, mg, ma, extra = worst
        bad += 0 if ok else 1
        ab = "" if ref is None else ("  A/B out == stats ==" if not any("differs" in n for n in notes) else "  A/B !=")
        print(f"{name}: rel-L2 vs fp64 {rg:.2e} (torch fp32 {ra:.2e})  max-abs {mg:.2e} (torch fp32 {ma:.2e})"
              f"{'  stats / table, worst |err| / allowed: ' + ', '.join(f'{k} {v:.2f}' for k, v in stat_use.items()) if fused else ''}{ab}"
              f"  {'ok' if ok else 'FAIL'}{extra}", flush=True)
        for n in notes:
            print("   " + n, flush=True)
    print("volume_check:", "ALL OK" if bad == 0 else f"{bad} FAILED")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
