"""Time VAENet's encode and decode on the GPU, and the stride-2 convolution launch alone:
  2-D  case a's architecture (ch=32, ch_mult=[1,2], attn_resolutions=[] at this size) at 256 x 256, batch 8
  3-D  case c's architecture (ch=32, ch_mult=[1,2]) at 64^3, batch 1
  the encoder's Downsample convolution at those shapes ([8,32,256,256], [1,32,64,64,64]) and at 128 channels, against the route
  the package had before it: the stride-1 convolution of the input zero-padded at the far end, then every second output
  (four times the arithmetic), and the exact-fp32 direct kernel.
Device events around `--iters` calls after a warm-up, three rounds per variant, the variants alternating inside a round; the
median round is printed.  Outputs of the two routes are compared first.

    python tools/vaenet_time.py"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from diffsci_amd import ops
from diffsci_amd.models.nets import vaenet

dev = torch.device("cuda:0")


def timed(variants, iters):
    rounds = {k: [] for k in variants}
    for _ in range(3):
        for k, f in variants.items():
            f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            rounds[k].append(e0.elapsed_time(e1) / iters)
    for k, r in rounds.items():
        print(f"  {k:44s} {sorted(r)[1]:9.3f} ms   (rounds: {', '.join(f'{v:.3f}' for v in r)})", flush=True)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def networks(iters):
    for name, cfg, shape in (("2-D", dict(dimension=2, ch=32, ch_mult=[1, 2], num_res_blocks=1, resolution=256, z_channels=4, z_dim=3),
                              (8, 1, 256, 256)),
                             ("3-D", dict(dimension=3, ch=32, ch_mult=[1, 2], num_res_blocks=1, resolution=64), (1, 1, 64, 64, 64))):
        torch.manual_seed(0)
        # mid attention over a 128 x 128 (32^3) latent is not what this first stage is used with at these sizes
        net = vaenet.VAENet(vaenet.VAENetConfig(has_mid_attn=False, **cfg)).to(dev).eval()
        x = torch.randn(shape, device=dev)
        z = net.encode(x)
        print(f"--- {name} VAENet(ch=32, ch_mult=[1,2]) x {list(shape)} -> z {list(z.shape)}", flush=True)

        def enc(fuse):
            def run():
                net.fuse_norm = fuse
                return net.encode(x)
            return run

        def dec(fuse):
            def run():
                net.fuse_norm = fuse
                return net.decode(z)
            return run
        variants = {"encode (folded norms)": enc(True), "encode (standalone norms)": enc(False),
                    "decode (folded norms)": dec(True), "decode (standalone norms)": dec(False)}
        if name == "3-D":                                       # identical launches on volumes
            variants = {"encode": enc(True), "decode": dec(True)}
        timed(variants, iters)
        del net
        torch.cuda.empty_cache()


def launches(iters):
    for B, C, H, W in ((8, 32, 256, 256), (8, 128, 128, 128), (2, 64, 64, 64)):
        torch.manual_seed(1)
        x = torch.randn(B, C, H, W, device=dev)
        w = torch.randn(C, C, 3, 3, device=dev) / (3 * C ** 0.5)
        b = torch.randn(C, device=dev)
        pk, pd = ops.pack_conv(w, "fp16x3"), ops.pack_conv_s2(w, "fp32")
        am = ops.absmax_rows(x)
        xp = F.pad(x, (0, 1, 0, 1))
        amp = ops.absmax_rows(xp)
        out = torch.empty(B, C, H // 2, W // 2, device=dev)
        full = torch.empty(B, C, H + 1, W + 1, device=dev)

        def old():
            ops.conv(xp, pk, bias=b, in_amax=amp, out=full)
            return full[..., 1::2, 1::2][..., :H // 2, :W // 2].contiguous()
        new = lambda: ops.conv_s2(x, pk, bias=b, in_amax=am, out=out)  # noqa: E731
        print(f"--- stride-2 3x3 convolution [{B},{C},{H},{W}]: routes agree to {rel(new(), old()):.2e}", flush=True)
        timed({"stride-2 launch (fp16x3)": new,
               "stride-1 over the padded input + subsample": old,
               "  of which the stride-1 launch alone": lambda: ops.conv(xp, pk, bias=b, in_amax=amp, out=full),
               "stride-2 exact-fp32 direct kernel": lambda: ops.conv_s2(x, pd, bias=b, out=out)}, iters)
    B, C, D = 1, 32, 64
    torch.manual_seed(2)
    x = torch.randn(B, C, D, D, D, device=dev)
    w = torch.randn(C, C, 3, 3, 3, device=dev) / (27 * C) ** 0.5
    b = torch.randn(C, device=dev)
    ps, pd, p1 = ops.pack_conv3d_s2(w, "fp16x3"), ops.pack_conv3d_s2(w, "fp32"), ops.pack_conv3d(w)
    xp = F.pad(x, (0, 1) * 3)

    def old3():
        return ops.conv3d_mfma(xp, p1, bias=b)[..., 1::2, 1::2, 1::2][..., :D // 2, :D // 2, :D // 2].contiguous()
    print(f"--- stride-2 3x3x3 convolution [{B},{C},{D},{D},{D}]: routes agree to {rel(ops.conv3d_s2(x, ps, bias=b), old3()):.2e}", flush=True)
    timed({"stride-2 composition (fp16x3 depth taps)": lambda: ops.conv3d_s2(x, ps, bias=b),
           "stride-1 over the padded volume + subsample": old3,
           "stride-2 exact-fp32 direct kernel": lambda: ops.conv3d_s2(x, pd, bias=b)}, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    with torch.inference_mode():
        launches(args.iters)
        networks(args.iters)


if __name__ == "__main__":
    main()
