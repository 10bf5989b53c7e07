"""Time the chunked volume decode's data movement and the decode itself on the GPU (a report, not a test):
  ops.box_copy3d against the same window assembled by torch on the device -- narrow per axis, cat where the window wraps,
      .contiguous() -- for windows of 64^3 and 128^3 x 32 planes out of a [1, 32, 256, 256, 256] stage buffer, unwrapped and
      wrapped in all three axes; time and achieved GB/s (window bytes read + written, over the time)
  extra.chunk_decode_strategy_b_3d against decoder(z) for VAENet(ch=32, ch_mult=[1,2,4]) on z [1,4,32,32,32] (a 128^3 volume),
      caps 128 (one tile per stage) and 64; time and torch.cuda.max_memory_allocated of each
Device events around `--iters` calls after a warm-up, three rounds per variant, the variants alternating inside a round; the
median round is printed with all three, so the spread is on the page.  Outputs are compared first.

    python tools/chunk_decode_time.py"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffsci_amd import ops
from diffsci_amd.extra import chunk_decode_strategy_b_3d
from diffsci_amd.models.nets import vaenet

dev = torch.device("cuda:0")


def timed(variants, iters, nbytes=None):
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
        mid = sorted(r)[1]
        rate = f"  {nbytes / mid / 1e6:8.1f} GB/s" if nbytes else ""
        print(f"  {k:46s} {mid:9.4f} ms{rate}   (rounds: {', '.join(f'{v:.4f}' for v in r)})", flush=True)


def torch_window(src, start, size):
    """The window as periodic_getitem_extended assembles it (one period at most), then one contiguous copy."""
    out = src
    for axis, (s, n) in enumerate(zip(start, size), start=2):
        S = out.shape[axis]
        s %= S
        if s + n <= S:
            out = out.narrow(axis, s, n)
        else:
            out = torch.cat([out.narrow(axis, s, S - s), out.narrow(axis, 0, n - (S - s))], dim=axis)
    return out.contiguous()


def copies(iters):
    torch.manual_seed(0)
    src = torch.randn(1, 32, 256, 256, 256, device=dev)
    for side in (64, 128):
        size = (side,) * 3
        out = torch.empty((1, 32) + size, device=dev)
        for what, start in (("unwrapped", (40, 40, 40)), ("wrapped in all three axes", (-9, 256 - 17, -side // 2))):
            assert torch.equal(ops.box_copy3d(src, start, out, (0, 0, 0), size), torch_window(src, start, size))
            print(f"--- window {side}^3 x 32 planes, {what}: start {start}", flush=True)
            timed({"ops.box_copy3d": lambda: ops.box_copy3d(src, start, out, (0, 0, 0), size),
                   "torch narrow + cat + contiguous": lambda: torch_window(src, start, size)}, iters, nbytes=2 * out.numel() * 4)
    del src
    torch.cuda.empty_cache()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def decodes(iters):
    torch.manual_seed(1)
    cfg = vaenet.VAENetConfig(dimension=3, ch=32, ch_mult=[1, 2, 4], has_mid_attn=False, resolution=128)
    dec = vaenet.VAEDecoder(cfg).to(dev).eval()
    z = torch.randn(1, cfg.z_dim, 32, 32, 32, device=dev)
    variants = {"decoder(z)": lambda: dec(z)}
    for cap in (128, 64):
        variants[f"chunked, cap {cap}"] = lambda cap=cap: chunk_decode_strategy_b_3d(dec, z, 64, max_stage_out_chunk=cap,
                                                                                     output_device=dev)
    full = variants["decoder(z)"]()
    print(f"--- VAEDecoder(ch=32, ch_mult=[1,2,4]) z {list(z.shape)} -> {list(full.shape)}", flush=True)
    for k, f in variants.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = f()
        torch.cuda.synchronize()
        print(f"  {k:46s} peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:9.1f} MiB (of which held before the call "
              f"{base / 2 ** 20:.1f}); vs decoder(z) rel-L2 {rel(out, full):.2e}", flush=True)
        del out
    timed(variants, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--decode-iters", type=int, default=3)
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    with torch.inference_mode():
        copies(args.iters)
        decodes(args.decode_iters)


if __name__ == "__main__":
    main()
