"""Time the LDM AutoencoderKL Decoder.forward on the GPU at the shapes a latent run decodes:
  2-D  ch=32, ch_mult=[1,2,4,4], z [8,4,32,32] -> [8,1,256,256]
  3-D  the same config,          z [1,4,8,8,8] -> [1,1,64,64,64]
for the folded and the standalone norm routes (fuse_norm; identical launches on volumes), next to the same architecture as eager
torch on the same GPU (tests/ldm_ref.py's functional restatement over the module's state_dict: F.conv, F.group_norm, bmm softmax).
Device events around `--iters` forwards after a warm-up, three rounds per variant, the variants alternating inside a round; the
median round is printed.  Outputs are compared first (rel-L2 against the torch result).

    python tools/ldm_decode_time.py                # the table
    python tools/ldm_decode_time.py --once 2d      # one warmed forward per route, for a kernel trace taken around this command"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffsci_amd.models.nets import autoencoderldm2d, autoencoderldm3d
from tests import ldm_ref

dev = torch.device("cuda:0")
CASES = {"2d": (autoencoderldm2d, (8, 4, 32, 32)), "3d": (autoencoderldm3d, (1, 4, 8, 8, 8))}


def build(which):
    mod, shape = CASES[which]
    torch.manual_seed(0)
    net = mod.Decoder(mod.ddconfig(ch=32, ch_mult=[1, 2, 4, 4], resolution=256 if which == "2d" else 64)).to(dev).eval()
    z = torch.randn(shape, device=dev)
    sd = {k: v.detach() for k, v in net.state_dict().items()}

    def hip(fuse):
        def run():
            net.fuse_norm = fuse
            return net(z)
        return run
    return net, {"hip folded": hip(True), "hip standalone": hip(False), "torch eager": lambda: ldm_ref.decoder(sd, z)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--once", choices=sorted(CASES), default=None)
    args = ap.parse_args()
    with torch.inference_mode():
        for which in ([args.once] if args.once else sorted(CASES)):
            net, variants = build(which)
            outs = {k: f() for k, f in variants.items()}                      # warm-up: code objects, packings, torch's algorithms
            torch.cuda.synchronize()
            ref = outs["torch eager"].double()
            print(f"--- {which} Decoder(ch=32, ch_mult=[1,2,4,4]) z {list(CASES[which][1])} -> {list(ref.shape)}", flush=True)
            for k, o in outs.items():
                print(f"{k:16s} rel-L2 vs torch eager {float((o.double() - ref).norm() / ref.norm()):.2e}", flush=True)
            if args.once:
                for k, f in variants.items():
                    f()
                torch.cuda.synchronize()
                continue
            rounds = {k: [] for k in variants}
            for _ in range(3):
                for k, f in variants.items():
                    f()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    rounds[k].append(e0.elapsed_time(e1) / args.iters)
            for k, r in rounds.items():
                print(f"{k:16s} {sorted(r)[1]:9.3f} ms per forward   (rounds: {', '.join(f'{v:.3f}' for v in r)})", flush=True)
            del net, variants, outs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
