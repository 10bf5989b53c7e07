"""Shared by tests/test_gpu_circular_dims.py and its child process: the persistent-kernel case of per-axis periodic padding.

The library reads DS_CONV_PC once per process, so the one-shot arm of a fused-loader launch (which the persistent kernel takes by
default) runs in a child with DS_CONV_PC=0:  python tests/circular_dims_pc.py OUT.pt  saves its results for every mask."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = (32, 64, 128, 32, 32)              # items = 2 channel tiles x 4 pixel tiles x 32 samples = 256
MASKS = ((True, False), (False, True))
EPS = 1e-5


def inputs():
    B, Cin, Cout, H, W = SHAPE
    g = torch.Generator().manual_seed(4242)
    x = torch.randn(B, Cin, H, W, generator=g) * 1.5 + 0.25
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    wn, bn = torch.randn(Cin, generator=g), torch.randn(Cin, generator=g)
    return x, w, bias, wn, bn


def table(ops, x, wn, bn):
    """The InstanceNorm table of x ([B, ceil16(Cin), 4] = (M, A, C, no exponent)), from fp64 statistics."""
    B, Cin = x.shape[:2]
    v = x.double()
    mean, var = v.mean(dim=(2, 3)), v.var(dim=(2, 3), unbiased=False)
    tab = torch.zeros(B, ops.table_channels(Cin), 4)
    tab[:, :Cin, 0], tab[:, :Cin, 1], tab[:, :Cin, 2] = mean.float(), (wn.double() / torch.sqrt(var + EPS)).float(), bn
    return tab


def run(ops, dev, mask, pre, pc_raw):
    """One launch; returns (out, tile statistics, out_amax) on the CPU."""
    B, Cin, Cout, H, W = SHAPE
    x, w, bias, wn, bn = inputs()
    pw = ops.pack_conv(w.to(dev), "fp16x3")
    ts = torch.zeros(B, Cout, ops.conv_tile_count(H, W), 4, device=dev)
    om = torch.zeros(B, dtype=torch.int32, device=dev)
    xd = x.to(dev)
    kw = dict(prenorm=table(ops, x, wn, bn).to(dev)) if pre else dict(in_amax=ops.absmax_rows(xd))
    out = ops.conv(xd, pw, bias=bias.to(dev), circular=mask, tile_stats=ts, out_amax=om, pc_raw=pc_raw, **kw)
    return out.cpu(), ts.cpu(), om.cpu()


if __name__ == "__main__":
    assert os.environ.get("DS_CONV_PC") == "0", "the child is the one-shot arm"
    from diffsci_amd import ops as _ops
    _dev = torch.device("cuda:0")
    torch.save({m: run(_ops, _dev, m, True, False) for m in MASKS}, sys.argv[1])
