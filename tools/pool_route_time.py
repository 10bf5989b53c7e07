"""Launch times of the two DownSamplers of config 2 (PUNetG-64, [64, 1, 128, 128]) on each PUNetG.pool_route, and of the residual
block's second convolution that produces their input with and without the pooled output of its store phase.
   python tools/pool_route_time.py [reps]"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffsci_amd import ops
from diffsci_amd._native import DS_LOAD_MAXPOOL2

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


for name, (B, C, S) in (("level 0 -> 1", (64, 64, 128)), ("level 1 -> 2", (64, 128, 64))):
    g = torch.Generator().manual_seed(0)
    h = torch.randn(B, C, S, S, generator=g).to(dev)                     # the level's last activation
    res1 = torch.randn(B, C, S, S, generator=g).to(dev)
    w2 = ops.pack_conv((torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9)).to(dev), "fp16x3")
    wd = ops.pack_conv((torch.randn(2 * C, C, 3, 3, generator=g) / math.sqrt(C * 9)).to(dev), "fp16x3")
    bias2, biasd = torch.randn(C, generator=g).to(dev), torch.randn(2 * C, generator=g).to(dev)
    tab = torch.zeros(B, ops.table_channels(C), 4)
    tab[:, :C, 0] = torch.randn(B, C, generator=g) * 0.3
    tab[:, :C, 1] = torch.rand(B, C, generator=g) + 0.5
    tab[:, :C, 2] = torch.randn(B, C, generator=g) * 0.3
    tab[:, :, 3] = 2.0 ** -3
    tab = tab.to(dev)
    oa = torch.zeros(B, dtype=torch.int32, device=dev)
    out2 = torch.empty(B, C, S, S, device=dev)
    pool = ops.PoolOut(torch.empty(B, C, S // 2, S // 2, device=dev))
    outd = torch.empty(B, 2 * C, S // 2, S // 2, device=dev)
    ts = torch.empty(B, 2 * C, ops.conv_tile_count(S // 2, S // 2), 4, device=dev)
    ia = ops.absmax_rows(h)
    hp = ops.maxpool_f(h, 2)
    kw2 = dict(bias=bias2, res1=res1, prenorm=tab, out_amax=oa, out=out2)
    kwd = dict(bias=biasd, tile_stats=ts, in_amax=ia, out=outd)
    t = {
        "conv2, plain": timed(lambda: ops.conv(h, w2, **kw2)),
        "conv2, pooled output": timed(lambda: ops.conv(h, w2, pool=pool, **kw2)),
        "DownSampler, max-pool loader": timed(lambda: ops.conv(h, wd, load_mode=DS_LOAD_MAXPOOL2, **kwd)),
        "pooling pass": timed(lambda: ops.maxpool_f(h, 2, out=hp)),
        "DownSampler, raw input, one-shot kernel": timed(lambda: ops.conv(hp, wd, **kwd)),
        "DownSampler, raw input, persistent kernel": timed(lambda: ops.conv(hp, wd, pc_raw=True, **kwd)),
    }
    assert pool.written
    print(f"{name}: [{B},{C},{S},{S}] -> [{B},{2 * C},{S // 2},{S // 2}]")
    for k, v in t.items():
        print(f"    {k:44s} {v:7.1f} us", flush=True)
    loader = t["conv2, plain"] + t["DownSampler, max-pool loader"]
    print(f"    loader   route: {loader:7.1f} us")
    print(f"    pass     route: {t['conv2, plain'] + t['pooling pass'] + t['DownSampler, raw input, persistent kernel']:7.1f} us")
    print(f"    epilogue route: {t['conv2, pooled output'] + t['DownSampler, raw input, persistent kernel']:7.1f} us")
