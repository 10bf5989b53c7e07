"""A/B timing of the statistics-writing 3x3 fp16x3 launches: this tree's library against another build of it (the parent commit's),
loaded side by side in one process and timed in alternating series between device events (what does the robust
shift of the tile statistics cost?).

    python tools/tile_stats_time.py --other /path/to/parent/libdiffsci_hip.so [--launches 300] [--series 6]

Shapes: config 2's levels 0 and 1, [64,64,128,128] and [64,128,64,64], C -> C.  Raw input runs the one-shot kernel, a prenorm table
the persistent one (level 0) or the two-channel-tile one-shot kernel (level 1); each with tile statistics and a residual, and without
statistics for reference.  Before timing, the two libraries' outputs are compared bit for bit (the statistics differ by design: the
shift K is another value).  Per row: every series' ms per launch, and min / median / max per library.  The statistic that decides
is the minimum (the least disturbed series); a library is slower when its minimum lies above the other's maximum, i.e. outside the
interval the other library's own repeated series span."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsci_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True, help="the other build of libdiffsci_hip.so")
ap.add_argument("--launches", type=int, default=300, help="launches per series")
ap.add_argument("--series", type=int, default=6, help="series per library, alternating")
args = ap.parse_args()

dev = torch.device("cuda:0")
new = N.lib()
old = ctypes.CDLL(args.other)
old.ds_conv2d_h3.restype = ctypes.c_int
old.ds_conv2d_h3.argtypes = new.ds_conv2d_h3.argtypes


def p(t):
    return None if t is None else t.data_ptr()


def launch(L, out, x, wp, B, C, S, tab, res, ts):
    rc = L.ds_conv2d_h3(p(out), p(x), p(wp), 0, None, None, 0, p(res), None, B, C, C, S, S, 0, p(tab), p(ts), None, None, None)
    assert rc == 0, rc


def time_ms(L, a, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch(L, *a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    s = sorted(v)
    return f"min {s[0]:.4f} median {(s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2:.4f} max {s[-1]:.4f}"


for B, C, S in ((64, 64, 128), (64, 128, 64)):
    torch.manual_seed(0)
    x = torch.randn(B, C, S, S, device=dev)
    res = torch.randn(B, C, S, S, device=dev)
    w = torch.randn(C, C, 3, 3, device=dev) * 0.02
    wp = torch.empty(new.ds_conv2d_h3_packed_bytes(C, C) // 4, device=dev)
    assert new.ds_conv2d_h3_pack_weights(p(wp), p(w), C, C, 0, None) == 0
    tab = torch.zeros(B, (C + 15) // 16 * 16, 4, device=dev)
    tab[:, :, 1] = 1.0
    nt = new.ds_conv_tile_count(S, S)
    for form, t in (("raw", None), ("prenorm", tab)):
        for with_stats in (True, False):
            o_new, o_old = torch.empty_like(x), torch.empty_like(x)
            ts_new = torch.zeros(B, C, nt, 4, device=dev) if with_stats else None
            ts_old = torch.zeros(B, C, nt, 4, device=dev) if with_stats else None
            a_new, a_old = (o_new, x, wp, B, C, S, t, res, ts_new), (o_old, x, wp, B, C, S, t, res, ts_old)
            for _ in range(5):
                launch(new, *a_new)
                launch(old, *a_old)
            torch.cuda.synchronize()
            assert torch.equal(o_new, o_old), (form, with_stats)
            rows = {"this": [], "other": []}
            for rep in range(args.series):
                order = (("other", old, a_old), ("this", new, a_new))
                for name, L, a in order if rep % 2 == 0 else order[::-1]:
                    rows[name].append(time_ms(L, a, args.launches))
            print(f"[{B},{C},{S},{S}] {form:7s} residual, {'tile statistics' if with_stats else 'no statistics '}: outputs bit-identical", flush=True)
            for name in ("other", "this"):
                print(f"    {name:5s} ms/launch: " + " ".join(f"{v:.4f}" for v in rows[name]) + f" | {stats(rows[name])}", flush=True)
            print(f"    this slower than other's own interval: {min(rows['this']) > max(rows['other'])}", flush=True)
