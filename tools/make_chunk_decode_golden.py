"""Generate tests/golden/chunk_decode_{a,b}.npz: the reference's chunked volume decode (diffsci/extra/chunk_decode.py,
chunk_decode_strategy_b_3d) run on the CPU in fp32 and as an fp64 copy (imported through oracle/tools/refshim.py; needs the
reference checkout that shim points at).  Data only: the decoder's state_dict, the latent, and per tiling the reference's output
in both precisions and its plan -- one int array [tiles, 18] per stage, a row being the read window's start and stop in the
previous stage's cells, the crop's start and stop in the tile's output, the destination box's start and stop, each as (H, W, D)
-- recorded by wrapping the slices it hands to periodic_getitem_extended, the result of _compute_tile_crop_coords and the box it
hands to _CPUStageBuffer.write_block.  Also the full decode, and as JSON strings the configuration, the tilings' arguments, the
stage radii and scales, and calculate_receptive_field() of the encoder, the decoder and the net (file a: of the default
VAENetConfig() too, which has attention).

    a   ch=8 num_groups=4 ch_mult=[1,2] num_res_blocks=1 z_channels=2 z_dim=2; z [1,2,6,5,12]; radii [5,9,14]
    b   ch=8 num_groups=8 ch_mult=[1,2,2] num_res_blocks=1 z_channels=3 z_dim=2 out_channels=2 resamp_with_conv=False
        memory_efficient_variant=True tanh_out=True output_bias=False; z [2,2,4,3,6]; radii [5,9,13,18], scales [1,2,4,4]

Both without attention (has_mid_attn=False), resolution=16; norm affines and every bias perturbed (+ 0.25 randn).

    python tools/make_chunk_decode_golden.py"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
from diffsci.extra import chunk_decode as C  # noqa: E402
from diffsci.models.nets import vaenet as R  # noqa: E402

torch.set_num_threads(8)
# tilings: chunk_latent, max_stage_out_chunk, periodicity, each an int / bool or (D, H, W)
CASES = {
    "a": (dict(dimension=3, ch=8, num_groups=4, ch_mult=[1, 2], num_res_blocks=1, z_channels=2, z_dim=2, has_mid_attn=False,
               resolution=16), (1, 2, 6, 5, 12), 610,
          [(64, None, False),
           (64, 4, False),
           (64, 4, True),
           ((11, 64, 64), (6, 8, 4), (True, False, True)),
           (64, (24, 4, 6), (False, True, False))]),
    "b": (dict(dimension=3, ch=8, num_groups=8, ch_mult=[1, 2, 2], num_res_blocks=1, z_channels=3, z_dim=2, out_channels=2,
               resamp_with_conv=False, memory_efficient_variant=True, tanh_out=True, output_bias=False, has_mid_attn=False,
               resolution=16), (2, 2, 4, 3, 6), 612,
          [(64, None, False),
           (64, (8, 16, 4), (True, False, True)),
           ((16, 4, 13), (12, 8, 8), (False, True, False))]),
}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def perturb(module):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if "norm" in k or k.endswith("bias"):
                v.add_(0.25 * torch.randn_like(v))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@contextlib.contextmanager
def recorded(stages):
    """Collect the reference's plan while it runs: per tile the window slices, the crop and the destination box."""
    getitem, crop_fn, init, write = (C.periodic_getitem_extended, C._compute_tile_crop_coords, C._CPUStageBuffer.__init__,
                                     C._CPUStageBuffer.write_block)
    record = {}

    def getitem_(flat, everything, sy, sx, sz):
        record["src"] = [sy.start, sx.start, sz.start, sy.stop, sx.stop, sz.stop]
        return getitem(flat, everything, sy, sx, sz)

    def crop_(*a, **k):
        c = crop_fn(*a, **k)
        record["crop"] = [c.yH_start, c.yW_start, c.yD_start, c.yH_end, c.yW_end, c.yD_end]
        return c

    def init_(self, *a, **k):
        stages.append([])
        return init(self, *a, **k)

    def write_(self, z0, z1, y0, y1, x0, x1, tile):
        stages[-1].append(record.pop("src") + record.pop("crop") + [y0, x0, z0, y1, x1, z1])
        return write(self, z0, z1, y0, y1, x0, x1, tile)

    C.periodic_getitem_extended, C._compute_tile_crop_coords = getitem_, crop_
    C._CPUStageBuffer.__init__, C._CPUStageBuffer.write_block = init_, write_
    try:
        yield
    finally:
        C.periodic_getitem_extended, C._compute_tile_crop_coords = getitem, crop_fn
        C._CPUStageBuffer.__init__, C._CPUStageBuffer.write_block = init, write


def jsonable(d):
    return json.dumps(d)               # float('inf') is written as Infinity, which json.loads reads back


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    for tag, (cfg_kw, zshape, seed, tilings) in CASES.items():
        torch.manual_seed(seed)
        net = quiet(R.VAENet, R.VAENetConfig(**cfg_kw)).eval()
        perturb(net)
        dec = net.decoder
        sd = dec.state_dict()
        dec64 = quiet(R.VAEDecoder, R.VAENetConfig(**cfg_kw)).double().eval()
        dec64.load_state_dict({k: v.double() for k, v in sd.items()})
        torch.manual_seed(seed + 1)
        z = torch.randn(*zshape)
        radii, scales = C._compute_stage_radii_and_scales(dec)
        info = dict(config=cfg_kw, radii=radii, scales=scales, tilings=[list(t) for t in tilings],
                    rf=dict(encoder=net.encoder.calculate_receptive_field(), decoder=dec.calculate_receptive_field(),
                            net=net.calculate_receptive_field()))
        if tag == "a":
            default = quiet(R.VAENet, R.VAENetConfig())
            info["rf_default"] = dict(encoder=default.encoder.calculate_receptive_field(),
                                      decoder=default.decoder.calculate_receptive_field(), net=default.calculate_receptive_field())
        arrs = {"sd/" + k: v for k, v in sd.items()}
        arrs.update(info=jsonable(info), z=z)
        with torch.inference_mode():
            arrs["full_f32"] = full = dec(z)
        for i, (chunk, cap, per) in enumerate(tilings):
            stages = []
            kw = dict(device="cpu", max_stage_out_chunk=cap, periodicity=per)
            with recorded(stages):
                out32 = C.chunk_decode_strategy_b_3d(dec, z, chunk, **kw)
            out64 = C.chunk_decode_strategy_b_3d(dec64, z.double(), chunk, **kw)
            assert len(stages) == len(radii)
            arrs[f"t{i}/out_f32"], arrs[f"t{i}/out_f64"] = out32, out64
            for s, rows in enumerate(stages):
                arrs[f"t{i}/plan_s{s}"] = np.asarray(rows, dtype=np.int64).reshape(-1, 18)
            print(f"chunk_decode_{tag} tiling {i} {chunk!r} cap {cap!r} periodic {per!r}: tiles per stage "
                  f"{[len(r) for r in stages]}; fp32 vs fp64 {rel(out32, out64):.3e}; vs the full decode {rel(out32, full):.3e}",
                  flush=True)
        path = os.path.join(gold, f"chunk_decode_{tag}.npz")
        np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
        assert os.path.getsize(path) < 1 << 20, path
        print(f"chunk_decode_{tag}: {os.path.getsize(path) / 1024:.1f} KiB, radii {radii}, scales {scales}", flush=True)


if __name__ == "__main__":
    main()
