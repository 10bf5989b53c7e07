"""Chunked (tiled) decode of a latent volume through a VAEDecoder (reference: diffsci/extra/chunk_decode.py, "strategy B"):
the decode a latent sampler needs when ``decoder(z)`` does not fit, stage by stage with halos.

The walk is cut into stages -- stage 0 (post_quant_conv, conv_in, the middle blocks), one per upsampling level, the final one
(up[0], norm_out, conv_out) -- and every stage is produced tile by tile into a buffer that holds the whole stage: read the
tile's centre plus this stage's own halo from the previous stage's buffer (wrapping around on periodic axes, clamping at the
border otherwise), run the stage's launches on that window, keep the centre.  A stage's own halo is the growth of the receptive
field radius over it (``VAEDecoder.calculate_receptive_field``), in latent cells.

Same tiles, same windows and same values as the reference's function -- and like it, NOT the values of ``decoder(z)``:
GroupNorm takes its statistics from the tile it sees, so the result is a function of the tiling (a single tile equals the full
decode; DESIGN.md section 4.14 has the measured distance).  What differs is where the data lives: the stage buffers are device
tensors (the reference keeps them in host memory and moves every tile both ways), a tile is ``ops.box_copy3d`` (gather) ->
the stage's launches -> ``ops.box_copy3d`` (scatter of the centre), nothing synchronises between tiles, and the previous stage's
buffer is released as soon as its successor is complete.

``decode_plan`` is the tiling as plain integers: no tensors, no GPU.  ``chunk_decode_strategy_b_3d`` iterates over exactly it."""
import itertools
from typing import NamedTuple, Tuple

import torch

from .. import ops
from ..models.nets.vaenet import decoder_receptive_field

Triple = Tuple[int, int, int]


class Tile(NamedTuple):
    """One launch group of a stage; every triple in the tensor's axis order (H, W, D).  src_*: the read window in the previous
    stage's cells (on a periodic axis it may start below 0 and end past the side); crop_*: the centre inside the stage's output
    for that window; dst_*: where the centre goes in this stage's buffer."""
    src_start: Triple
    src_stop: Triple
    crop_start: Triple
    crop_stop: Triple
    dst_start: Triple
    dst_stop: Triple

    def row(self):
        """The 18 integers in the order of the fields."""
        return [v for t in self for v in t]


def _norm3(v, name):
    """An int, or three of them in (D, H, W) order."""
    if isinstance(v, int):
        return (v, v, v)
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return tuple(int(a) for a in v)
    raise ValueError(f"{name} must be int or 3-tuple/list (D, H, W). Got: {v!r}")


def _norm3_bool(v, name):
    if isinstance(v, bool):
        return (v, v, v)
    if isinstance(v, (tuple, list)) and len(v) == 3:
        return tuple(bool(a) for a in v)
    raise ValueError(f"{name} must be bool or 3-tuple/list (D, H, W). Got: {v!r}")


def _hwd(dhw):
    """(D, H, W), the order of the arguments, to (H, W, D), the order of the tensor's axes."""
    return (dhw[1], dhw[2], dhw[0])


def _refuse_config(config):
    # the reference's guard: any configured attention, whatever attn_type makes of it
    if config.has_mid_attn or len(config.attn_resolutions) > 0:
        raise NotImplementedError("This chunked decoder assumes NO attention in the decoder.")
    if config.dimension != 3:
        raise NotImplementedError(f"the chunked decode tiles volumes: dimension={config.dimension} is not implemented")


def stage_radii_and_scales(config):
    """(radii, scales): after each stage, the receptive-field radius in latent cells and the upsampling factor reached."""
    _refuse_config(config)
    info = decoder_receptive_field(config)
    n = int(config.num_resolutions)
    per_level = (int(config.num_res_blocks) + 1) * int(info["rf_per_block"])
    mid = int(info["rf_after_middle"])
    radii = [(mid + per_level * s) // 2 for s in range(n)] + [int(info["rf_latent"]) // 2]
    scales = [2 ** s for s in range(n)] + [2 ** max(0, n - 1)]
    return radii, scales


def _pieces(lo, hi, step):
    return [(a, min(a + step, hi)) for a in range(lo, hi, step)]


def _centre_spans(length, chunk, radius0):
    """Stage-0 centres along one axis: the whole axis when the chunk covers it, else steps of what the first halo leaves."""
    return [(0, length)] if chunk >= length else _pieces(0, length, max(1, chunk - 2 * radius0))


def decode_plan(config, latent_shape, chunk_latent, max_stage_out_chunk=128, periodicity=False):
    """The tiling of chunk_decode_strategy_b_3d as integers: a list with one list of ``Tile`` per stage.

    config: the decoder's VAENetConfig; latent_shape: (H, W, D), or the latent's full shape [B, z_dim, H, W, D];
    chunk_latent, max_stage_out_chunk, periodicity: as given to the decode, ints / bools or triples in (D, H, W) order."""
    radii, scales = stage_radii_and_scales(config)
    sides = tuple(int(s) for s in tuple(latent_shape)[-3:])
    if len(sides) != 3 or min(sides) < 1:
        raise ValueError(f"latent_shape must end in three positive sides (H, W, D); got {tuple(latent_shape)!r}")
    chunk = _hwd(_norm3(chunk_latent, "chunk_latent"))
    periodic = _hwd(_norm3_bool(periodicity, "periodicity"))
    cap = None if max_stage_out_chunk is None else _hwd(_norm3(max_stage_out_chunk, "max_stage_out_chunk"))
    spans = [_centre_spans(sides[a], chunk[a], radii[0]) for a in range(3)]
    order = (2, 0, 1)                                   # loops run D, H, W; triples are stored H, W, D
    plan, src_scale = [], 1
    for s, dest_scale in enumerate(scales):
        halo = max(0, radii[s] - (radii[s - 1] if s else 0))
        up = dest_scale // src_scale
        tiles = []
        for centre in itertools.product(*(spans[a] for a in order)):
            subs = []                                   # a stage's output tile stays within the cap, in its own cells
            for a, (lo, hi) in zip(order, centre):
                step = hi - lo if cap is None else max(1, min(hi - lo, cap[a] // dest_scale))
                subs.append(_pieces(lo, hi, step))
            for sub in itertools.product(*subs):
                t = [[0] * 3 for _ in range(6)]
                for a, (lo, hi) in zip(order, sub):
                    ws, we = lo - halo, hi + halo
                    if not periodic[a]:
                        ws, we = max(0, ws), min(sides[a], we)
                    t[0][a], t[1][a] = ws * src_scale, we * src_scale
                    t[2][a], t[3][a] = (lo - ws) * src_scale * up, (hi - ws) * src_scale * up
                    t[4][a], t[5][a] = lo * dest_scale, hi * dest_scale
                tiles.append(Tile(*(tuple(v) for v in t)))
        plan.append(tiles)
        src_scale = dest_scale
    return plan


def _run_stage(decoder, s, x):
    n = int(decoder.config.num_resolutions)
    if s == 0:
        return decoder._stage0(x)[0]
    if s < n:
        return decoder._up_stage(n - s, x)[0]
    return decoder._final_stage(x)


def chunk_decode_strategy_b_3d(decoder, z_latent, chunk_latent, *, device=None, time=None, debug=False, max_stage_out_chunk=128,
                               periodicity=False, output_device=None):
    """Decode z_latent [B, z_dim, H, W, D] through `decoder` (a VAEDecoder of volumes without attention) in tiles.

    chunk_latent: the stage-0 tile, halo included, in latent cells; max_stage_out_chunk: a cap on any stage's output tile, in
    that stage's cells (None: none); periodicity: the axes whose halos wrap around; each an int / bool or a triple in (D, H, W)
    order although the tensor's axes are (H, W, D).  z_latent may live on the CPU (it is copied to the decoder's device once).
    Returns [B, out_channels, H f, W f, D f], f = 2 ** (levels - 1): on the CPU as the reference does, or where it was computed
    with output_device given.  device: None, or the decoder's own.  time: None (time embeddings are not built).  debug prints
    the plan's sizes.  The decoder's training flag is restored on exit."""
    config = decoder.config
    _refuse_config(config)
    if time is not None:
        raise NotImplementedError("a time argument (with_time_emb) is outside the HIP sampling path: call with time=None")
    if not isinstance(z_latent, torch.Tensor) or z_latent.dim() != 5:
        raise ValueError("z_latent must be [B, z_dim, H, W, D]; got "
                         f"{tuple(z_latent.shape) if isinstance(z_latent, torch.Tensor) else type(z_latent).__name__}")
    if z_latent.shape[1] != config.z_dim:
        raise ValueError(f"z_latent has {z_latent.shape[1]} channels; the decoder expects z_dim = {config.z_dim}")
    plan = decode_plan(config, z_latent.shape, chunk_latent, max_stage_out_chunk, periodicity)
    _, scales = stage_radii_and_scales(config)
    if decoder.conv_precision not in ops.CONV_PRECISIONS:
        raise ValueError(f"unknown conv_precision {decoder.conv_precision!r}; choose from {ops.CONV_PRECISIONS}")
    weight = next(decoder.parameters())
    ops.require_device(weight, "the decoder")
    dev = weight.device
    if device is not None and torch.device(device) not in (dev, torch.device(dev.type)):
        raise ValueError(f"device={device!r}, but the decoder lives on {dev}: the tiles are computed where its weights are")
    B, sides = z_latent.shape[0], tuple(z_latent.shape[2:])
    if debug:
        print(f"chunk decode: latent {sides} (H, W, D), scales {scales}, tiles per stage {[len(t) for t in plan]}")
    was_training = decoder.training
    decoder.eval()
    try:
        with torch.cuda.device(dev):
            decoder._hand_down()
            src = z_latent.detach().to(device=dev, dtype=torch.float32).contiguous()
            for s, tiles in enumerate(plan):
                dst = None
                for t in tiles:
                    size = tuple(b - a for a, b in zip(t.src_start, t.src_stop))
                    window = torch.empty((B, src.shape[1]) + size, dtype=torch.float32, device=dev)
                    ops.box_copy3d(src, t.src_start, window, (0, 0, 0), size)
                    y = _run_stage(decoder, s, window)
                    if dst is None:
                        dst = torch.empty((B, y.shape[1]) + tuple(n * scales[s] for n in sides), dtype=torch.float32, device=dev)
                    ops.box_copy3d(y, t.crop_start, dst, t.dst_start, tuple(b - a for a, b in zip(t.crop_start, t.crop_stop)))
                src = dst                                # the previous stage's buffer is released here
            torch.cuda.synchronize(dev)
    finally:
        decoder.train(was_training)
    return src.cpu() if output_device is None else src.to(output_device)
