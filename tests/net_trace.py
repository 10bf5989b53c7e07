"""A whole PUNetG or ADM forward (or one stand-alone ADM block) through the recording stand-in of tests/abi_trace.py, on the host,
and the tables of network configurations whose records are pinned (TABLES: tests/golden/<table>.json.gz, written by
tools/make_net_trace_golden.py from the PARENT commit's diffsci_amd/).  A record holds, per case, every launch (entry point, arguments, pointers as [label, byte
offset]) and, among them, every return of a buffer to the pool; how many pool buffers were taken and how many never given back; and a digest of every pool buffer ATen wrote
(fill_, copy_, torch.add(out=)): kernels do not run, so a pool buffer holds its take number + 1 until torch itself writes it.
No RNG: parameters, buffers and inputs are filled from the arithmetic pattern of abi_trace.Ctx.f, so the packed weights' shift
words -- launch arguments -- are the same everywhere.  diffsci_amd is imported inside the functions: the golden tool runs this
module with the parent's package first on sys.path."""
import ctypes
import hashlib

import torch

from . import abi_trace

B = 2
BASE = dict(input_channels=2, output_channels=1, model_channels=16, channel_expansion=(2,), number_resnet_downward_block=2,
            number_resnet_upward_block=2, number_resnet_attn_block=2, number_resnet_before_attn_block=1,
            number_resnet_after_attn_block=1)
ADM_BASE = dict(input_channels=2, output_channels=1, model_channels=16, time_embed_dim=8, output_embed_dim=16, channel_expansion=(2,),
                number_resnet_downward_block=2, number_resnet_upward_block=2, number_resnet_attn_block=2,
                number_resnet_before_attn_block=1, number_resnet_after_attn_block=1)
PC = "ds_conv2d_h3_pc"


class Recorder(abi_trace.Recorder):
    """ds_conv2d_h3_pc is no launch by abi_trace.is_launch -- its stream is not last, and it answers `pooled` on the host --
    and the real entry asks for a device.  Recorded like a launch, minus the answer pointer; the answer is written here: 1
    when a pool pointer was passed and the case says the kernel pools, else 0."""

    def __init__(self, real, pooled):
        super().__init__(real)
        self._pooled = pooled

    def __getattr__(self, name):
        if name != PC:
            return super().__getattr__(name)
        N = _native()
        types = N._PROTOS[PC][1]
        answer = types.index(ctypes.POINTER(ctypes.c_int))

        def launch(*args):
            assert len(args) == len(types), (PC, len(args), len(types))
            self.calls.append([PC] + [self._arg(v, t) for i, (v, t) in enumerate(zip(args, types)) if i != answer])
            args[answer]._obj.value = int(self._pooled and args[answer - 1] is not None)
            return 0
        return launch


class Pool(abi_trace.Pool):
    """Buffer n is filled with n + 1 on take; `writes` digests every buffer that no longer holds that value uniformly.  No buffer
    is handed out twice, so WHEN one goes back is recorded among the launches (["give", label]): a real pool hands it to the
    next take of its shape, and a buffer given back before its last reader has been launched would be overwritten under it."""

    def __init__(self, rec):
        super().__init__(rec)
        self.bufs = []

    def take(self, shape, device):
        t = super().take(shape, device)
        t.fill_(float(self.n))
        self.bufs.append(t)
        return t

    def give(self, t):
        super().give(t)
        self.rec.calls.append(["give", self.rec._pointer(t.data_ptr())[0]])

    def writes(self):
        return [[f"pool{i}", hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()]
                for i, t in enumerate(self.bufs) if not bool((t == float(i + 1)).all())]


def _native():
    from diffsci_amd import _native as N
    return N


def pattern(k, *shape):
    """Ctx.f's values, started k steps further on: exact in fp32, different for different k."""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n, dtype=torch.float32) * 37 + 7 * k) % 101) - 50).div(64).reshape(shape).contiguous()


class Half(torch.nn.Module):
    """An extra_residual of exact arithmetic."""

    def forward(self, x):
        return x * 0.5


def punetg(dim, cls="PUNetG", cls_args=(), **cfg):
    """A network family: -> the network of one case and the switches it gets whatever the environment says."""
    from diffsci_amd.models.nets import punetg as nets
    from diffsci_amd.models.nets.punetg_config import PUNetGConfig
    config = PUNetGConfig(**{**BASE, "dimension": dim, **cfg})
    return getattr(nets, cls)(config, *cls_args), dict(pool_route="epilogue", norm_images=True)


def adm(dim, cls_args=(), **cfg):
    from diffsci_amd.models.nets import adm as nets
    return nets.ADM(nets.ADMConfig(**{**ADM_BASE, **cfg}), *cls_args), dict(norm_images=True, tile_stats_norms=True)


def adm_block(dim, cls="ADMBaseBlock", **kw):
    """A stand-alone block: no pool, every buffer torch's own ("fresh")."""
    from diffsci_amd.models.nets import adm as nets
    return getattr(nets, cls)(dimension=dim, **kw), {}


class Net:
    """One case's network under trace: c.net, the recorder c.rec, named inputs from c.f / c.x."""

    def __init__(self, rec, pool, family=punetg, dim=2, side=8, switches=(), **kw):
        self.rec, self.dim, self.side, self.k = rec, dim, side, 0
        net, fixed = family(dim, **kw)
        self.net = net = net.eval()
        tensors = list(net.named_parameters()) + list(net.named_buffers())
        for k, (name, t) in enumerate(tensors):
            with torch.no_grad():
                t.copy_(pattern(k, *t.shape))
            rec.name(name, t.detach())
        self.k = len(tensors)
        for name, v in list(fixed.items()) + list(switches):
            setattr(net, name, v)
        if hasattr(net, "_ws"):
            net._ws = pool
        names = {id(m): n for n, m in net.named_modules()}
        for key, v in (net.packed_weights() if hasattr(net, "packed_weights") else net._packs()).items():
            label = key if isinstance(key, str) else (names[key[0]] + "." + key[1] if isinstance(key, tuple) else names[key])
            self._name_packed("pk:" + label, v)

    def _name_packed(self, label, v):
        if isinstance(v, torch.Tensor):
            self.rec.name(label, v)
        elif isinstance(v, (list, tuple)):
            for z, p in enumerate(v):
                self._name_packed(f"{label}.z{z}", p)
        else:                                                                    # an ops.PackedConv, as abi_trace.Ctx.pack labels it
            for tag, p in [("", v)] + [(f".sub{i}", s[2]) for i, s in enumerate(v.subs or [])]:
                if p.data is not None:
                    self.rec.name(label + tag, p.data)
                if p.up is not None:
                    self.rec.name(label + tag + ".up", p.up)

    def name_timeblock_convs(self):
        """The 1x1 packings of the per-pixel time MLPs (a field of shifts)."""
        lins = {id(m): n for n, m in self.net.named_modules()}
        for key, v in self.net._timeblock_convs().items():
            self._name_packed("tb:" + lins[key], v)

    def f(self, label, *shape):
        self.k += 1
        return self.rec.name(label, pattern(self.k, *shape))

    def x(self, channels=None, label="x"):
        channels = self.net.config.input_channels if channels is None else channels
        return self.f(label, B, channels, *[self.side] * self.dim)

    def widths(self):
        return [blk.conv1.out_channels for blk in self.net._resblocks()]


def _forward(c):
    """PUNetG fields and ADM: the whole eager evaluation, time embedding and per-block MLPs included.  Volumes: from tabulated shifts of known
    contents -- ops.conv3d_mfma copies the shift rows into a pool buffer with ATen, and the MLPs' results are never computed."""
    if c.dim == 2:
        c.net.forward_unguarded(c.x(), c.f("t", B))
    else:
        c.net.forward_with_shifts(c.x(), [c.f(f"shift{k}", B, C) for k, C in enumerate(c.widths())])


def _rows(c):
    shifts = [c.f(f"shift{k}", 5, C) for k, C in enumerate(c.widths())]
    c.net.forward_with_shifts(c.x(), shifts, row=3, out=c.x(c.net.config.output_channels, "out"))


def _field(c):
    c.name_timeblock_convs()
    mc = c.net.config.model_channels
    ye = c.f("ye", 1 if c.dim == 3 else B, mc, *[c.side] * c.dim)
    c.net.forward_with_shifts(c.x(), c.net.field_shifts(c.f("te", B, mc), ye, B))


def _field_tensors(c):
    c.net.forward_with_shifts(c.x(), [c.f(f"shift{k}", B, C, c.side, c.side) for k, C in enumerate(c.widths())])


def _cond(c):
    c.net.forward_unguarded(c.x(1), c.f("t", B), {"c": c.f("c", 1, 1, c.side, c.side)})


def _stages(c):
    net, te = c.net, c.f("te", B, c.net.config.model_channels)
    h, skips = net.encode(c.x(net.config.model_channels), te)                    # the stages start after the input layer
    net.decode(net.bottom_forward(h, te), te, skips)


def case(run=_forward, pooled=True, **kw):
    return run, pooled, kw


def both(name, **kw):
    return {f"{name}_2d": case(**kw), f"{name}_3d": case(dim=3, **kw)}


ONE_EACH = dict(number_resnet_downward_block=1, number_resnet_upward_block=1, number_resnet_attn_block=1)
CASES = {
    **both("default"),
    **both("circular", convolution_type="circular"),
    "mp_cosine_2d": case(convolution_type="mp", attn_type="cosine"),
    "factor3_2d": case(transition_scale_factor=3, side=12),
    "factor3_3d": case(transition_scale_factor=3, side=6, dim=3),
    "nobias_3d": case(bias=False, dim=3),
    "nobias_fourier_2d": case(bias=False, in_embedding=True),
    "attn0_2d": case(number_resnet_attn_block=0),
    "attn0_after0_2d": case(number_resnet_attn_block=0, number_resnet_after_attn_block=0),  # x + x feeds the UpSampler
    "attn1_after0_2d": case(number_resnet_attn_block=1, number_resnet_after_attn_block=0),
    "attn3_before0_2d": case(number_resnet_attn_block=3, number_resnet_before_attn_block=0),
    "attn_residual_2d": case(attn_residual=True),
    "grouppix_2d": case(first_resblock_norm="GroupPix"),
    "k5_2d": case(kernel_size=5),
    "k5_3d": case(kernel_size=5, dim=3, **ONE_EACH),
    "inout5_out8_2d": case(in_out_kernel_size=5, output_channels=8),
    "nolevel_out8_2d": case(channel_expansion=(), output_channels=8),
    **both("unfused", switches=(("fuse_norm", False),)),
    "images_2d": case(model_channels=32, side=16, switches=(("fuse_max_cot", 0),)),
    "images_off_2d": case(model_channels=32, side=16, switches=(("fuse_max_cot", 0), ("norm_images", False))),
    "table_images_2d": case(model_channels=32, side=72, switches=(("fuse_max_cot", 0),)),   # 72 x 72 planes: not the image kernel's
    "bf16x6_2d": case(switches=(("conv_precision", "bf16x6"),)),
    "fp32_3d": case(dim=3, switches=(("conv_precision", "fp32"),)),
    "exact_input_2d": case(switches=(("exact_input_layer", True),)),
    "pool_loader_2d": case(switches=(("pool_route", "loader"),)),
    "pool_pass_2d": case(switches=(("pool_route", "pass"),)),
    "pool_declined_2d": case(pooled=False),
    **both("rows", run=_rows),
    **both("field", run=_field),
    "field_tensors_2d": case(run=_field_tensors),
    **both("extra_residual", cls_args=(None, Half())),
    "cond_2d": case(run=_cond, cls="PUNetGCond", cls_args=(None, ["c"])),
    "stages_2d": case(run=_stages),
    "stages_factor3_2d": case(run=_stages, transition_scale_factor=3, side=12),
}


def _adm_rows(c):
    shifts = [c.f(f"shift{k}", 5, 2 * blk.cout) for k, blk in enumerate(c.net._blocks())]
    c.net.forward_with_shifts(c.x(), shifts, row=3, out=c.x(c.net.config.output_channels, "out"))


def _adm_cond(c):
    c.net.forward_unguarded(c.x(), c.f("t", B), c.f("y", B, c.net.config.output_embed_dim))


def _block(c):
    """blk(x, te[, skip]) of a stand-alone block, on fields or volumes."""
    blk, sides = c.net, [c.side] * c.dim
    skip = c.f("skip", B, blk.channels_skip, *sides) if blk.channels_skip else None
    blk(c.f("x", B, blk.channels_in, *sides), c.f("te", B, blk.channels_embed), skip)


def acase(**kw):
    return case(family=adm, **kw)


def blocks(name, side=8, side3=4, **kw):
    """One stand-alone block with a residual branch, on fields and on volumes."""
    kw = dict(run=_block, family=adm_block, channels_in=16, channels_out=32, channels_embed=8, has_residual=True, **kw)
    return {f"block_{name}_2d": case(side=side, **kw), f"block_{name}_3d": case(dim=3, side=side3, **kw)}


IMAGES = dict(model_channels=32, side=16, switches=(("fuse_max_cot", 0),))
ADM_CASES = {
    "default": acase(),
    "circular": acase(convolution_type="circular"),
    "decoder2": acase(decoder_type=2),
    "add": acase(skip_integration_type="add"),
    "decoder2_add": acase(decoder_type=2, skip_integration_type="add"),
    "factor3": acase(transition_scale_factor=3, side=12),
    "factor1": acase(transition_scale_factor=1),
    "norms_swapped": acase(first_resblock_norm="GroupRMS", second_resblock_norm="GroupLN"),
    "unfused": acase(switches=(("fuse_norm", False),)),
    "images": acase(**IMAGES),
    "images_off": acase(**{**IMAGES, "switches": (("fuse_max_cot", 0), ("norm_images", False))}),
    "images_stats_pass": acase(**{**IMAGES, "switches": (("fuse_max_cot", 0), ("tile_stats_norms", False))}),
    "factor3_images": acase(**{**IMAGES, "side": 12}, transition_scale_factor=3),
    "factor1_images": acase(**IMAGES, transition_scale_factor=1),
    "bf16x6": acase(switches=(("conv_precision", "bf16x6"),)),
    "fp32": acase(switches=(("conv_precision", "fp32"),)),
    "exact_input": acase(switches=(("exact_input_layer", True),)),
    "no_parity": acase(switches=(("upsample_parity", False),)),
    "out8": acase(output_channels=8),
    "two_levels": acase(channel_expansion=(2, 2), side=16),
    "one_each": acase(number_resnet_downward_block=1, number_resnet_upward_block=1),
    "attn1": acase(number_resnet_attn_block=1),
    "no_attn_residual": acase(attn_residual=False),
    "rows": acase(run=_adm_rows),
    "side64_images": acase(model_channels=32, side=64, switches=(("fuse_max_cot", 0),)),          # ds_conv2d_h3_up_img
    "side64_images_off": acase(side=64, switches=(("norm_images", False),)),                     # ds_conv2d_h3_up
    "cond": acase(run=_adm_cond, cls_args=(Half(),)),
    **blocks("plain"),
    **blocks("down", image_sample="downsample"),
    **blocks("up", image_sample="upsample"),
    **blocks("down3", side3=6, image_sample="downsample", image_sample_factor=3, side=12),
    **blocks("up3", image_sample="upsample", image_sample_factor=3),
    **blocks("skip_concat", channels_skip=16),
    **blocks("skip_add", channels_skip=16, skip_integration_type="add"),
    **blocks("up_skip_concat", image_sample="upsample", channels_skip=16),
    **blocks("attn", has_attn=True),
    **blocks("attn_heads2", has_attn=True, attn_heads=2),
    **blocks("attn_no_residual", has_attn=True, attn_residual=False),
    **blocks("down_fp32", image_sample="downsample", switches=(("conv_precision", "fp32"),)),
    **blocks("up_fp32", image_sample="upsample", switches=(("conv_precision", "fp32"),)),
    "block_encoder_2d": case(run=_block, family=adm_block, cls="ADMEncoderBlock", channels_in=16, channels_out=32,
                             channels_embed=8, has_downsample=True, has_residual=True),
    "block_decoder_3d": case(run=_block, family=adm_block, cls="ADMDecoderBlock", dim=3, side=4, channels_in=16, channels_out=32,
                             channels_embed=8, channels_skip=16, has_upsample=True, has_residual=True),
}
TABLES = {"net_trace": CASES, "adm_trace": ADM_CASES}                               # golden file -> its case table


def trace_of(name, cases=CASES):
    """The pinned record of one case."""
    from diffsci_amd import ops
    N = _native()
    run, pooled, kw = cases[name]
    rec = Recorder(N.lib(), pooled)
    pool = Pool(rec)
    saved = [(N, "lib", N.lib), (ops, "_stream", ops._stream), (ops, "_off_device", ops._off_device)]
    try:
        N.lib, ops._stream, ops._off_device = (lambda: rec), (lambda: 0), (lambda t: None)
        run(Net(rec, pool, **kw))
    finally:
        for mod, attr, v in saved:
            setattr(mod, attr, v)
    return {"calls": rec.calls, "pool": [pool.n, len(pool.out)], "writes": pool.writes()}
