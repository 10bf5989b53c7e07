"""VAENet first stage on HIP kernels: encoder, posterior draw and decoder, 2-D fields and 3-D volumes (reference:
diffsci/models/nets/vaenet.py, the dimension-flexible successor of the LDM AutoencoderKL).

Same constructor parameters, defaults, attribute names and state_dict keys as the reference, so its checkpoints load with
strict=True: every convolution but Downsample.conv is a ``PatchedConv`` holding its weight one level down (``....conv.weight``),
``quant_conv`` lives in the encoder and ``post_quant_conv`` in the decoder.  ``encode(x)`` returns a sampled latent tensor and
``decode(z)`` a tensor: the protocol ``KarrasModule(autoencoder=...)`` runs as given.

The blocks are the LDM launcher's (autoencoderldm.py: the folded / standalone GroupNorm routes, the 1x1 and attention launches,
the nearest-x2 loader) with the configuration's ``num_groups``; what is new here:

  Downsample with a convolution     ops.conv_s2 / ops.conv3d_s2 (ds_conv_s2.hip: stride 2, zero pad at the far end only);
                                    it leaves no tile statistics, so the next norm1 takes its statistics from a pass
  Downsample without                ops.avgpool_f(x, 2)
  Upsample                          F.interpolate(mode="area") at scale 2 is nearest x2 bit for bit: the existing loader
  the posterior draw                ops.posterior_sample (in-kernel Philox, or a recorded eps)

``patch_size`` is accepted and ignored (patching changes the reference's memory use, not its values); ``use_flash_attention``
selects between two formulations of the same softmax attention there and nothing here.  Not built: dimension=1, time
embeddings, minimal_rf_mode, linear attention (NotImplementedError at construction).  ``calculate_receptive_field`` of the
encoder, the decoder and the net return the reference's dicts; the chunked volume decode that reads them is
diffsci_amd/extra/chunk_decode.py."""
import pathlib
from typing import List

import torch
import yaml

from ... import ops
from . import autoencoderldm as L
from .autoencoderldm import EPS, _Launcher


class VAENetConfig:
    """Configuration class for dimensionally-flexible VAE architecture (vaenet.py:15-110)."""

    def __init__(
        self,
        dimension: int = 3,
        in_channels: int = 1,
        out_channels: int = 1,
        z_channels: int = 4,
        z_dim: int = 4,
        ch: int = 32,
        ch_mult: List[int] = [1, 2, 4],
        num_res_blocks: int = 2,
        attn_resolutions: List[int] = [],
        dropout: float = 0.0,
        resolution: int = 64,
        has_mid_attn: bool = True,
        resamp_with_conv: bool = True,
        attn_type: str = "vanilla",
        tanh_out: bool = False,
        input_bias: bool = True,
        output_bias: bool = True,
        with_time_emb: bool = False,
        double_z: bool = True,
        num_groups: int = 32,
        patch_size: int = None,
        memory_efficient_variant: bool = False,
        use_flash_attention: bool = True,
        minimal_rf_mode: bool = False,
    ):
        assert dimension in [1, 2, 3], f"Dimension must be 1, 2, or 3, got {dimension}"
        self.dimension = dimension
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.z_channels = z_channels
        self.z_dim = z_dim
        self.ch = ch
        self.ch_mult = ch_mult
        self.num_res_blocks = num_res_blocks
        self.attn_resolutions = attn_resolutions
        self.dropout = dropout
        self.resolution = resolution
        self.has_mid_attn = has_mid_attn
        self.resamp_with_conv = resamp_with_conv
        self.attn_type = attn_type
        self.tanh_out = tanh_out
        self.input_bias = input_bias
        self.output_bias = output_bias
        self.with_time_emb = with_time_emb
        self.double_z = double_z
        self.num_resolutions = len(self.ch_mult)
        self.num_groups = num_groups
        self.patch_size = patch_size
        self.memory_efficient_variant = memory_efficient_variant
        self.use_flash_attention = use_flash_attention
        self.minimal_rf_mode = minimal_rf_mode

    _FIELDS = ("dimension", "in_channels", "out_channels", "z_channels", "z_dim", "ch", "ch_mult", "num_res_blocks",
               "attn_resolutions", "dropout", "resolution", "has_mid_attn", "resamp_with_conv", "attn_type", "tanh_out",
               "input_bias", "output_bias", "with_time_emb", "double_z", "num_groups", "patch_size",
               "memory_efficient_variant", "use_flash_attention", "minimal_rf_mode")

    def export_description(self) -> dict:
        return {name: getattr(self, name) for name in self._FIELDS}

    @classmethod
    def from_description(cls, description: dict):
        return cls(**description)

    @classmethod
    def from_config_file(cls, config_file: pathlib.Path | str):
        with open(config_file, "r") as f:
            return cls.from_description(yaml.safe_load(f))


def _conv_cls(dimension):
    if dimension == 1:
        raise NotImplementedError("dimension=1 is not implemented on the HIP path: VAENet runs fields (2) and volumes (3)")
    if dimension not in (2, 3):
        raise ValueError(f"Unsupported dimension: {dimension}")
    return torch.nn.Conv3d if dimension == 3 else torch.nn.Conv2d


def _refuse_config(config):
    """The reference options without a HIP route, named in the message."""
    _conv_cls(config.dimension)
    if config.with_time_emb:
        raise NotImplementedError("with_time_emb=True is outside the HIP sampling path: KarrasModule calls the first stage "
                                  "without a time")
    if config.minimal_rf_mode:
        raise NotImplementedError("minimal_rf_mode=True (MinimalResnetBlock) is not implemented on the HIP path")
    if config.attn_type == "linear":
        raise NotImplementedError("attn_type='linear' is not implemented on the HIP path: use 'vanilla' or 'none'")
    if config.attn_type not in ("vanilla", "none"):
        raise AssertionError(f"attn_type {config.attn_type} unknown")


def _refuse_time(time):
    if time is not None:
        raise NotImplementedError("a time argument (with_time_emb) is outside the HIP sampling path: call with time=None")


class PatchedConv(torch.nn.Module):
    """vaenet.py:189-249 as a parameter container: the weight lives in the child ``conv`` (built with padding=0, as the
    reference's: the launches pad), ``weight`` / ``bias`` are what the launcher reads.  patch_size is kept and unused."""

    def __init__(self, in_channels: int, out_channels: int, patch_size: int | None = None, kernel_size: int = 3, stride: int = 1,
                 padding: int | None = None, bias: bool = True, dimension: int = 3):
        super().__init__()
        assert kernel_size % 2 == 1, f"Kernel size must be odd, got {kernel_size}"
        assert stride == 1, f"Only implemented for stride == 1, got {stride}"
        assert padding is None or padding == kernel_size // 2, f"Padding must be kernel_size//2, got {padding}"
        if kernel_size not in (1, 3):
            raise NotImplementedError(f"kernel_size={kernel_size}: VAENet's convolutions are 1x1 and 3x3")
        self.padding = padding if padding is not None else kernel_size // 2
        self.dimension = dimension
        self.kernel_size = kernel_size
        self.conv = _conv_cls(dimension)(in_channels, out_channels, kernel_size, padding=0, bias=bias)
        self.patch_size = patch_size

    @classmethod
    def initialize_with_dimension(cls, dimension: int):
        import functools
        return functools.partial(cls, dimension=dimension)

    @property
    def weight(self):
        return self.conv.weight

    @property
    def bias(self):
        return self.conv.bias

    @property
    def in_channels(self):
        return self.conv.in_channels

    @property
    def out_channels(self):
        return self.conv.out_channels

    def forward(self, x):
        raise NotImplementedError("PatchedConv is a parameter container: the blocks launch its convolution (ops.conv / ops.conv3d*)")


def get_norm(in_channels, num_groups=32):
    return torch.nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=EPS, affine=True)


class ResnetBlock(L.ResnetBlock):
    """vaenet.py:266-325; the LDM block's launches with num_groups groups."""

    def __init__(self, *, dimension, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=0, num_groups=32,
                 patch_size=None):
        torch.nn.Module.__init__(self)
        Conv = PatchedConv.initialize_with_dimension(dimension)
        _conv_cls(dimension)
        self._dim = dimension
        self.dimension = dimension
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        self.patch_size = patch_size
        self.norm1 = get_norm(in_channels, num_groups=num_groups)
        self.conv1 = Conv(in_channels, out_channels, kernel_size=3, stride=1, padding=1, patch_size=patch_size)
        if temb_channels > 0:
            self.temb_proj = torch.nn.Linear(temb_channels, out_channels)
        self.norm2 = get_norm(out_channels, num_groups=num_groups)
        self.dropout = torch.nn.Dropout(dropout)
        self.conv2 = Conv(out_channels, out_channels, kernel_size=3, stride=1, padding=1, patch_size=patch_size)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = Conv(in_channels, out_channels, kernel_size=3, stride=1, padding=1, patch_size=patch_size)
            else:
                self.nin_shortcut = Conv(in_channels, out_channels, kernel_size=1, stride=1, padding=0, patch_size=patch_size)
        self._init_launcher(num_groups)


class AttnBlock(L.AttnBlock):
    """vaenet.py:417-537: both of the reference's formulations are softmax(q^T k * C**-0.5) v, the launcher's attention."""

    def __init__(self, dimension, in_channels, num_groups=32, patch_size=None, use_flash_attention=True):
        torch.nn.Module.__init__(self)
        Conv = PatchedConv.initialize_with_dimension(dimension)
        _conv_cls(dimension)
        self._dim = dimension
        self.dimension = dimension
        self.in_channels = in_channels
        self.patch_size = patch_size
        self.use_flash_attention = use_flash_attention
        self.norm = get_norm(in_channels, num_groups=num_groups)
        self.q = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0, patch_size=patch_size)
        self.k = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0, patch_size=patch_size)
        self.v = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0, patch_size=patch_size)
        self.proj_out = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0, patch_size=patch_size)
        self.scale = in_channels ** -0.5
        self._init_launcher(num_groups)


def make_attn(dimension, in_channels, attn_type="vanilla", num_groups=32, patch_size=None, use_flash_attention=True):
    assert attn_type in ["vanilla", "linear", "none"], f'attn_type {attn_type} unknown'
    if attn_type == "linear":
        raise NotImplementedError("attn_type='linear' is not implemented on the HIP path: use 'vanilla' or 'none'")
    if attn_type == "none":
        return torch.nn.Identity()
    return AttnBlock(dimension, in_channels, num_groups=num_groups, patch_size=patch_size, use_flash_attention=use_flash_attention)


class Upsample(L.Upsample):
    """vaenet.py:620-644: interpolate(scale_factor=2, mode="area") repeats every element twice per axis -- nearest x2 -- then
    the 3x3 convolution when with_conv, the upsampling in its loader."""

    def __init__(self, dimension, in_channels, with_conv, patch_size=None):
        torch.nn.Module.__init__(self)
        _conv_cls(dimension)
        self._dim = dimension
        self.dimension = dimension
        self.with_conv = with_conv
        self.patch_size = patch_size
        self.in_channels = in_channels
        if self.with_conv:
            self.conv = PatchedConv(in_channels, in_channels, kernel_size=3, stride=1, padding=1, patch_size=patch_size,
                                    dimension=dimension)
        self._init_launcher()


def _check_downsample_sides(x, rank, channels, levels, what):
    """ValueError before any launch when one of `levels` successive halvings meets a side below 2 (the reference's
    convolution / pooling fails there too).  A wrong rank or channel count is _check's to report."""
    if not isinstance(x, torch.Tensor) or x.dim() != rank or x.shape[1] != channels:
        return
    spatial = x.shape[2:]
    sides = [int(s) for s in spatial]
    for _ in range(levels):
        if min(sides) < 2:
            raise ValueError(f"{what}: a Downsample needs spatial sides of at least 2; input {tuple(int(s) for s in spatial)} "
                             f"reaches {tuple(sides)}")
        sides = [s // 2 for s in sides]


class Downsample(_Launcher):
    """vaenet.py:647-682: pad (0, 1) per spatial axis + Conv(k=3, stride=2, padding=0) -- one stride-2 launch (fields) or its
    depth-tap composition (volumes) -- or AvgPool(2).  The plain convolution keeps its reference key (conv.weight)."""

    def __init__(self, dimension, in_channels, with_conv, patch_size=None):
        super().__init__()
        Conv = _conv_cls(dimension)
        self._dim = dimension
        self.dimension = dimension
        self.with_conv = with_conv
        self.patch_size = patch_size
        self.in_channels = in_channels
        if self.with_conv:
            self.conv = Conv(in_channels, in_channels, kernel_size=3, stride=2, padding=0)
        self._init_launcher()

    def _run(self, x, xs=None):
        if not self.with_conv:
            return ops.avgpool_f(x, 2), None
        w = self.conv.weight.detach()
        if self._dim == 2:
            pk = self._cached("conv", (self.conv.weight,), lambda: ops.pack_conv_s2(w, self.conv_precision))
            return ops.conv_s2(x, pk, bias=self.conv.bias), None
        packs = self._cached("conv", (self.conv.weight,), lambda: ops.pack_conv3d_s2(w, self.conv_precision))
        return ops.conv3d_s2(x, packs, bias=self.conv.bias), None

    @ops.device_guard
    def forward(self, x):
        _check_downsample_sides(x, 2 + self._dim, self.in_channels, 1, "Downsample")
        x = self._check(x, self.in_channels, "Downsample")
        return self._run(x)[0]


def _attend(att, h, hs):
    return att._run(h, hs) if isinstance(att, L.AttnBlock) else (h, hs)          # Identity for attn_type "none"


def _hand_down(root):
    for m in root.modules():
        if isinstance(m, _Launcher) and m is not root:
            m.conv_precision, m.fuse_norm = root.conv_precision, root.fuse_norm


def _has_attention(config):
    """An attention block sees the whole volume; attn_type "none" builds Identity in its place."""
    return config.attn_type != "none" and bool(config.has_mid_attn or len(config.attn_resolutions) > 0)


def _rf_per_block(config):
    return 2 if getattr(config, "minimal_rf_mode", False) else 4          # two 3x3 convolutions, or MinimalResnetBlock's one


def _rf_mode(config):
    return "minimal" if getattr(config, "minimal_rf_mode", False) else "standard"


def _grow(trace, rf, by, what):
    trace.append(f"{what}: RF = {rf + by}")
    return rf + by


def decoder_receptive_field(cfg):
    """vaenet.py:1142-1228: the receptive field in latent cells after every piece of the walk -- what a tiled decode sizes
    its halos from (extra/chunk_decode.py) -- or the infinite case when an attention block is configured."""
    if _has_attention(cfg):
        return {"rf_latent": float("inf"), "has_attention": True, "feasible_chunking": False,
                "reason": "Decoder uses global attention"}
    per_block = _rf_per_block(cfg)
    trace = ["post_quant_conv (1x1): RF = 1"]
    rf = _grow(trace, 1, 2, "conv_in (3x3)")
    rf = _grow(trace, rf, per_block, "mid.block_1")
    rf = rf_mid = _grow(trace, rf, per_block, "mid.block_2")
    blocks = cfg.num_res_blocks + 1
    for i_level in reversed(range(cfg.num_resolutions)):
        rf = _grow(trace, rf, blocks * per_block, f"up[{i_level}] ({blocks} blocks)")
        if i_level != 0:
            trace.append(f"up[{i_level}].upsample (no RF change in latent coords)")
    rf = _grow(trace, rf, 2, "conv_out (3x3)")
    overlap = int(rf * 1.5)                       # the reference's suggestion: 1.5 rf, up to 16 / 24 / 32 / a multiple of 16
    overlap = next((n for n in (16, 24, 32) if overlap <= n), -(-overlap // 16) * 16)
    factor = 2 ** (cfg.num_resolutions - 1)
    return {"rf_latent": rf, "rf_after_middle": rf_mid, "rf_output": rf * factor, "min_overlap": rf,
            "recommended_overlap": overlap, "spatial_upsampling_factor": factor, "has_attention": False,
            "feasible_chunking": True, "trace": trace, "rf_per_block": per_block, "mode": _rf_mode(cfg),
            "num_convolutions": sum("RF" in t and "no RF" not in t for t in trace)}


class VAEEncoder(_Launcher):
    """vaenet.py:685-876.  conv_precision / fuse_norm are read at every forward and handed down, as on the LDM Decoder."""

    def __init__(self, config: VAENetConfig):
        super().__init__()
        _refuse_config(config)
        self.config = config
        self.dimension = self._dim = config.dimension
        self.patch_size = config.patch_size
        Conv = PatchedConv.initialize_with_dimension(config.dimension)
        self.temb_ch = 0
        kw = dict(dimension=config.dimension, temb_channels=self.temb_ch, dropout=config.dropout, num_groups=config.num_groups,
                  patch_size=config.patch_size)
        akw = dict(attn_type=config.attn_type, num_groups=config.num_groups, patch_size=config.patch_size,
                   use_flash_attention=config.use_flash_attention)
        self.conv_in = Conv(config.in_channels, config.ch, kernel_size=3, stride=1, padding=1, bias=config.input_bias,
                            patch_size=config.patch_size)
        curr_res = config.resolution
        block_in = config.ch
        self.down = torch.nn.ModuleList()
        for i_level in range(config.num_resolutions):
            block, attn = torch.nn.ModuleList(), torch.nn.ModuleList()
            block_out = config.ch * config.ch_mult[i_level]
            for _ in range(config.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, **kw))
                block_in = block_out
                if curr_res in config.attn_resolutions:
                    attn.append(make_attn(config.dimension, block_in, **akw))
            down = torch.nn.Module()
            down.block, down.attn = block, attn
            if i_level != config.num_resolutions - 1:
                down.downsample = Downsample(config.dimension, block_in, config.resamp_with_conv, patch_size=config.patch_size)
                curr_res = curr_res // 2
            self.down.append(down)
        self.mid = torch.nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, **kw)
        if config.has_mid_attn:
            self.mid.attn_1 = make_attn(config.dimension, block_in, **akw)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, **kw)
        z_channels = 2 * config.z_channels if config.double_z else config.z_channels
        self.norm_out = get_norm(block_in, num_groups=config.num_groups)
        self.conv_out = Conv(block_in, z_channels, kernel_size=3, stride=1, padding=1, bias=True, patch_size=config.patch_size)
        self.quant_conv = Conv(z_channels, 2 * config.z_dim, kernel_size=1, patch_size=config.patch_size)
        self._init_launcher(config.num_groups)

    @ops.device_guard
    def forward(self, x, time=None):
        cfg = self.config
        _refuse_time(time)
        if self.training and cfg.dropout > 0:
            raise NotImplementedError("dropout > 0 in training mode is outside the HIP sampling path: call .eval()")
        _check_downsample_sides(x, 2 + self._dim, cfg.in_channels, cfg.num_resolutions - 1, "VAEEncoder")
        x = self._check(x, cfg.in_channels, "VAEEncoder")
        _hand_down(self)
        B, dev = x.shape[0], x.device
        hs = self._tiles(B, cfg.ch, x.shape[2:], dev)
        h = self._conv3("conv_in", self.conv_in, x, tile_stats=hs)
        for i_level in range(cfg.num_resolutions):
            down = self.down[i_level]
            for i_block in range(cfg.num_res_blocks):
                h, hs = down.block[i_block]._run(h, hs)
                if len(down.attn) > i_block:
                    h, hs = _attend(down.attn[i_block], h, hs)
            if i_level != cfg.num_resolutions - 1:
                h, hs = down.downsample._run(h, hs)
        h, hs = self.mid.block_1._run(h, hs)
        if hasattr(self.mid, "attn_1"):
            h, hs = _attend(self.mid.attn_1, h, hs)
        h, hs = self.mid.block_2._run(h, hs)
        h = self._norm_swish_conv("conv_out", self.norm_out, self.conv_out, h, hs)
        m = self.quant_conv
        return self._conv1("quant_conv", (m.weight,), (m.bias,), self._v4(h)).view((B, m.out_channels) + tuple(h.shape[2:]))

    def calculate_receptive_field(self):
        """vaenet.py:878-945: the receptive field in input cells (3x3 convolutions add 2, a block 4, a strided convolution 2, a
        pooling 1, each counted at full resolution as the reference does), and that over the downsampling factor."""
        cfg = self.config
        if _has_attention(cfg):
            return {"rf_input": float("inf"), "rf_latent": float("inf"), "has_attention": True, "feasible_chunking": False}
        per_block = _rf_per_block(cfg)
        trace = []
        rf = _grow(trace, 1, 2, "conv_in")
        stride = 1
        for i_level in range(cfg.num_resolutions):
            rf = _grow(trace, rf, cfg.num_res_blocks * per_block, f"down[{i_level}] ({cfg.num_res_blocks} blocks)")
            if i_level != cfg.num_resolutions - 1:
                rf = _grow(trace, rf, 2 if cfg.resamp_with_conv else 1, f"down[{i_level}].downsample")
                stride *= 2
        rf = _grow(trace, rf, 2 * per_block, "mid blocks")
        rf = _grow(trace, rf, 2, "conv_out")
        return {"rf_input": rf, "rf_latent": rf // stride, "downsampling_factor": stride, "has_attention": False,
                "feasible_chunking": True, "trace": trace, "rf_per_block": per_block, "mode": _rf_mode(cfg)}


class VAEDecoder(L.Decoder):
    """vaenet.py:948-1140: post_quant_conv, then the LDM decoder's walk.  memory_efficient_variant only changes the channel
    counts of the levels."""

    def __init__(self, config: VAENetConfig):
        torch.nn.Module.__init__(self)
        _refuse_config(config)
        self.config = config
        self.dimension = self._dim = config.dimension
        self.patch_size = config.patch_size
        Conv = PatchedConv.initialize_with_dimension(config.dimension)
        self.temb_ch = 0
        kw = dict(dimension=config.dimension, temb_channels=self.temb_ch, dropout=config.dropout, num_groups=config.num_groups,
                  patch_size=config.patch_size)
        akw = dict(attn_type=config.attn_type, num_groups=config.num_groups, patch_size=config.patch_size,
                   use_flash_attention=config.use_flash_attention)
        self.post_quant_conv = Conv(config.z_dim, config.z_channels, kernel_size=1, patch_size=config.patch_size)
        self.num_resolutions = len(config.ch_mult)
        self.min_res = config.resolution // (2 ** (self.num_resolutions - 1))
        curr_res = self.min_res
        block_in = config.ch * config.ch_mult[-1]
        self.conv_in = Conv(config.z_channels, block_in, kernel_size=3, stride=1, padding=1, bias=config.input_bias,
                            patch_size=config.patch_size)
        self.mid = torch.nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, **kw)
        if config.has_mid_attn:
            self.mid.attn_1 = make_attn(config.dimension, block_in, **akw)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, **kw)
        self.up = torch.nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block, attn = torch.nn.ModuleList(), torch.nn.ModuleList()
            if config.memory_efficient_variant and i_level != 0:
                block_out = config.ch * config.ch_mult[i_level - 1]
            else:
                block_out = config.ch * config.ch_mult[i_level]
            for _ in range(config.num_res_blocks + 1):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, **kw))
                block_in = block_out
                if curr_res in config.attn_resolutions:
                    attn.append(make_attn(config.dimension, block_in, **akw))
            up = torch.nn.Module()
            up.block, up.attn = block, attn
            if i_level != 0:
                up.upsample = Upsample(config.dimension, block_in, config.resamp_with_conv, patch_size=config.patch_size)
                curr_res = curr_res * 2
            self.up.insert(0, up)
        self.norm_out = get_norm(block_in, num_groups=config.num_groups)
        self.conv_out = Conv(block_in, config.out_channels, kernel_size=3, stride=1, padding=1, bias=config.output_bias,
                             patch_size=config.patch_size)
        # what the LDM decoder's walk reads
        self.__dict__.update(z_channels=config.z_channels, dropout=config.dropout, has_mid_attn=config.has_mid_attn,
                             num_res_blocks=config.num_res_blocks, give_pre_end=False, tanh_out=config.tanh_out)
        self._init_launcher(config.num_groups)

    def _stage0(self, z):
        """post_quant_conv, then the LDM decoder's stage 0."""
        m = self.post_quant_conv
        h = self._conv1("post_quant_conv", (m.weight,), (m.bias,), self._v4(z))
        return L.Decoder._stage0(self, h.view((z.shape[0], m.out_channels) + tuple(z.shape[2:])))

    @ops.device_guard
    def forward(self, z, time=None):
        _refuse_time(time)
        if self.training and self.config.dropout > 0:
            raise NotImplementedError("dropout > 0 in training mode is outside the HIP sampling path: call .eval()")
        return self._walk(self._check(z, self.config.z_dim, "VAEDecoder"))

    def calculate_receptive_field(self):
        return decoder_receptive_field(self.config)


class VAENet(torch.nn.Module):
    """vaenet.py:1231-1265.  ``conv_precision`` ("fp16x3" | "bf16x6" | "fp32") and ``fuse_norm`` switch both halves, as on
    the LDM Decoder.  ``eps`` of encode is the one extension: a recorded draw [B, z_dim, ...] instead of in-kernel noise."""

    def __init__(self, config: VAENetConfig):
        super().__init__()
        _refuse_config(config)
        self.config = config
        self.encoder = VAEEncoder(config)
        self.decoder = VAEDecoder(config)
        self.conv_precision = "fp16x3"
        self.fuse_norm = True

    def _switches(self):
        for half in (self.encoder, self.decoder):
            half.conv_precision, half.fuse_norm = self.conv_precision, self.fuse_norm

    def encode(self, x, time=None, sample=True, eps=None):
        """The moments [B, 2 z_dim, ...] (sample=False) or mean + exp(0.5 logvar) * noise."""
        self._switches()
        moments = self.encoder(x, time)
        if not sample:
            return moments
        with ops.on_device_of(moments):
            return ops.posterior_sample(moments, eps)

    def decode(self, z, time=None):
        self._switches()
        return self.decoder(z, time)

    def forward(self, x, time=None):
        moments = self.encode(x, time)
        return moments, self.decode(moments[:, :self.config.z_dim].contiguous(), time)

    def export_description(self) -> dict:
        return {"config": self.config.export_description()}

    def calculate_receptive_field(self):
        """vaenet.py:1267-1286: both halves' fields and the configuration entries they follow from."""
        cfg = self.config
        return {"encoder": self.encoder.calculate_receptive_field(), "decoder": self.decoder.calculate_receptive_field(),
                "config": {"minimal_rf_mode": getattr(cfg, "minimal_rf_mode", False), "num_res_blocks": cfg.num_res_blocks,
                           "ch_mult": cfg.ch_mult, "has_mid_attn": cfg.has_mid_attn, "attn_type": cfg.attn_type,
                           "attn_resolutions": cfg.attn_resolutions}}

    def print_receptive_field_summary(self):
        """calculate_receptive_field() as text."""
        info, cfg = self.calculate_receptive_field(), self.config
        enc, dec = info["encoder"], info["decoder"]
        print(f"VAENet receptive fields ({cfg.dimension}-D, ch_mult {cfg.ch_mult}, num_res_blocks {cfg.num_res_blocks}, "
              f"has_mid_attn {cfg.has_mid_attn}, attn_type {cfg.attn_type!r}, {_rf_mode(cfg)} blocks)")
        if enc["has_attention"]:
            print("  encoder: global attention, the field is unbounded")
        else:
            print(f"  encoder: {enc['rf_input']} input cells = {enc['rf_latent']} latent cells "
                  f"(downsampling x{enc['downsampling_factor']})")
        if dec["has_attention"]:
            print("  decoder: global attention, the field is unbounded: a chunked decode is not feasible")
        else:
            print(f"  decoder: {dec['rf_latent']} latent cells ({dec['rf_after_middle']} after the middle blocks) = "
                  f"{dec['rf_output']} output cells (upsampling x{dec['spatial_upsampling_factor']})")
            print(f"  chunked decode: feasible; overlap at least {dec['min_overlap']} latent cells, suggested "
                  f"{dec['recommended_overlap']}")
