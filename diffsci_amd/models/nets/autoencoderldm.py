"""LDM AutoencoderKL decoder on HIP kernels, 2-D fields and 3-D volumes (reference: diffsci/models/nets/autoencoderldm2d.py
and autoencoderldm3d.py, the latent-diffusion first stage).  One implementation; ``autoencoderldm2d`` / ``autoencoderldm3d``
bind it to a dimension and carry the public names.

Decode half only: ``Decoder``, its blocks, and ``AutoencoderKL.decode`` -- what ``KarrasModule.sample(..., is_latent_shape=True)``
needs after its last step.  Same constructor parameters, attribute names and state_dict keys as the reference, so its latent
checkpoints load.  The torch.nn layers are parameter containers; every tensor operation of a forward is a launch into
libdiffsci_hip.so, eager (one call per run):

  conv_in / conv1 / conv2 / conv_shortcut / conv_out      ds_conv2d* (fields), ops.conv3d_mfma / ds_conv3d_direct (volumes)
  nin_shortcut, q | k | v (one packed launch), proj_out    ds_conv1x1_h3 / ds_conv2d (volumes as [B, C, D*H, W])
  Upsample                                                 the convolution's nearest-x2 loader; ds_upsample_f without a convolution
  GroupNorm(32, C) (+ swish)                               ds_groupnorm_stats + ds_groupnorm_apply, or folded (below)
  attention over the flattened positions                   ds_attention* (logits * C**-0.5)
  residual adds                                            res1 of the convolution's epilogue
  tanh_out                                                 ds_add_act

Norm routes (attribute ``fuse_norm``, as ADM's).  Folded, 2-D at conv_precision "fp16x3": a norm followed by swish and a 3x3
convolution (norm1, norm2, norm_out) never reaches HBM -- the producing convolution leaves tile statistics, ds_groupnorm_table
turns them into the consumer's loader table (with the sample's activation exponent), and the consumer normalises while it stages
its input; AttnBlock's norm takes its statistics from the tiles and is applied by ds_groupnorm_apply.  Standalone, everywhere else
and with ``fuse_norm = False``: statistics pass, apply pass (which also leaves the per-sample max |.| for the consumer's exponent),
convolution."""
import torch

from ... import ops
from ..._native import DS_LOAD_PLAIN, DS_LOAD_UPSAMPLE2
from . import runtime

NUM_GROUPS = 32
EPS = 1e-6
ENCODER_MESSAGE = ("the encoder (Encoder, quant_conv, the posterior) is outside the HIP sampling path: this AutoencoderKL decodes "
                   "only, and sample(..., is_latent_shape=True) needs no encoder")


def Normalize(in_channels, num_groups=NUM_GROUPS):
    """GroupNorm(32, C), eps 1e-6, affine: the parameter container; raises ValueError as torch does when 32 does not divide C."""
    return torch.nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=EPS, affine=True)


DDCONFIG_FIELDS = ("double_z", "z_channels", "resolution", "in_channels", "out_ch", "ch", "ch_mult", "num_res_blocks",
                   "attn_resolutions", "dropout", "has_mid_attn")


def set_ddconfig(cfg, given):
    """The body of the two modules' ddconfig.__init__ (autoencoderldm2d.py:228-251 / autoencoderldm3d.py:258-281): their signatures
    differ in the default resolution, so each module writes its own and hands its locals() here."""
    for name in DDCONFIG_FIELDS:
        setattr(cfg, name, given[name])


class _Launcher(torch.nn.Module):
    """What the blocks share: the dimension, the kernel switches, the GroupNorm group count (32 in the LDM modules; VAENet's
    blocks set their configuration's) and the packed weights (repacked when a weight, the device or conv_precision changes)."""
    _dim = 2

    def _init_launcher(self, num_groups=NUM_GROUPS):
        self.conv_precision = "fp16x3"
        self.fuse_norm = True
        self.num_groups = num_groups
        self.__dict__["_packs"] = {}

    def _conv_cls(self):
        return torch.nn.Conv3d if self._dim == 3 else torch.nn.Conv2d

    def _folds(self):
        return bool(self.fuse_norm) and self.conv_precision == "fp16x3" and self._dim == 2

    def _cached(self, name, tensors, make):
        sig = runtime.weights_signature(tensors, self.conv_precision)
        hit = self._packs.get(name)
        if hit is None or hit[0] != sig:
            with torch.no_grad():
                hit = self._packs[name] = (sig, make())
        return hit[1]

    def _check(self, x, channels, what):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 + self._dim:
            raise ValueError(f"{what} takes {2 + self._dim}-D tensors [B, C, {'D, ' if self._dim == 3 else ''}H, W]; got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        if x.shape[1] != channels:
            raise ValueError(f"{what} expects {channels} channels; got {x.shape[1]}")
        if self.conv_precision not in ops.CONV_PRECISIONS:
            raise ValueError(f"unknown conv_precision {self.conv_precision!r}; choose from {ops.CONV_PRECISIONS}")
        ops.require_device(x, "x")
        return x.contiguous()

    @staticmethod
    def _v4(t):                                      # the 1x1 convolutions and the attention see volumes as [B, C, D*H, W]
        return t if t.dim() == 4 else t.view(t.shape[0], t.shape[1], -1, t.shape[-1])

    def _conv3(self, name, m, x, up=False, res1=None, prenorm=None, tile_stats=None, in_amax=None):
        """3x3(x3) 'same' convolution, with the nearest x2 upsampling in its loader when up."""
        mode = DS_LOAD_UPSAMPLE2 if up else DS_LOAD_PLAIN
        w = m.weight.detach()
        if self._dim == 2:
            pk = self._cached(name, (m.weight,), lambda: ops.pack_conv(w, self.conv_precision, upsampled=up))
            kw = dict(in_amax=in_amax) if pk.kind == "fp16x3" else {}
            return ops.conv(x, pk, bias=m.bias, load_mode=mode, res1=res1, prenorm=prenorm, tile_stats=tile_stats, **kw)
        if self.conv_precision == "fp16x3" and min(w.shape[0], w.shape[1]) > 4:
            packs = self._cached(name, (m.weight,), lambda: ops.pack_conv3d(w, upsampled=up))
            return ops.conv3d_mfma(x, packs, bias=m.bias, load_mode=mode, res1=res1)
        return ops.conv3d(x, m.weight, bias=m.bias, load_mode=mode, res1=res1)       # thin layers / exact fp32

    def _pack1(self, name, weights, biases):
        """(packing, bias) of the 1x1(x1) convolution by the row-wise concatenation of `weights`."""
        prec = "fp16x3" if self.conv_precision == "fp16x3" else "fp32"

        def make():
            w = torch.cat([t.detach().reshape(t.shape[0], t.shape[1], 1, 1) for t in weights], dim=0).contiguous()
            return ops.pack_conv(w, prec), torch.cat([t.detach() for t in biases]).contiguous()
        return self._cached(name, tuple(weights) + tuple(biases), make)

    def _conv1(self, name, weights, biases, x, res1=None, tile_stats=None, **amax):
        """That convolution of x [B, C, (D*)H, W]."""
        pk, bias = self._pack1(name, weights, biases)
        kw = amax if pk.kind == "fp16x3" else {}
        return ops.conv(x, pk, bias=bias, res1=res1, tile_stats=tile_stats, **kw)

    def _tiles(self, B, C, spatial, device):
        """A tile-statistics buffer for a [B, C, H, W] convolution output on the folded route, else None."""
        if not self._folds():
            return None
        return torch.empty((B, C, ops.conv_tile_count(*spatial), 4), dtype=torch.float32, device=device)

    def _norm_swish_conv(self, name, norm, conv, x, xs, res1=None, tile_stats=None):
        """conv(swish(norm(x))) [+ res1]; xs: the tile statistics x's producer left, or None."""
        count = x.numel() // (x.shape[0] * x.shape[1])
        G = self.num_groups
        if self._folds():
            tab = (ops.groupnorm_table(norm.weight, norm.bias, G, count, tile_stats=xs, eps=EPS) if xs is not None else
                   ops.groupnorm_table(norm.weight, norm.bias, G, count, stats=ops.groupnorm_stats(x, G, EPS), eps=EPS))
            return self._conv3(name, conv, x, res1=res1, prenorm=tab, tile_stats=tile_stats)
        st = ops.groupnorm_stats(x, G, EPS)
        am = ops.amax_new(x.shape[0], x.device) if (self._dim == 2 and self.conv_precision == "fp16x3") else None
        a = ops.groupnorm_apply(x, st, norm.weight, norm.bias, G, act=True, out_amax=am)
        return self._conv3(name, conv, a, res1=res1, in_amax=am)


class ResnetBlock(_Launcher):
    """autoencoderldm2d.py:29-88: norm1 -> swish -> conv1 -> norm2 -> swish -> conv2, plus x (through nin_shortcut / conv_shortcut
    when the channel count changes).  The decoder runs it with temb=None; a time embedding and active dropout are refused."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        Conv = self._conv_cls()
        self.norm1 = Normalize(in_channels)
        self.conv1 = Conv(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if temb_channels > 0:
            self.temb_proj = torch.nn.Linear(temb_channels, out_channels)
        self.norm2 = Normalize(out_channels)
        self.dropout = torch.nn.Dropout(dropout)
        self.conv2 = Conv(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = Conv(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = Conv(in_channels, out_channels, kernel_size=1, stride=1, padding=0)
        self._init_launcher()

    def _refuse(self, temb):
        if temb is not None:
            raise NotImplementedError("ResnetBlock with a time embedding (temb is not None) is outside the decoder's sampling "
                                      "path: the LDM decoder calls its blocks with temb=None")
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("dropout > 0 in training mode is outside the HIP sampling path: call .eval()")

    def _run(self, x, xs=None):
        B, Co, dev = x.shape[0], self.out_channels, x.device
        ys = self._tiles(B, Co, x.shape[2:], dev)
        y = self._norm_swish_conv("conv1", self.norm1, self.conv1, x, xs, tile_stats=ys)
        r = x
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                r = self._conv3("conv_shortcut", self.conv_shortcut, x)
            else:
                m = self.nin_shortcut
                r = self._conv1("nin_shortcut", (m.weight,), (m.bias,), self._v4(x)).view((B, Co) + tuple(x.shape[2:]))
        os_ = self._tiles(B, Co, x.shape[2:], dev)
        return self._norm_swish_conv("conv2", self.norm2, self.conv2, y, ys, res1=r, tile_stats=os_), os_

    @ops.device_guard
    def forward(self, x, temb=None):
        self._refuse(temb)
        return self._run(self._check(x, self.in_channels, "ResnetBlock"))[0]


class AttnBlock(_Launcher):
    """autoencoderldm2d.py:123-174: x + proj_out(softmax(q^T k * C**-0.5) applied to v) over the flattened positions of norm(x)."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        Conv = self._conv_cls()
        self.norm = Normalize(in_channels)
        self.q = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = Conv(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self._init_launcher()

    def _run(self, x, xs=None):
        B, C = x.shape[0], self.in_channels
        L = x.numel() // (B * C)
        h3 = self.conv_precision == "fp16x3"
        G = self.num_groups
        st = (ops.groupnorm_stats_tiles(xs, G, L, EPS) if (xs is not None and self._folds())
              else ops.groupnorm_stats(x, G, EPS))
        a_in = ops.amax_new(B, x.device) if h3 else None
        hn = ops.groupnorm_apply(x, st, self.norm.weight, self.norm.bias, G, act=False, out_amax=a_in)
        w_in, b_in = self._pack1("qkv", (self.q.weight, self.k.weight, self.v.weight), (self.q.bias, self.k.bias, self.v.bias))
        w_out, b_out = self._pack1("proj_out", (self.proj_out.weight,), (self.proj_out.bias,))
        x4 = self._v4(x)
        os_ = self._tiles(B, C, x.shape[2:], x.device)
        out = runtime.attention(self._v4(hn), w_in, b_in, w_out, b_out, E=C, heads=1, precision=self.conv_precision,
                                in_amax=a_in, res1=x4, tile_stats=os_)                            # one head: logits / sqrt(C)
        return out.view(x.shape), os_

    @ops.device_guard
    def forward(self, x):
        return self._run(self._check(x, self.in_channels, "AttnBlock"))[0]


def make_attn(cls, in_channels, attn_type="vanilla"):
    """autoencoderldm2d.py:177-185 without the print; linear attention is not built."""
    if attn_type not in ("vanilla", "linear", "none"):
        raise AssertionError(f"attn_type {attn_type} unknown")
    if attn_type == "linear":
        raise NotImplementedError("attn_type='linear' (use_linear_attn=True) is not implemented on the HIP path: "
                                  "use 'vanilla' or 'none'")
    return cls(in_channels) if attn_type == "vanilla" else torch.nn.Identity(in_channels)


class Upsample(_Launcher):
    """autoencoderldm2d.py:188-203: nearest x2, then a 3x3 convolution when with_conv (the upsampling happens in its loader)."""

    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        self.in_channels = in_channels
        if self.with_conv:
            self.conv = self._conv_cls()(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self._init_launcher()

    def _run(self, x, xs=None):
        if not self.with_conv:
            return ops.upsample_f(x, 2), None
        os_ = self._tiles(x.shape[0], x.shape[1], tuple(2 * s for s in x.shape[2:]), x.device)
        return self._conv3("conv", self.conv, x, up=True, tile_stats=os_), os_

    @ops.device_guard
    def forward(self, x):
        return self._run(self._check(x, self.in_channels, "Upsample"))[0]


class Decoder(_Launcher):
    """autoencoderldm2d.py:358-474 / autoencoderldm3d.py:414-551.  conv_precision ("fp16x3" | "bf16x6" | "fp32") and fuse_norm are
    read at every forward and handed down to the blocks.  "bf16x6" exists for the 3x3 convolutions of fields only: the 1x1
    convolutions then run the exact-fp32 kernel, and on volumes every convolution at a precision other than "fp16x3" runs exact
    fp32 (ops.conv3d, the direct kernel), i.e. "bf16x6" and "fp32" are the same launches there."""
    _ResnetBlock, _AttnBlock, _Upsample = ResnetBlock, AttnBlock, Upsample

    def __init__(self, ddconfig, resamp_with_conv=True, give_pre_end=False, tanh_out=False, use_linear_attn=False,
                 attn_type="vanilla", **ignorekwargs):
        super().__init__()
        if use_linear_attn:
            attn_type = "linear"
        self.give_pre_end = give_pre_end
        self.tanh_out = tanh_out
        for name in DDCONFIG_FIELDS:
            setattr(self, name, getattr(ddconfig, name))
        self.temb_ch = 0
        self.num_resolutions = len(self.ch_mult)
        Conv, Res = self._conv_cls(), self._ResnetBlock

        block_in = self.ch * self.ch_mult[self.num_resolutions - 1]
        curr_res = self.resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, self.z_channels) + (curr_res,) * self._dim
        self.conv_in = Conv(self.z_channels, block_in, kernel_size=3, stride=1, padding=1)

        self.mid = torch.nn.Module()
        self.mid.block_1 = Res(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=self.dropout)
        if self.has_mid_attn:
            self.mid.attn_1 = make_attn(self._AttnBlock, block_in, attn_type=attn_type)
        self.mid.block_2 = Res(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=self.dropout)

        self.up = torch.nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block, attn = torch.nn.ModuleList(), torch.nn.ModuleList()
            block_out = self.ch * self.ch_mult[i_level]
            for _ in range(self.num_res_blocks + 1):
                block.append(Res(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch, dropout=self.dropout))
                block_in = block_out
                if curr_res in self.attn_resolutions:
                    attn.append(make_attn(self._AttnBlock, block_in, attn_type=attn_type))
            up = torch.nn.Module()
            up.block, up.attn = block, attn
            if i_level != 0:
                up.upsample = self._Upsample(block_in, resamp_with_conv)
                curr_res = curr_res * 2
            self.up.insert(0, up)                     # level 0 first, as the reference's keys have it

        self.norm_out = Normalize(block_in)
        self.conv_out = Conv(block_in, self.out_ch, kernel_size=3, stride=1, padding=1)
        self._init_launcher()

    def _hand_down(self):
        for m in self.modules():
            if isinstance(m, _Launcher) and m is not self:
                m.conv_precision, m.fuse_norm = self.conv_precision, self.fuse_norm

    # The walk in the three pieces a tiled decode runs one at a time (diffsci_amd/extra/chunk_decode.py); each takes and returns
    # (h, hs): the activation and the tile statistics its producer left (None off the folded route: always on volumes).
    @staticmethod
    def _attend(att, h, hs):
        return att._run(h, hs) if isinstance(att, AttnBlock) else (h, hs)          # Identity for attn_type "none"

    def _stage0(self, z):
        """conv_in, mid.block_1, mid.attn_1 if present, mid.block_2."""
        self.last_z_shape = z.shape
        hs = self._tiles(z.shape[0], self.conv_in.out_channels, z.shape[2:], z.device)
        h = self._conv3("conv_in", self.conv_in, z, tile_stats=hs)
        h, hs = self.mid.block_1._run(h, hs)
        if self.has_mid_attn:
            h, hs = self._attend(self.mid.attn_1, h, hs)
        return self.mid.block_2._run(h, hs)

    def _level_blocks(self, i_level, h, hs):
        up = self.up[i_level]
        for i_block in range(self.num_res_blocks + 1):
            h, hs = up.block[i_block]._run(h, hs)
            if len(up.attn) > 0:
                h, hs = self._attend(up.attn[i_block], h, hs)
        return h, hs

    def _up_stage(self, i_level, h, hs=None):
        """up[i_level]'s blocks and attention, then its upsample (i_level >= 1)."""
        h, hs = self._level_blocks(i_level, h, hs)
        return self.up[i_level].upsample._run(h, hs)

    def _final_stage(self, h, hs=None):
        """up[0]'s blocks, then norm_out + swish + conv_out and tanh if configured."""
        h, hs = self._level_blocks(0, h, hs)
        if self.give_pre_end:
            return h
        h = self._norm_swish_conv("conv_out", self.norm_out, self.conv_out, h, hs)
        if self.tanh_out:
            h = ops.tanh(h)
        return h

    def _walk(self, z):
        self._hand_down()
        h, hs = self._stage0(z)
        for i_level in reversed(range(1, self.num_resolutions)):
            h, hs = self._up_stage(i_level, h, hs)
        return self._final_stage(h, hs)

    @ops.device_guard
    def forward(self, z):
        if self.training and self.dropout > 0:
            raise NotImplementedError("dropout > 0 in training mode is outside the HIP sampling path: call .eval()")
        return self._walk(self._check(z, self.z_channels, "Decoder"))


class AutoencoderKL(_Launcher):
    """autoencoderldm2d.py:552-614 / autoencoderldm3d.py:641-712, decode half: `decoder` and `post_quant_conv`.  A full reference
    checkpoint (encoder.*, loss.*, quant_conv.*, decoder.*, post_quant_conv.*) loads through init_from_ckpt (strict=False, as the
    reference's); lossconfig and the training arguments are accepted and unused."""
    _Decoder = Decoder

    def _setup(self, ddconfig, embed_dim, ckpt_path, ignore_keys, image_key, colorize_nlabels, monitor):
        self.image_key = image_key
        self.decoder = self._Decoder(ddconfig)
        assert ddconfig.double_z
        self.post_quant_conv = self._conv_cls()(embed_dim, ddconfig.z_channels, 1)
        self.embed_dim = embed_dim
        if colorize_nlabels is not None:
            assert type(colorize_nlabels) is int
            self.register_buffer("colorize", torch.randn(3, colorize_nlabels, *((1,) * self._dim)))
        if monitor is not None:
            self.monitor = monitor
        self._init_launcher()
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    def init_from_ckpt(self, path, ignore_keys=list()):
        sd = torch.load(path, map_location="cpu")["state_dict"]
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        return self.load_state_dict(sd, strict=False)

    def encode(self, x):
        raise NotImplementedError(ENCODER_MESSAGE)

    @ops.device_guard
    def decode(self, z):
        z = self._check(z, self.embed_dim, "AutoencoderKL.decode")
        self.decoder.conv_precision, self.decoder.fuse_norm = self.conv_precision, self.fuse_norm
        m = self.post_quant_conv
        h = self._conv1("post_quant_conv", (m.weight,), (m.bias,), self._v4(z))
        return self.decoder(h.view((z.shape[0], m.out_channels) + tuple(z.shape[2:])))

    def forward(self, input, sample_posterior=True):
        raise NotImplementedError(ENCODER_MESSAGE)
