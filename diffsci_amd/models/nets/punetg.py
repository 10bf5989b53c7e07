"""PUNetG score network on HIP kernels.

Same constructor, forward protocol ``net(x, t=None, y=None)`` and state_dict key names as the
reference (diffsci/models/nets/punetg.py:80-106,356-416), so reference checkpoints load with
``load_state_dict``.  The torch.nn layers created here are *parameter containers only* -- they
give the reference's key names and default initialisers -- and are never called: every tensor
operation of the forward pass is a launch into libdiffsci_hip.so:

  convin / convout / conv1+time-shift / conv2+residual   ds_conv2d (fp32 MFMA implicit GEMM)
  DownSampler (max-pool -> conv), UpSampler (nearest -> conv) + skip add   ds_conv2d load modes (transition_scale_factor 2),
                                                            ds_maxpool_f / ds_upsample_f + plain conv (any other factor)
  GroupNorm(C,C)+SiLU, GroupRMSNorm(C,C)+SiLU              ds_inorm_silu
  GaussianFourierProjection, ResnetTimeBlock MLPs          ds_fourier_features, ds_linear
  ... with a field-valued conditional embedding            per-pixel / per-voxel MLPs as 1x1 convolutions at the block's resolution;
                                                            on volumes ds_cornerpool_f forms te + ye there (CornerPool3d)
  TwoDimensionalAttention (nn.MultiheadAttention, 1 head)  ds_conv2d (1x1 projections) + ds_attention
  x + xa (punetg.py:385)                                    folded into the preceding conv epilogue
"""
import math
import os
from typing import Any

import torch

from ... import ops
from ..._native import DS_LOAD_MAXPOOL2, DS_LOAD_UPSAMPLE2
from . import commonlayers, precision, runtime
from .punetg_config import PUNetGConfig, scale_factor
from .runtime import AmaxArena, Workspace, _amax_kw, require_eval, shift_rows, weights_signature

POOL_ROUTES = ("loader", "pass", "epilogue")
POOL_ROUTE_DEFAULT = "epilogue"


class _AffineHolder(torch.nn.Module):
    """weight/bias container for GroupRMSNorm / GroupPixNorm (commonlayers.py:332-361, 387-414); no parameters
    when affine=False."""

    def __init__(self, C, affine=True):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(C)) if affine else None
        self.bias = torch.nn.Parameter(torch.zeros(C)) if affine else None


NORM_KINDS = {"GroupLN": 0, "GroupRMS": 1, "GroupPix": 3}       # anything else: Identity (kind 2), commonlayers.py:882-899


def make_norm(name, C, affine=True):
    """ResnetBlockC.get_normalization_functions (commonlayers.py:882-899) with num_groups = C."""
    if name == "GroupLN":
        return torch.nn.GroupNorm(C, C, affine=affine)
    if name in ("GroupRMS", "GroupPix"):
        return _AffineHolder(C, affine)
    return torch.nn.Identity()


def mp_weight(w):
    """Effective weight of the magnitude-preserving layers in eval mode (normedlayers.py:17-22,46-55,95-99):
    normalize(w) / sqrt(fan_in) with normalize(x) = x / (eps + ||x_row|| * sqrt(1/fan_in)), eps = 1e-4."""
    fan_in = w[0].numel()
    n = torch.linalg.vector_norm(w, dim=list(range(1, w.ndim)), keepdim=True)
    alpha = math.sqrt(n.numel() / w.numel())
    return (w / torch.add(1e-4, n, alpha=alpha)) / math.sqrt(fan_in)


class _MPConv(torch.nn.Module):
    """MagnitudePreservingConv2d parameters (normedlayers.py:26-44): N(0,1) weight, zero bias."""
    mp = True

    def __init__(self, cin, cout, k, bias=True, dim=2):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(cout, cin, *([k] * dim)))
        self.bias = torch.nn.Parameter(torch.zeros(cout)) if bias else None
        self.in_channels, self.out_channels = cin, cout


class _MPLinear(torch.nn.Module):
    """MagnitudePreservingLinear parameters (normedlayers.py:6-15)."""
    mp = True

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(cout, cin))
        self.bias = torch.nn.Parameter(torch.zeros(cout))


class _InHouseAttention(torch.nn.Module):
    """The reference's own MultiHeadAttention (attention.py:110-153), used instead of nn.MultiheadAttention when the
    network is magnitude preserving or attn_type == "cosine" (attention.py:29-52): one head, dk = dv = dmodel, no
    biases; N(0,1) weights renormalised on the fly when magnitude preserving, Xavier-uniform otherwise."""

    def __init__(self, C, magnitude_preserving, cosine):
        super().__init__()
        for n in ("q", "k", "v", "o"):
            w = torch.empty(1, C, C)
            (torch.nn.init.normal_ if magnitude_preserving else torch.nn.init.xavier_uniform_)(w)
            setattr(self, n + "_proj_matrix", torch.nn.Parameter(w))
        self.embed_dim = C
        self.magnitude_preserving, self.cosine = magnitude_preserving, cosine

    def _normalized(self, weight, kind):
        """MultiHeadAttention.normalize_weight (magnitude preserving only) + the unconditional 1/sqrt(fan_in) of
        forward (attention.py:183-196, 232-247)."""
        fan_in = weight.shape[0] * weight.shape[2] if kind == "wo" else weight.shape[1]
        if self.magnitude_preserving:
            norm = torch.linalg.vector_norm(weight, dim=[0, 2] if kind == "wo" else 1, keepdim=True)
            alpha = math.sqrt(norm.numel() / weight.numel())
            weight = weight / (alpha * norm + 1e-4)
        return weight / math.sqrt(fan_in)

    def projection_weights(self):
        """(in_proj [3E, E], out_proj [E, E]) as 1x1-convolution weights: q = x Wq -> rows of Wq^T;
        out[l] = sum_k a[k] wo[0, l, k]."""
        wq, wk, wv = (self._normalized(getattr(self, n + "_proj_matrix").detach(), "w" + n)[0].t() for n in "qkv")
        wo = self._normalized(self.o_proj_matrix.detach(), "wo")[0]
        return torch.cat([wq, wk, wv], dim=0).contiguous(), wo.contiguous()


class _TimeBlock(torch.nn.Module):
    """ResnetTimeBlock parameters: net.{0,2,4} Linear (commonlayers.py:512-522), magnitude-preserving
    linears when the convolutions are."""

    def __init__(self, embed, out, mp=False):
        super().__init__()
        lin = (lambda i, o: _MPLinear(i, o)) if mp else torch.nn.Linear
        self.net = torch.nn.Sequential(
            lin(embed, 4 * embed), torch.nn.Identity(),
            lin(4 * embed, 4 * embed), torch.nn.Identity(),
            lin(4 * embed, out))


# CircularConv2d / CircularConv3d (commonlayers.py:918-1040): the weights live one level down, in .conv
_CircConv = commonlayers._CircularConv


def make_conv(cin, cout, k, kind="default", bias=True, dim=2):
    """choose_conv_cls (punetg.py:217-236): kind = convolution_type ("default" | "circular" | "mp"), dim 2 or 3."""
    if kind is True or kind == "circular":
        return (commonlayers.CircularConv3d if dim == 3 else commonlayers.CircularConv2d)(cin, cout, k, bias=bias)
    if kind == "mp":
        return _MPConv(cin, cout, k, bias, dim)
    return (torch.nn.Conv3d if dim == 3 else torch.nn.Conv2d)(cin, cout, k, padding="same", bias=bias)


class _ResBlock(torch.nn.Module):
    """ResnetBlockC parameters (commonlayers.py:766-807)."""

    def __init__(self, C, embed, conv_kind="default", bias=True, norms=("GroupLN", "GroupRMS"), affine=True, dim=2, k=3):
        super().__init__()
        self.gnorm1 = make_norm(norms[0], C, affine)
        self.gnorm2 = make_norm(norms[1], C, affine)
        self.conv1 = make_conv(C, C, k, conv_kind, bias, dim)
        self.conv2 = make_conv(C, C, k, conv_kind, bias, dim)
        self.timeblock = _TimeBlock(embed, C, mp=conv_kind == "mp")


class _Sampler(torch.nn.Module):
    def __init__(self, cin, cout, conv_kind="default", bias=True, dim=2, k=3):
        super().__init__()
        self.conv = make_conv(cin, cout, k, conv_kind, bias, dim)


class _Attn(torch.nn.Module):
    def __init__(self, C, mp=False, cosine=False, heads=1):
        super().__init__()
        self.mhattn = (_InHouseAttention(C, mp, cosine) if (mp or cosine)
                       else torch.nn.MultiheadAttention(C, num_heads=heads, batch_first=True))


class _Fourier(torch.nn.Module):
    def __init__(self, embed_dim, scale):
        super().__init__()
        self.register_buffer("W", torch.randn(embed_dim // 2) * scale)


class _FourierInput(torch.nn.Module):
    """ConvolutionalFourierProjection buffers (commonlayers.py:229-244), bias=False: W [input_dim, embed_dim/2]."""

    def __init__(self, input_dim, embed_dim, scale):
        super().__init__()
        self.register_buffer("W", torch.randn(input_dim, embed_dim // 2) * scale)
        self.in_channels, self.out_channels = input_dim, embed_dim


class _ConditionDrop(torch.nn.Module):
    """ConditionDrop parameters (commonlayers.py:1100-1127): identity outside training; the null embedding is only a
    state_dict entry here."""

    def __init__(self, p, hidden_dim, null_is_learnable=True):
        super().__init__()
        self.p = p
        if null_is_learnable:
            self.null_embedding = torch.nn.Parameter(torch.randn(1, hidden_dim))
        else:
            self.register_buffer("null_embedding", torch.zeros(1, hidden_dim))


def corner_pool_factor(field, block):
    """ResnetBlockC.rescale_yt (commonlayers.py:838-869) as a rule: a field of time embeddings with sides `field` serves a block
    with sides `block` through the top-left corner of every window of f pixels a side (CornerPool) -> f, 1 for equal sides.  The
    factor comes from the first side; every side must satisfy block * f == field.  A coarser field takes the reference through
    torch.nn.Upsample(shape_factor), whose first argument is the output size -- it fails there unless the block's side equals
    the factor; not reproduced."""
    field, block = tuple(field), tuple(block)
    if len(field) == len(block):
        if field == block:
            return 1
        if field[0] <= block[0]:
            raise NotImplementedError("a conditional-embedding field coarser than a block's resolution (the reference's "
                                      "upscaling branch passes the factor as torch.nn.Upsample's size and fails as well)")
        f = field[0] // block[0]
        if all(d * f == s for d, s in zip(block, field)):
            return f
    raise ValueError(f"yt_dims {field} and y_dims {block} are not compatible")


class _FieldShifts:
    """Per-pixel time shifts, computed where they are used.  A field-valued conditional embedding makes the time embedding a
    field te [B, C, He, We] (punetg.py:405-410) and every block's ResnetTimeBlock a per-pixel MLP (commonlayers.py:537-546)
    whose result the block brings to its own resolution by taking the top-left corner of every window (rescale_yt,
    commonlayers.py:838-869).  The MLP is pointwise, so corner-pooling its INPUT gives the same values: each block evaluates
    its three 1x1 convolutions at its own resolution (16x fewer pixels two levels down) from a pooled copy of te that the
    blocks of a level share.  Every buffer comes from the network's workspace, so the evaluation can sit inside a captured run."""

    def __init__(self, te, ws, h3, owned=False, rows=None, batch=None):
        """2-D networks: te is the field te + ye [B, C, He, We].  Volumes: te is the embedded condition ye [1 or B, C, De, He, We]
        alone, rows the time embedding [1 or B, C] (None: zeros) and batch the batch of x -- `level` adds the two while it pools
        (ops.cornerpool_f), so their sum at the field's own resolution is never written."""
        self.te, self.ws, self.te_owned = te, ws, owned
        self.rows, self.batch = rows, te.shape[0] if batch is None else batch
        self.am = AmaxArena(ws, self.batch, te.device) if h3 else None
        self.levels = {}

    def level(self, *dims):
        """te at a block's resolution -- level(H, W) -> [B, C, H, W], level(D, H, W) -> [B, C, D, H, W] -- and its amax row
        (fp16x3)."""
        dims = tuple(int(v) for v in dims)
        got = self.levels.get(dims)
        if got is None:
            f = corner_pool_factor(self.te.shape[2:], dims)
            if self.te.dim() == 5:           # volumes: one ds_cornerpool_f launch per resolution writes te + ye there and leaves its amax row
                a = self.am.row() if self.am is not None else None
                t = ops.cornerpool_f(self.te, f, te=self.rows, out_amax=a,
                                     out=self.ws.take((self.batch, self.te.shape[1]) + dims, self.te.device))
            else:
                t = self.te
                if f > 1:
                    t = self.ws.take(tuple(self.te.shape[:2]) + dims, self.te.device)
                    t.copy_(self.te[:, :, ::f, ::f])                  # CornerPool2d(f): the top-left corner of every window
                a = self.am.of(t) if self.am is not None else None
            got = self.levels[dims] = (t, a, t is not self.te)
        return got[0], got[1]

    def release(self):
        for t, _, owned in self.levels.values():
            if owned:
                self.ws.give(t)
        self.levels = {}
        if self.am is not None:
            self.am.release()
            self.am = None
        if self.te_owned:
            self.ws.give(self.te)
            self.te_owned = False


class PUNetG(commonlayers.PeriodicAxes, torch.nn.Module):
    def __init__(self,
                 config: PUNetGConfig,
                 conditional_embedding: torch.nn.Module | None = None,
                 extra_residual: torch.nn.Module | None = None):
        super().__init__()
        why = config.unsupported_reason()
        if why:
            raise NotImplementedError(why)
        # extra_residual (punetg.py:83-92,249-261; commonlayers.py:831-833): ONE user module shared by every residual
        # block, y = (conv2(...) + x) + extra_residual(x).  It is ordinary torch code run as given (it may allocate), so a
        # network that carries one is evaluated launch by launch instead of from a captured graph.
        self.extra_residual = extra_residual
        self.capturable = extra_residual is None
        self.config = config
        # transition_scale_factor: 2 pools / upsamples inside the Down / UpSamplers' convolution loaders (DS_LOAD_MAXPOOL2 /
        # DS_LOAD_UPSAMPLE2, parity-packed upsampler weights); any other factor runs ds_maxpool_f / ds_upsample_f into a
        # workspace buffer and the plain convolution after it
        self.factor = scale_factor(config.transition_scale_factor)
        mc = config.model_channels
        self.time_projection = _Fourier(mc, config.time_projection_scale)
        self.conditional_embedding = conditional_embedding
        self.cond_drop = (_ConditionDrop(config.cond_drop, mc, config.cond_drop_learnable)
                          if config.cond_drop is not None and config.cond_drop > 0 else None)     # punetg.py:102-106
        # periodic padding: circular_axes, one bool per spatial axis in tensor-axis order, is the one source (commonlayers.
        # PeriodicAxes): `circular` = some axis wraps (the routes: no norm_images, no pool_route, no exact input layer),
        # `circular_arg` = what every launch of the walk passes as circular=.  convolution_type "circular" is every axis;
        # extra.convert_conv_to_circular sets a subset.
        self.circular_axes = (config.convolution_type == "circular",) * config.dimension
        self.mp = config.convolution_type == "mp"
        self.cosine_attn = config.attn_type == "cosine"
        self.inhouse_attn = self.mp or self.cosine_attn        # attention.py:29-52
        norms = (config.first_resblock_norm, config.second_resblock_norm)
        self.norm_kinds = tuple(NORM_KINDS.get(n, 2) for n in norms)
        # bias=False: no convolution biases; a constant-one input channel is appended instead (punetg.py:190-191,390-394)
        dim = self.dim = config.dimension
        # the reference's construction sequence and builder names (punetg.py:94-106); the builders return parameter CONTAINERS
        # with the reference's state_dict keys -- the tensor work is in forward_with_shifts
        self.convin, self.convout = self.make_convin_and_convout()
        self.downward_blocks, self.downsamplers = self.make_downward_blocks()
        self.upward_blocks, self.upsamplers = self.make_upward_blocks()
        self.before_block, self.after_block = self.make_non_attn_bottom_blocks()
        self.attn_resnet_block, self.attn_block = self.make_attn_bottom_blocks()
        # Arithmetic of the 3x3 convolutions -- all three give fp32-level error (tests/test_gpu_kernels.py):
        #   "fp16x3": fp16 hi+lo split, 3 MFMA products (default; inputs must stay below 65504 in magnitude)
        #   "bf16x6": exact 3-way bf16 split, 6 MFMA products (no range limit, half the speed)
        #   "fp32"  : exact-fp32 MFMA (1/16 of the 16-bit rate)
        self.conv_precision = "fp16x3"
        # fp16x3 only: a non-finite output from finite inputs means an activation left fp16's range; switch to the
        # range-free "bf16x6" once and recompute (nets/precision.py) instead of handing the user NaNs
        self.auto_precision = True
        # With the fp16x3 kernels the two norms of a residual block are folded into the convolutions
        # around them (statistics from the producer's epilogue, normalise + SiLU in the consumer's
        # loader): the normalised tensors never touch HBM.  False: standalone ds_inorm_silu kernels.
        self.fuse_norm = True
        # ... but only where one workgroup column covers all output channels: with Cout/64 > fuse_max_cot channel
        # tiles every tile's workgroup would redo the activation of the same input patch (5.3x the transcendental
        # work of a standalone pass at Cout = 256), and the standalone kernel wins
        self.fuse_max_cot = 2
        # The DownSampler's MaxPool2d(2) (fields, fp16x3, 3x3 transition kernel; every route gives the same bits):
        #   "loader"  : the convolution's loader pools (DS_LOAD_MAXPOOL2: four raw pixels per element, once per channel tile)
        #   "pass"    : a pooling pass (ops.maxpool_f), then a plain convolution on the persistent kernel
        #   "epilogue": the level's last residual block writes the pooled tensor from its store phase (ops.PoolOut) and the plain
        #               convolution follows; where that launch does not qualify, the loader
        # DIFFSCI_POOL_ROUTE sets the default (A/B runs)
        self.pool_route = os.environ.get("DIFFSCI_POOL_ROUTE", POOL_ROUTE_DEFAULT)
        # Standalone norms hand their convolutions pre-split fp16 images (ops.inorm_silu_images / ops.conv_img) where the layer
        # qualifies (_norm_images_ok); DIFFSCI_NORM_IMAGES=0 keeps the fp32 route (A/B runs)
        self.norm_images = os.environ.get("DIFFSCI_NORM_IMAGES", "1") != "0"
        # Single-head attention blocks on the image-form route fold their K and V projections into the Q and the output projection
        # (runtime.attention, folded=: an E -> E in-projection instead of E -> 3E, x itself as keys and values);
        # DIFFSCI_ATTN_FOLD=0 keeps the three projections (A/B runs)
        self.attn_fold = os.environ.get("DIFFSCI_ATTN_FOLD", "1") != "0"
        self._packed = None
        self._packed_sig = None
        self._ws = Workspace()
        self._am = None              # the amax arena of the forward pass in flight
        self._window_cache = {}
        # set by precision.escalate_input when the input's channels differ by more than 2^14 in magnitude within a sample
        self.exact_input_layer = False

    def drop_caches(self):
        """commonlayers.PeriodicAxes.drop_caches, with this network's own: the time blocks' packings, the workspace, the norm
        window cache."""
        super().drop_caches()
        self.__dict__.pop("_tb_packed", None)
        self.__dict__.pop("_tb_packed_sig", None)
        self.__dict__.pop("_attn_folded", None)
        self._ws, self._am, self._window_cache = Workspace(), None, {}

    # ------------------------------------------------------------------ builders (punetg.py:122-334: same names and arguments)
    def choose_conv_cls(self):
        """punetg.py:217-236: the convolution constructor of this configuration -- here a callable
        (in_channels, out_channels, kernel_size, bias=True) that builds the parameter container of that convolution type."""
        if self.config.dimension not in (2, 3):
            raise NotImplementedError("1D convolution not implemented yet") if self.config.dimension == 1 \
                else ValueError(f"Invalid dimension {self.config.dimension}")
        kind, dim = self.config.convolution_type, self.config.dimension

        def conv_cls(in_channels, out_channels, kernel_size, bias=True, **_):
            return make_conv(in_channels, out_channels, kernel_size, kind, bias, dim)
        return conv_cls

    def make_convin_and_convout(self):
        """punetg.py:188-215.  bias=False: no convolution biases; a constant-one input channel is appended instead."""
        c = self.config
        conv_cls = self.choose_conv_cls()
        cin = c.input_channels + (0 if c.bias else 1)
        if c.in_embedding:                               # fixed Fourier input embedding instead of a convolution, punetg.py:194-202
            convin = _FourierInput(cin, c.model_channels, c.input_projection_scale)
        else:
            convin = conv_cls(cin, c.model_channels, c.in_out_kernel_size, bias=bool(c.bias))
        convout = conv_cls(c.model_channels, c.output_channels, c.in_out_kernel_size, bias=bool(c.bias))
        return convin, convout

    def resnet_fn(self, input_multiplier: int):
        """punetg.py:238-261: one ResnetBlockC's parameters."""
        c = self.config
        blk = _ResBlock(input_multiplier * c.model_channels, c.model_channels, c.convolution_type, bool(c.bias),
                        (c.first_resblock_norm, c.second_resblock_norm), bool(c.affine_norm), c.dimension, c.kernel_size)
        if self.extra_residual is not None:
            blk.extra_residual = self.extra_residual        # the reference registers the shared module in every block
        return blk

    def resnet_block_fn(self, input_multiplier: int, number_resnet_per_block: int):
        return torch.nn.ModuleList([self.resnet_fn(input_multiplier) for _ in range(number_resnet_per_block)])

    def attn_fn(self, input_multiplier: int):
        """punetg.py:272-289."""
        if self.config.dimension not in (2, 3):
            raise NotImplementedError("1D attention not implemented yet") if self.config.dimension == 1 \
                else ValueError(f"Invalid dimension {self.config.dimension}")
        return _Attn(input_multiplier * self.config.model_channels, self.config.magnitude_preserving,
                     self.config.attn_type == "cosine")

    def attn_block_fn(self, input_multiplier: int, number_resnet_attn_block: int):
        return torch.nn.ModuleList([self.attn_fn(input_multiplier) for _ in range(number_resnet_attn_block - 1)])

    def downsampler_fn(self, input_multiplier: int, output_multiplier: int):
        """punetg.py:300-316: DownSampler (max-pool, then convolution)."""
        c = self.config
        return _Sampler(input_multiplier * c.model_channels, output_multiplier * c.model_channels, c.convolution_type,
                        bool(c.bias), c.dimension, c.transition_kernel_size)

    def upsampler_fn(self, input_multiplier: int, output_multiplier: int):
        """punetg.py:318-334: UpSampler (nearest upsampling, then convolution): the same parameters as a DownSampler."""
        return self.downsampler_fn(input_multiplier, output_multiplier)

    def make_downward_blocks(self):
        mult = self.config.extended_channel_expansion
        blocks, samplers = torch.nn.ModuleList(), torch.nn.ModuleList()
        for i, m in enumerate(mult[:-1]):
            blocks.append(self.resnet_block_fn(m, self.config.number_resnet_downward_block))
            samplers.append(self.downsampler_fn(m, mult[i + 1]))
        return blocks, samplers

    def make_upward_blocks(self):
        rmult = list(reversed(self.config.extended_channel_expansion))
        blocks, samplers = torch.nn.ModuleList(), torch.nn.ModuleList()
        for i, m in enumerate(rmult[:-1]):
            samplers.append(self.upsampler_fn(m, rmult[i + 1]))
            blocks.append(self.resnet_block_fn(rmult[i + 1], self.config.number_resnet_upward_block))
        return blocks, samplers

    def make_non_attn_bottom_blocks(self):
        m = self.config.extended_channel_expansion[-1]
        return (self.resnet_block_fn(m, self.config.number_resnet_before_attn_block),
                self.resnet_block_fn(m, self.config.number_resnet_after_attn_block))

    def make_attn_bottom_blocks(self):
        m, n = self.config.extended_channel_expansion[-1], self.config.number_resnet_attn_block
        return self.resnet_block_fn(m, n), self.attn_block_fn(m, n)

    def calculate_receptive_field(self) -> dict:
        """punetg.py:423-628: theoretical receptive field of the network in input pixels.  A convolution of size k at cumulative
        stride s widens it by (k - 1) s, a residual block by twice that, a max-pool of size p by (p - 1) s before multiplying
        the stride by p; nearest upsampling only divides the stride; global attention makes it infinite."""
        c = self.config
        trace = []
        n_attn = c.number_resnet_attn_block - 1
        if n_attn > 0:
            trace.append(f"{n_attn} global attention layer(s): every output pixel sees every input pixel")
            return {'rf': float('inf'), 'has_attention': True, 'num_attention_layers': n_attn, 'trace': trace,
                    'feasible_chunking': False,
                    'config_summary': {'number_resnet_attn_block': c.number_resnet_attn_block, 'kernel_size': c.kernel_size,
                                       'in_out_kernel_size': c.in_out_kernel_size, 'channel_expansion': c.channel_expansion}}
        rf, stride = 1, 1

        def widen(k, name, times=1):
            nonlocal rf
            rf += times * (k - 1) * stride
            trace.append(f"{name}: {times} x (k = {k}) at stride {stride} -> {rf}")
        if c.in_embedding:
            trace.append("convin is a per-pixel Fourier embedding: unchanged")
        else:
            widen(c.in_out_kernel_size, "convin")
        levels = len(c.channel_expansion)
        for lv in range(levels):
            for b in range(c.number_resnet_downward_block):
                widen(c.kernel_size, f"down[{lv}].resnet[{b}]", 2)
            widen(c.transition_scale_factor, f"down[{lv}].maxpool")
            stride *= c.transition_scale_factor
            widen(c.transition_kernel_size, f"down[{lv}].conv")
        for name, n in (("before_block", c.number_resnet_before_attn_block), ("attn_resnet_block", c.number_resnet_attn_block),
                        ("after_block", c.number_resnet_after_attn_block)):
            for b in range(n):
                widen(c.kernel_size, f"{name}[{b}]", 2)
        for lv in range(levels - 1, -1, -1):
            stride //= c.transition_scale_factor
            widen(c.transition_kernel_size, f"up[{lv}].conv")
            for b in range(c.number_resnet_upward_block):
                widen(c.kernel_size, f"up[{lv}].resnet[{b}]", 2)
        widen(c.in_out_kernel_size, "convout")
        return {'rf': rf, 'has_attention': False, 'num_attention_layers': 0, 'trace': trace, 'feasible_chunking': True,
                'downsampling_factor': c.transition_scale_factor ** levels,
                'config_summary': {k: getattr(c, k) for k in (
                    'number_resnet_attn_block', 'number_resnet_downward_block', 'number_resnet_upward_block',
                    'number_resnet_before_attn_block', 'number_resnet_after_attn_block', 'kernel_size', 'in_out_kernel_size',
                    'transition_kernel_size', 'transition_scale_factor', 'channel_expansion')}}

    # ------------------------------------------------------------------ reference surface
    def export_description(self) -> dict[str, Any]:
        cemb = self.conditional_embedding
        cemb_args = cemb.export_description() if getattr(cemb, "export_description", None) else None
        return dict(config=self.config.export_description(),
                    conditional_embedding_args=cemb_args,
                    has_conditional_embedding=cemb is not None)

    def set_conditional_embedding(self, conditional_embedding: torch.nn.Module | None = None):
        self.conditional_embedding = conditional_embedding

    @ops.device_guard
    def forward(self, x, t=None, y=None):
        """punetg.py:389-416.  x [B, Cin, H, W]; t [B] noise conditioning; y optional condition.  A top-level call: the result
        is checked by the domain guards (nets/precision.py: one device reduction and a host read) and recomputed if one fires;
        the sampler's eager path calls forward_unguarded and checks once per run."""
        return runtime.guarded_forward(self, self.forward_unguarded, x, t, y)

    def check_field_size(self, shape):
        """With transition_scale_factor f != 2 every spatial side must divide by f ** (number of transitions), else a decoder
        level misses the skip it joins (the reference fails there, at the addition); raised before any launch.  Factor 2 keeps
        the checks of its loaders."""
        f, n = self.factor, len(self.config.channel_expansion)
        if f == 2 or n == 0:
            return
        sides = tuple(shape[2:])
        if any(v % f ** n for v in sides):
            what = "volume" if len(sides) == 3 else "field"
            raise ValueError(f"a {'x'.join(map(str, sides))} {what} does not divide by transition_scale_factor ** {n} = {f ** n} "
                             f"({n} transitions by {f}): choose sides that are multiples of {f ** n}")

    @ops.device_guard
    def forward_unguarded(self, x, t=None, y=None):
        ops.require_device(x, "x")
        self.check_field_size(x.shape)
        return self.forward_with_shifts(x.contiguous(), self._eager_shifts(x, t, self.embed_condition(y)), row=None)

    def _eager_shifts(self, x, t, ye):
        """The time shifts of one eager evaluation from the embedded condition ye (None, [1 or B, C] or a field)."""
        B = x.shape[0]
        if ye is not None and ye.dim() > 2:                       # a field of embeddings: per-pixel time shifts
            return self.field_shifts(None if t is None else self.embed_time(t.reshape(-1).to(x)), ye, B)
        if t is None:                                              # punetg.py:398-399, 410: zeros (+ ye)
            te = torch.zeros(B, self.config.model_channels, device=x.device)
            if ye is not None:
                te = te + ye
        else:
            te = self.embed_time(t.reshape(-1).to(x), ye)
        return self.time_shifts(te)

    # ------------------------------------------------------------------ conditioning
    def embed_condition(self, y):
        """ye of punetg.py:400-410 (conditional_embedding is a user module, run as given)."""
        if y is None:
            return None
        ye = y if self.conditional_embedding is None else self.conditional_embedding(y)
        if ye.dim() == 2 + self.dim:                              # punetg.py:405-407: a field [B or 1, C, (D,) H, W]
            if ye.shape[1] != self.config.model_channels:
                raise ValueError("a field-valued conditional embedding must have model_channels channels")
            ops.require_device(ye, "conditional embedding")
            return ye.detach().to(torch.float32).contiguous()         # inference only: the kernels carry no autograd graph
        if ye.dim() != 2:
            raise ValueError(f"a conditional embedding is a vector [B or 1, C] or, on a dimension={self.dim} network, a field of "
                             f"rank {2 + self.dim} ([B or 1, C, {'D, H, W' if self.dim == 3 else 'H, W'}]); got rank {ye.dim()}")
        return ye.to(torch.float32).contiguous()

    def condition_is_field(self, y):
        """True when conditional_embedding(y) is a field: every evaluation then computes per-pixel time shifts (they depend on
        sigma, so nothing is tabulated per run; engine.ModuleSource evaluates them out of the workspace through `field_shifts`)."""
        ye = None if y is None else self.embed_condition(y)
        return ye is not None and ye.dim() > 2

    def field_shifts(self, te, ye, B):
        """The time embedding as a field, te.reshape(B, C, 1, 1) + ye (punetg.py:405-410; te [1 or B, C] or None for zeros,
        ye [1 or B, C, He, We]), wrapped for the blocks to evaluate their per-pixel time MLPs from (`_FieldShifts`).  All
        buffers are workspace buffers: forward_with_shifts gives them back.  On volumes (ye [1 or B, C, De, He, We]) the sum is
        left to ds_cornerpool_f, which forms it at each block resolution while it pools: ye and te are handed over as they are
        (the caller keeps them alive until forward_with_shifts returns)."""
        if ye.shape[0] not in (1, B):
            raise ValueError("conditional embedding batch must be 1 or match x")
        if te is not None and te.shape[0] not in (1, B):
            raise ValueError("time batch must be 1 or match x")
        ws = self._ws
        if ye.dim() == 5:
            return _FieldShifts(ye, ws, self.conv_precision == "fp16x3", rows=te, batch=B)
        field = ws.take((B,) + tuple(ye.shape[1:]), ye.device)
        if te is None:
            field.copy_(ye.expand(B, -1, -1, -1))
        else:
            torch.add(te[:, :, None, None].expand(B, -1, 1, 1), ye, out=field)
        return _FieldShifts(field, ws, self.conv_precision == "fp16x3", owned=True)

    def _field_shift(self, blk, fs, *dims):
        """ResnetTimeBlock of one block on the field at the block's resolution: the three linears as 1x1 convolutions on the
        matrix cores, SiLU in between (commonlayers.py:537-546) -> [B, C_block, H, W] from the workspace (the caller gives it back).
        Volumes (dims = D, H, W): the same convolutions on the [B, C, D*H, W] view of the buffers -- a 1x1 convolution does not care
        how the positions are laid out, and this view fills the kernel's 8 x 32 / 16 x 16 pixel tiles where [B, C, 1, D*H*W] would
        use one row of each (measured: 140 of the 197 ms of a 64^3, B = 8 evaluation went to those launches)."""
        pk, ws = self._timeblock_convs(), fs.ws
        te, a0 = fs.level(*dims)
        B, dev = te.shape[0], te.device
        if len(dims) == 3:
            te = te.view(B, te.shape[1], dims[0] * dims[1], dims[2])
        H, W = te.shape[2:]
        n = blk.timeblock.net
        a1 = fs.am.row() if fs.am is not None else None
        a2 = fs.am.row() if fs.am is not None else None
        h = ops.conv(te, pk[id(n[0])], bias=n[0].bias, out=ws.take((B, n[0].out_features, H, W), dev),
                     **_amax_kw(pk[id(n[0])], in_amax=a0, out_amax=a1))
        ops.inorm_silu(h, None, None, kind=2, out=h)                 # |SiLU(v)| <= |v|: a1 stays a valid bound
        h2 = ops.conv(h, pk[id(n[2])], bias=n[2].bias, out=ws.take((B, n[2].out_features, H, W), dev),
                      **_amax_kw(pk[id(n[2])], in_amax=a1, out_amax=a2))
        ops.inorm_silu(h2, None, None, kind=2, out=h2)
        out = ops.conv(h2, pk[id(n[4])], bias=n[4].bias, out=ws.take((B, n[4].out_features, H, W), dev),
                       **_amax_kw(pk[id(n[4])], in_amax=a2))
        ws.give(h)
        ws.give(h2)
        return out                                                   # volumes: [B, C_block, D*H, W], viewed by the caller

    def _timeblock_convs(self):
        lins = list(self._timeblock_linears())
        sig = weights_signature([l.weight for l in lins], self.conv_precision)
        if getattr(self, "_tb_packed_sig", None) != sig:
            with torch.no_grad():
                self._tb_packed = {}
                for l in lins:
                    w = mp_weight(l.weight.detach()) if self.mp else l.weight.detach()
                    self._tb_packed[id(l)] = ops.pack_conv(w.reshape(w.shape[0], w.shape[1], 1, 1).contiguous(),
                                                           "fp16x3" if self.conv_precision == "fp16x3" else "fp32")
            self._tb_packed_sig = sig
        return self._tb_packed

    def embed_time(self, t, ye=None):
        """te = GaussianFourierProjection(t) [+ ye]  (punetg.py:396-410)."""
        if ye is not None and ye.shape[0] not in (1, t.numel()):
            raise ValueError("conditional embedding batch must be 1 or match t")
        return ops.fourier_features(t.contiguous(), self.time_projection.W, add=ye)

    def time_shifts(self, te):
        """Per-block ResnetTimeBlock(te): list of [M, C_block] tensors in block order."""
        pk = self.packed_weights() if self.mp else None                # once per call, not once per block
        return [self._shift_of(blk, te, pk) for blk in self._resblocks()]

    def _resblocks(self):
        for lv in self.downward_blocks:
            yield from lv
        yield from self.before_block
        yield from self.attn_resnet_block
        yield from self.after_block
        for lv in self.upward_blocks:
            yield from lv

    # ------------------------------------------------------------------ the reference's public stages
    # PUNetG.encode / bottom_forward / decode and their helpers (punetg.py:336-387) for callers that drive the
    # stages themselves (e.g. the encoder / decoder halves of punetg_encdec.py).  Eager launches of the same
    # kernels as forward(); te is the [B, model_channels] embedding (time projection + condition); results are
    # fresh tensors, never workspace buffers.
    def _shift_of(self, blk, te, pk=None):
        """ResnetTimeBlock(te) of one block -> [M, C_block]; pk: the packed weights, when the caller has them at hand."""
        if pk is None and self.mp:
            pk = self.packed_weights()
        n = blk.timeblock.net
        wgt = (lambda lin: pk[(id(lin), "eff")]) if pk is not None else (lambda lin: lin.weight)
        h = ops.linear(te, wgt(n[0]), n[0].bias, act=1)
        h = ops.linear(h, wgt(n[2]), n[2].bias, act=1)
        return ops.linear(h, wgt(n[4]), n[4].bias, act=0)

    def _run_blocks(self, x, te, resnet_block, attn_block=()):
        """-> (tensor, stats, owned): owned tensors are workspace buffers the caller must clone and give back."""
        if self.dim != 2:
            raise NotImplementedError("the public stage methods are implemented for 2-D networks")
        pk, ws = self.packed_weights(), self._ws
        h, hs, own = x, None, False
        for i, blk in enumerate(resnet_block):
            h2, hs2 = self._res(blk, h, self._shift_of(blk, te), pk, ws, xs=hs)
            if own:
                ws.give(h)
                if hs is not None:
                    ws.give(hs)
            h, hs, own = h2, hs2, True
            if i < len(attn_block):
                hs2 = self._stats_buf(ws, h.shape[0], h.shape[1], h.shape[2], h.shape[3], h.device)
                h2 = self._attention(attn_block[i], h, pk, ws, tile_stats=hs2)
                ws.give(h)
                if hs is not None:
                    ws.give(hs)
                h, hs = h2, hs2
        return h, hs, own

    def _release(self, h, hs, own):
        out = h.clone() if own else h
        if own:
            self._ws.give(h)
        if hs is not None:
            self._ws.give(hs)
        return out

    @ops.device_guard
    def resnet_block_forward(self, x, te, resnet_block):
        require_eval(self, self.config.dropout, self.config.cond_dropout, self.config.cond_drop)
        ops.require_device(x, "x")
        return self._release(*self._run_blocks(x.contiguous(), te, resnet_block))

    @ops.device_guard
    def resnet_attn_block_forward(self, x, te, resnet_block, attn_block):
        require_eval(self, self.config.dropout, self.config.cond_dropout, self.config.cond_drop)
        ops.require_device(x, "x")
        return self._release(*self._run_blocks(x.contiguous(), te, resnet_block, attn_block))

    def encode(self, x, te):
        """punetg.py:356-365 -> (x at the bottom resolution, [level outputs])."""
        pk = self.packed_weights()
        intermediate_outputs = []
        for resnet_block, downsampler in zip(self.downward_blocks, self.downsamplers):
            x = self.resnet_block_forward(x, te, resnet_block)
            intermediate_outputs.append(x.clone())
            if self.factor == 2:
                x = self._conv(downsampler.conv, x, pk, load_mode=DS_LOAD_MAXPOOL2)
            else:
                x = self._conv(downsampler.conv, ops.maxpool_f(x, self.factor), pk)
        return x, intermediate_outputs

    def decode(self, x, te, intermediate_outputs):
        """punetg.py:367-376 (pops the skips, like the reference)."""
        pk = self.packed_weights()
        for resnet_block, upsampler in zip(self.upward_blocks, self.upsamplers):
            if self.factor == 2:
                x = self._conv(upsampler.conv, x.contiguous(), pk, load_mode=DS_LOAD_UPSAMPLE2, res1=intermediate_outputs.pop())
            else:
                x = self._conv(upsampler.conv, ops.upsample_f(x.contiguous(), self.factor), pk, res1=intermediate_outputs.pop())
            x = self.resnet_block_forward(x, te, resnet_block)
        return x

    def bottom_forward(self, x, te):
        """punetg.py:378-387."""
        x = self.resnet_block_forward(x, te, self.before_block)
        xa = self.resnet_attn_block_forward(x, te, self.attn_resnet_block, self.attn_block)
        x = ops.add(x, xa)
        return self.resnet_block_forward(x, te, self.after_block)

    # ------------------------------------------------------------------ weights
    def _conv_modules(self):
        if not isinstance(self.convin, _FourierInput):
            yield self.convin
        yield self.convout
        for blk in self._resblocks():
            yield blk.conv1
            yield blk.conv2
        for s in list(self.downsamplers) + list(self.upsamplers):
            yield s.conv

    def _timeblock_linears(self):
        for blk in self._resblocks():
            n = blk.timeblock.net
            yield from (n[0], n[2], n[4])

    def packed_weights(self):
        """MFMA-operand repack of every conv / projection weight, cached per parameter version.  Magnitude-preserving
        layers contribute their eval-mode effective weights (mp_weight), computed here once per weight version."""
        mods = list(self._conv_modules())
        tracked = [m.weight for m in mods]
        for a in self.attn_block:
            tracked += ([a.mhattn.q_proj_matrix, a.mhattn.k_proj_matrix, a.mhattn.v_proj_matrix, a.mhattn.o_proj_matrix]
                        if self.inhouse_attn else [a.mhattn.in_proj_weight, a.mhattn.out_proj.weight])
        if self.mp:
            tracked += [lin.weight for lin in self._timeblock_linears()]
        sig = weights_signature(tracked, self.conv_precision, getattr(self, "upsample_parity", True), self.exact_input_layer)
        if self._packed is not None and sig == self._packed_sig:
            return self._packed
        pk = {}
        with torch.no_grad():
            # parity kernels exist for nearest x2 only: other factors upsample in a pass of their own
            ups = {id(u.conv) for u in self.upsamplers} if getattr(self, "upsample_parity", True) and self.factor == 2 else set()
            for m in mods:
                w = m.weight.detach()
                if getattr(m, "mp", False):
                    w = mp_weight(w)
                    pk[(id(m), "eff")] = w                         # the direct output-layer kernel takes the raw layout
                if self.dim == 2:
                    pk[id(m)] = ops.pack_conv(w, self.conv_precision, upsampled=id(m) in ups)
                    if m is self.convin and self.conv_precision == "fp16x3":
                        pk[(id(m), "wmax")] = w.abs().amax(dim=(0, 2, 3)).contiguous()   # the input layer's channel guard
                        if self.exact_input_layer:
                            pk[(id(m), "exact")] = ops.pack_conv(w, "fp32")
                elif self.conv_precision == "fp16x3":              # volumes on the matrix cores: one packing per depth tap
                    pk[(id(m), "3d")] = ops.pack_conv3d(w, upsampled=id(m) in ups)
                # other precisions: ds_conv3d_direct reads the torch layout
            prec = "fp16x3" if self.conv_precision == "fp16x3" else "fp32"
            for a in self.attn_block:
                E = a.mhattn.embed_dim
                if self.inhouse_attn:
                    w_in, w_out = a.mhattn.projection_weights()
                else:
                    w_in, w_out = a.mhattn.in_proj_weight.detach(), a.mhattn.out_proj.weight.detach()
                pk[(id(a), "in")] = ops.pack_conv(w_in.reshape(3 * E, E, 1, 1), prec)
                pk[(id(a), "out")] = ops.pack_conv(w_out.reshape(E, E, 1, 1), prec)
            if self.mp:
                for lin in self._timeblock_linears():
                    pk[(id(lin), "eff")] = mp_weight(lin.weight.detach()).contiguous()
        self._packed, self._packed_sig = pk, sig
        return pk

    # ------------------------------------------------------------------ the network
    def _conv(self, m, x, pk, in_amax=None, out_amax=None, **kw):
        return ops.conv(x, pk[id(m)], bias=m.bias, circular=self.circular_arg, **_amax_kw(pk[id(m)], in_amax=in_amax, out_amax=out_amax), **kw)

    def _out_is_direct(self, m):
        return m.out_channels <= 4 and getattr(self, "direct_out", True) and self.config.in_out_kernel_size == 3

    def _out_conv(self, m, h, pk, out, circular, in_amax=None):
        """The output layer: Cout <= 4 streams the input once through the direct fp32 kernel instead of
        padding Cout to a 64-channel MFMA tile."""
        if self._out_is_direct(m):
            return ops.conv_direct(h, pk.get((id(m), "eff"), m.weight), m.bias, circular=circular, out=out)
        return ops.conv(h, pk[id(m)], bias=m.bias, circular=circular, out=out, **_amax_kw(pk[id(m)], in_amax=in_amax))

    def _fused(self):
        return self.fuse_norm and self.conv_precision == "fp16x3"

    def _stats_buf(self, ws, B, C, H, W, dev):
        """Tile-statistics buffer for a [B, C, H, W] convolution output (None when norms are not fused)."""
        if not self._fused():
            return None
        return ws.take((B, C, ops.conv_tile_count(H, W), 4), dev)

    def _res(self, blk, x, shift, pk, ws, res2=None, xs=None, want_stats=True, out_amax=None, pool=None):
        """ResnetBlockC.forward (commonlayers.py:824-833); returns (fresh buffer, its tile statistics);
        x untouched.  xs = tile statistics of x (from the convolution that produced it) or None.  out_amax: a zeroed amax row
        that receives the per-sample max |result| (the result feeds a raw-input launch: Down/UpSampler, attention).  pool: an
        ops.PoolOut that conv2's store phase may fill with MaxPool2d(2) of the result (pool.written tells)."""
        B, C, H, W = x.shape
        dev = x.device
        if self.extra_residual is not None:
            er = self.extra_residual(x)
            ops.require_device(er, "extra_residual output")
            if tuple(er.shape) != tuple(x.shape):
                raise ValueError("extra_residual must preserve the shape of its input")
            saved, self.extra_residual = self.extra_residual, None
            try:
                y, _ = self._res(blk, x, shift, pk, ws, res2=None, xs=xs, want_stats=False)
            finally:
                self.extra_residual = saved
            ops.add(y, er.contiguous(), out=y)                      # (conv2 + x) + extra_residual(x)
            if res2 is not None:
                ops.add(y, res2, out=y)                             # x + xa of bottom_forward, after the block as in the reference
            if out_amax is not None:
                ops.absmax_rows(y, out=out_amax)
            return y, None                                          # no tile statistics of the sum: the consumer normalises standalone
        if isinstance(shift, _FieldShifts):                # a field of time shifts: conv1's epilogue adds it as a residual
            yt = self._field_shift(blk, shift, H, W)
            got = self._res_body(blk, x, None, yt, pk, ws, res2, xs, want_stats, out_amax, pool)
            ws.give(yt)
            return got
        yt = None
        if shift is not None and shift.dim() == 4:         # the same, handed over as a tensor [B, C, He, We]
            f = corner_pool_factor(shift.shape[2:], (H, W))
            yt, shift = (shift if f == 1 else shift[:, :, ::f, ::f].contiguous()), None
        return self._res_body(blk, x, shift, yt, pk, ws, res2, xs, want_stats, out_amax, pool)

    def _res_body(self, blk, x, shift, yt, pk, ws, res2, xs, want_stats, out_amax, pool=None):
        B, C, H, W = x.shape
        dev = x.device
        k1, k2 = self.norm_kinds                           # 0 GroupLN, 1 GroupRMS, 2 none, 3 GroupPix (not a table)
        w1, b1 = getattr(blk.gnorm1, "weight", None), getattr(blk.gnorm1, "bias", None)
        w2, b2 = getattr(blk.gnorm2, "weight", None), getattr(blk.gnorm2, "bias", None)
        # The folded route: the table carries the sample's activation exponent in its fourth column (a bound on the activation's
        # argument from the statistics), and the loader produces SiLU(norm(x)) times that power of two -- inside the fp16x3 window
        # whatever the affine parameters or an eps-dominated variance do.  The image / standalone routes below rely on the norm to put its output in the window:
        # real norms with affine parameters of ordinary size (windowed); otherwise the activation's exponent is measured.
        if (self._fused() and xs is not None and (C + 63) // 64 <= self.fuse_max_cot and k1 != 3 and k2 != 3
                and self.config.kernel_size == 3):                                  # the norm+SiLU loader is the 3x3 kernel's
            tab = ws.take((B, ops.table_channels(C), 4), dev)
            ops.inorm_table(xs, w1, b1, k1, H * W, eps=1e-5, out=tab)
            ys = self._stats_buf(ws, B, C, H, W, dev)
            y = self._conv(blk.conv1, x, pk, shift=shift, res1=yt, prenorm=tab, tile_stats=ys, out=ws.take(x.shape, dev))
            ops.inorm_table(ys, w2, b2, k2, H * W, eps=1e-5, out=tab)
            os_ = self._stats_buf(ws, B, C, H, W, dev) if want_stats else None
            out = self._conv(blk.conv2, y, pk, res1=x, res2=res2, prenorm=tab, tile_stats=os_, out=ws.take(x.shape, dev),
                             out_amax=out_amax, **({} if pool is None else {"pool": pool}))
            ws.give(y)
            ws.give(ys)
            ws.give(tab)
            return out, os_
        windowed = k1 in (0, 1) and k2 in (0, 1) and self._norms_in_window(blk)
        if windowed and self._norm_images_ok(blk, C, H, W, k1, k2):
            # standalone norms (the 256-channel level): written as the convolution's pre-split fp16 images, which it stages by
            # LDS-DMA -- same bytes as the fp32 result, bit-identical values, no split in the convolution (ops.conv_img)
            img = ops.inorm_silu_images(x, w1, b1, k1, eps=1e-5, out=ws.take((ops.conv_images_floats(B, C, H, W),), dev))
            y = ops.conv_img(img, pk[id(blk.conv1)], B, C, H, W, bias=blk.conv1.bias, shift=shift, res1=yt, out=ws.take(x.shape, dev))
            ops.inorm_silu_images(y, w2, b2, k2, eps=1e-5, out=img)
            os_ = self._stats_buf(ws, B, C, H, W, dev) if want_stats else None
            out = ops.conv_img(img, pk[id(blk.conv2)], B, C, H, W, bias=blk.conv2.bias, res1=x, res2=res2, tile_stats=os_,
                               out=ws.take(x.shape, dev), out_amax=out_amax, pool=pool)
            ws.give(img)
            ws.give(y)
            return out, os_
        if windowed and self._table_images_ok(blk, C, k1, k2) and self._fused() and xs is not None:
            # planes the image norm kernel does not take (more than 4096 floats): the activation from the fused loader's table
            # (built from the producer's tile statistics), written as images by an apply pass
            tab = ws.take((B, ops.table_channels(C), 4), dev)
            ops.inorm_table(xs, w1, b1, k1, H * W, eps=1e-5, out=tab)
            img = ops.table_apply_images(x, tab, out=ws.take((ops.conv_images_floats(B, C, H, W),), dev))
            ys = self._stats_buf(ws, B, C, H, W, dev)
            y = ops.conv_img(img, pk[id(blk.conv1)], B, C, H, W, bias=blk.conv1.bias, shift=shift, res1=yt, tile_stats=ys,
                             out=ws.take(x.shape, dev))
            ops.inorm_table(ys, w2, b2, k2, H * W, eps=1e-5, out=tab)
            ops.table_apply_images(y, tab, out=img)
            os_ = self._stats_buf(ws, B, C, H, W, dev) if want_stats else None
            out = ops.conv_img(img, pk[id(blk.conv2)], B, C, H, W, bias=blk.conv2.bias, res1=x, res2=res2, tile_stats=os_,
                               out=ws.take(x.shape, dev), out_amax=out_amax, pool=pool)
            for t in (img, y, ys, tab):
                ws.give(t)
            return out, os_
        # standalone norms; the activation's exponent is measured (one reduction pass) unless the norm puts it in the window
        a = ops.inorm_silu(x, w1, b1, kind=k1, eps=1e-5, out=ws.take(x.shape, dev))
        y = self._conv(blk.conv1, a, pk, shift=shift, res1=yt, out=ws.take(x.shape, dev), in_amax=self._act_amax(a, windowed))
        ops.inorm_silu(y, w2, b2, kind=k2, eps=1e-5, out=a)
        os_ = self._stats_buf(ws, B, C, H, W, dev) if want_stats else None
        self._conv(blk.conv2, a, pk, res1=x, res2=res2, tile_stats=os_, out=y, in_amax=self._act_amax(a, windowed), out_amax=out_amax)
        ws.give(a)
        return y, os_

    def _consumes_stats(self, blk, C, H, W):
        """Does _res(blk, x [., C, H, W], xs=...) read the tile statistics of its input?  (The folded-loader route and the
        table -> images route do; the image route and the standalone norms compute their own.)  Producers ask before they spend
        epilogue work on statistics nobody reads: at config 2 that was every launch of the 256-channel level, the last block of
        every level (its result feeds a Down / UpSampler) and the attention's output projection."""
        if blk is None or not self._fused() or self.extra_residual is not None:
            return False
        k1, k2 = self.norm_kinds
        if (C + 63) // 64 <= self.fuse_max_cot and k1 != 3 and k2 != 3 and self.config.kernel_size == 3:
            return True
        windowed = k1 in (0, 1) and k2 in (0, 1) and self._norms_in_window(blk)
        if windowed and self._norm_images_ok(blk, C, H, W, k1, k2):
            return False
        return windowed and self._table_images_ok(blk, C, k1, k2)

    def _act_amax(self, a, windowed):
        """in_amax of a standalone norm + SiLU output: none needed inside the fp16x3 window, else a reduction into an arena row
        (a row of the current forward's arena; outside a forward -- never -- ops reduces into a fresh tensor)."""
        if windowed or self.conv_precision != "fp16x3":
            return ops.NORMALISED
        return self._am.of(a) if self._am is not None else None

    def _norms_in_window(self, blk):
        """Both norms of the block are affine-free or carry affine parameters of ordinary size (|w|, |b| largest entries within
        [2^-6, 2^6] / below 2^6): SiLU(norm(x) * w + b) then sits inside the fp16x3 window (|x| in [2^-3, 2^16) at 22 bits,
        degrading gracefully to 2^-25 absolute) for any input magnitude.  Checked on the host once per parameter version."""
        return precision.norms_in_window(self._window_cache, id(blk), (blk.gnorm1, blk.gnorm2))

    def _images_ok(self, blk, C, k1, k2, kinds):
        """The norms of this block (kinds k1, k2 among `kinds`) can hand their convolutions pre-split images: fp16x3 3x3
        convolutions with zero padding that keep the channel count, an even number of 16-channel chunks."""
        return (getattr(self, "norm_images", True) and self.conv_precision == "fp16x3" and not self.circular
                and self.config.kernel_size == 3 and k1 in kinds and k2 in kinds and ((C + 15) // 16) % 2 == 0
                and blk.conv1.out_channels == C and blk.conv2.out_channels == C)

    def _table_images_ok(self, blk, C, k1, k2):
        """The table route: any plane size; GroupLN / GroupRMS / no norm."""
        return self._images_ok(blk, C, k1, k2, (0, 1, 2))

    def _norm_images_ok(self, blk, C, H, W, k1, k2):
        """The standalone norms writing images themselves: GroupLN / GroupRMS, planes the image kernel takes."""
        return self._images_ok(blk, C, k1, k2, (0, 1)) and ops.inorm_silu_images_supported(H, W)

    def forward_with_shifts(self, x, shifts, row=None, out=None):
        """UNet body given the per-block time shifts.  shifts[k] is [M, C_k]; row selects one row
        shared by the whole batch (sampling: sigma is a per-step constant), row=None means one row
        per sample (M == B); or a field of shifts (`field_shifts`), given back here.  Fields [B, C, H, W] and volumes
        [B, C, D, H, W] take the same walk; what it launches is the dimension's answer (`_Fields`, `_Volumes`)."""
        require_eval(self, self.config.dropout, self.config.cond_dropout, self.config.cond_drop)
        self.check_field_size(x.shape)
        try:
            d = (_Volumes if self.dim == 3 else _Fields)(self, x, shifts, row)
            return self._walk(d, x.contiguous() if self.dim == 3 else x, out)
        finally:
            if self._am is not None:                       # the arena a field pass set for its launches
                self._am.release()
                self._am = None
            if isinstance(shifts, _FieldShifts):
                shifts.release()

    def _walk(self, d, x, out):
        """The network once (punetg.py:356-416): levels, skip stack, bottom group with x + xa folded into the attention group's
        last launch, output layer.  An activation is a record (tensor, the statistics its producer left or None, the amax row
        its producer filled or None), and every producer is told who consumes its result (`to`): the residual block that will
        normalise it, the module of the raw-input launch that reads it as it is (Down / UpSampler, attention, output layer), or
        None for anything else.  Whether that earns statistics or a row is the dimension's business.  Every buffer comes from
        the workspace -- the sampler's planner captures this as a hipGraph -- and goes back as soon as its reader has run."""
        ws, cfg = self._ws, self.config
        B, dev, sides = x.shape[0], x.device, tuple(x.shape[2:])

        def give(a):
            ws.give(a[0])
            if a[1] is not None:
                ws.give(a[1])

        def chain(blocks, a, to):
            """a through residual blocks, each input given back once its block has run; `to` consumes the last result."""
            for j, blk in enumerate(blocks):
                a2 = d.res(blk, a, blocks[j + 1] if j + 1 < len(blocks) else to)
                give(a)
                a = a2
            return a

        xe = None
        if not cfg.bias:                                                             # punetg.py:390-394
            ones = ws.take((B, 1) + sides, dev)
            ones.fill_(1.0)
            xe = ops.concat2(x, ones, out=ws.take((B, x.shape[1] + 1) + sides, dev))
            ws.give(ones)
            x = xe
        ndown, nup = len(self.downward_blocks), len(self.upward_blocks)
        bottom = list(self.before_block) + list(self.attn_resnet_block) + list(self.after_block)
        # who reads the bottom's result raw: the first UpSampler.  (A network without levels hands it to the output layer, which
        # reduces its input itself: None.)
        rest = self.upsamplers[0] if ndown else None

        def entering(lv):                                                            # the block that normalises what enters level lv
            if lv < ndown and len(self.downward_blocks[lv]):
                return self.downward_blocks[lv][0]
            return bottom[0] if bottom else None
        if isinstance(self.convin, _FourierInput):                                   # no producer statistics: standalone first norm
            a = ops.fourier_channels(x, self.convin.W, out=ws.take((B, cfg.model_channels) + sides, dev)), None, None
        else:
            a = d.conv_in(x, entering(0))
        if xe is not None:
            ws.give(xe)
        skips = []
        for lv, blocks in enumerate(self.downward_blocks):                          # punetg.py:356-365
            a = chain(blocks, a, self.downsamplers[lv])
            skips.append(a[0])
            if a[1] is not None:
                ws.give(a[1])                                                        # the skip is only added, never normalised
            a = d.down(self.downsamplers[lv], a, entering(lv + 1))
        nbefore, nattn, nafter = len(self.before_block), len(self.attn_resnet_block), len(self.after_block)
        # punetg.py:378-387.  Without an attention group x + x follows, which reads no statistics (and, between blocks, no row)
        a = chain(self.before_block, a, self.attn_resnet_block[0] if nattn else (None if nafter else rest))
        xa = a
        for i, blk in enumerate(self.attn_resnet_block):
            last = i == nattn - 1
            att = self.attn_block[i] if i < len(self.attn_block) else None
            after = bottom[nbefore + i + 1] if nbefore + i + 1 < len(bottom) else rest
            # x + xa is folded into the last residual block's epilogue when no attention follows it
            xa2 = d.res(blk, xa, after if att is None else att, res2=a[0] if (last and att is None) else None)
            if xa is not a:
                give(xa)
            xa = xa2
            if att is not None:
                xa2 = d.attn(att, xa, after, res2=a[0] if last else None)
                give(xa)
                xa = xa2
        if nattn == 0:
            xa = ops.add(a[0], a[0], out=ws.take(a[0].shape, dev)), None, None
        give(a)
        a = chain(self.after_block, xa, rest)
        for lv, blocks in enumerate(self.upward_blocks):                             # punetg.py:367-376
            skip = skips.pop()
            a2 = d.up(self.upsamplers[lv], a, skip, blocks[0] if len(blocks) else None)
            give(a)
            ws.give(skip)
            a = chain(blocks, a2, self.upsamplers[lv + 1] if lv + 1 < nup else self.convout)
        y = d.out(a, out)
        give(a)
        return y

    def _attention(self, att, x, pk, ws, res2=None, tile_stats=None, in_amax=None, out_amax=None):
        """TwoDimensionalAttention.forward (attention.py:67-72,82-90), channel-major throughout.  The block's three launches
        read raw tensors: x (in_amax: its producer's row, or None = reduced here), qkv and the attention output, whose
        exponents travel from epilogue to loader through rows of the forward's arena."""
        m = att.mhattn
        in_bias = None if self.inhouse_attn else m.in_proj_bias    # the in-house attention has no biases
        out_bias = None if self.inhouse_attn else m.out_proj.bias
        am = self._am if self.conv_precision == "fp16x3" else None
        own = None
        if am is None and self.conv_precision == "fp16x3":           # called outside forward_with_shifts (the 3-D path sets its own)
            own = am = AmaxArena(ws, x.shape[0], x.device)
        E, heads = x.shape[1], getattr(m, "num_heads", 1)
        folded = None
        if self.attn_fold:
            # the unfolded packings stand in for the folded ones (same kind) to ask whether the route is taken at all
            probe = runtime.FoldedAttention(pk[(id(att), "in")], None, pk[(id(att), "out")], None)
            if runtime.attention_folds(probe, E, x.shape[2] * x.shape[3], heads, self.conv_precision, self.cosine_attn):
                folded = self._folded_attention(att)
        y = runtime.attention(x, pk[(id(att), "in")], in_bias, pk[(id(att), "out")], out_bias, E=E,
                              heads=heads, precision=self.conv_precision, ws=ws, am=am, in_amax=in_amax,
                              out_amax=out_amax, res1=x if self.config.attn_residual else None, res2=res2, tile_stats=tile_stats,
                              cosine=self.cosine_attn, folded=folded)
        if own is not None:
            own.release()
        return y

    def _folded_attention(self, att):
        """runtime.FoldedAttention of one attention block (fp16x3 packings of M = Wk^T Wq and W' = Wo Wv with their biases, formed in
        fp64 from the weights packed_weights() reads), built on first use of the folded route and kept until a projection weight
        or bias changes.  Not an entry of packed_weights(): the route is taken by some shapes only."""
        m = att.mhattn
        if self.inhouse_attn:
            tracked = [m.q_proj_matrix, m.k_proj_matrix, m.v_proj_matrix, m.o_proj_matrix]
        else:
            tracked = [t for t in (m.in_proj_weight, m.out_proj.weight, m.in_proj_bias, m.out_proj.bias) if t is not None]
        sig = weights_signature(tracked, self.conv_precision)
        cache = self.__dict__.setdefault("_attn_folded", {})
        hit = cache.get(id(att))
        if hit is not None and hit[0] == sig:
            return hit[1]
        with torch.no_grad():
            if self.inhouse_attn:
                (w_in, w_out), b_in, b_out = m.projection_weights(), None, None
            else:
                w_in, w_out, b_in, b_out = m.in_proj_weight, m.out_proj.weight, m.in_proj_bias, m.out_proj.bias
            E = m.embed_dim
            M, c, Wp, bp = runtime.fold_attention_weights(w_in, b_in, w_out, b_out)
            f32 = lambda t: None if t is None else t.float().contiguous()
            folded = runtime.FoldedAttention(ops.pack_conv(f32(M).reshape(E, E, 1, 1), "fp16x3"), f32(c),
                                             ops.pack_conv(f32(Wp).reshape(E, E, 1, 1), "fp16x3"), f32(bp))
        cache[id(att)] = (sig, folded)
        return folded


def _shift_source(shifts, row, B):
    """-> sh(), the next residual block's time shift: tabulated shifts in block order, row `row` of each (runtime.shift_rows);
    a field of shifts goes to every block as it is, and the block evaluates its own (PUNetG._field_shift)."""
    if isinstance(shifts, _FieldShifts):
        return lambda: shifts
    it = iter(shifts)
    return lambda: shift_rows(next(it), row, B)


class _Fields:
    """What PUNetG._walk launches on [B, C, H, W] fields.  Every activation travels with the tile statistics its producer left --
    asked for only where the consuming block reads them (`_consumes_stats`) -- and, where it feeds a raw-input launch, with an
    amax row.  Activation exponents (ops.py): every launch that reads a tensor which no norm has put into the fp16x3 window --
    convin, the Down / UpSamplers, the attention and its projections, a k x k output layer -- takes the per-sample max |x| its
    producer's epilogue left in a row of the pass's arena, or a reduction over the tensor where the producer is not one of our
    epilogues (the network input) or left none."""

    def __init__(self, net, x, shifts, row):
        if net.pool_route not in POOL_ROUTES:
            raise ValueError(f"pool_route {net.pool_route!r}; choose from {POOL_ROUTES}")
        self.net, self.pk, self.ws = net, net.packed_weights(), net._ws
        self.B, self.dev = x.shape[0], x.device
        self.sh = _shift_source(shifts, row, self.B)       # a field handed over as a tensor allocates: not for captured runs
        self.h3 = net.conv_precision == "fp16x3"
        # (the arena is zeroed by the input layer's own reduction launch when that is the first thing the forward does)
        lazy = self.h3 and not isinstance(net.convin, _FourierInput) and not net.exact_input_layer
        self.am = net._am = AmaxArena(self.ws, self.B, self.dev, zero=not lazy) if self.h3 else None
        self.direct_out = net._out_is_direct(net.convout)
        self.pool = None                                    # "epilogue": the PoolOut a level's last block may have filled

    def stats(self, to, C, H, W):
        """A statistics buffer for a [B, C, H, W] result, only if its consumer reads it."""
        if not self.net._consumes_stats(to if isinstance(to, _ResBlock) else None, C, H, W):
            return None
        return self.net._stats_buf(self.ws, self.B, C, H, W, self.dev)

    def row(self, to):
        """A zeroed amax row for a result that feeds a raw-input launch (the direct output layer computes in fp32: none)."""
        raw = to is not None and not isinstance(to, _ResBlock) and not (to is self.net.convout and self.direct_out)
        return self.am.row() if (self.h3 and raw) else None

    def amax_of(self, a):
        """The row that travels with a, else a reduction."""
        if not self.h3:
            return None
        return a[2] if a[2] is not None else self.am.of(a[0])

    def plain_down(self, smp):
        """pool_route: this DownSampler as a plain convolution of an already pooled tensor (a 3x3 fp16x3 packing only)."""
        pw = self.pk[id(smp.conv)]
        return (self.net.factor == 2 and self.h3 and self.net.pool_route != "loader" and pw.kind == "fp16x3" and pw.ks == 3
                and pw.subs is None)

    def conv_in(self, x, to):
        net, m = self.net, self.net.convin
        shape = (self.B, m.out_channels) + tuple(x.shape[2:])
        if self.h3 and net.exact_input_layer:
            # the input's channels are too far apart in magnitude for one exponent per sample (precision.escalate_input):
            # exact-fp32 kernel, no tile statistics (the first block normalises standalone)
            # (circular= : a periodic network with exact_input_layer set by hand must raise -- the exact-fp32 kernel zero-pads)
            return ops.conv(x, self.pk[(id(m), "exact")], bias=m.bias, circular=net.circular_arg, out=self.ws.take(shape, self.dev)), None, None
        hs = self.stats(to, *shape[1:])
        wmax = self.pk.get((id(m), "wmax"))
        return net._conv(m, x, self.pk, tile_stats=hs, out=self.ws.take(shape, self.dev),
                         in_amax=self.am.of_input(x, precision.input_layer_flag(net, self.dev), wmax) if self.h3 else None), hs, None

    def res(self, blk, a, to, res2=None):
        net, (h, hs, _) = self.net, a
        ha = self.row(to)
        if (any(to is s for s in net.downsamplers) and self.plain_down(to) and net.pool_route == "epilogue"
                and not (h.shape[2] % 2 or h.shape[3] % 2)):
            self.pool = ops.PoolOut(self.ws.take((self.B, h.shape[1], h.shape[2] // 2, h.shape[3] // 2), self.dev))
        h2, hs2 = net._res(blk, h, self.sh(), self.pk, self.ws, res2=res2, xs=hs, out_amax=ha, pool=self.pool,
                           want_stats=net._consumes_stats(to if isinstance(to, _ResBlock) else None, *h.shape[1:]))
        return h2, hs2, ha

    def down(self, smp, a, to):
        """DownSampler (max-pool -> conv) of the level's last result, which stays with the caller as the skip."""
        net, ws, f, h, ds = self.net, self.ws, self.net.factor, a[0], smp.conv
        Ho, Wo = h.shape[2] // f, h.shape[3] // f
        hs = self.stats(to, ds.out_channels, Ho, Wo)
        pool, self.pool = self.pool, None
        hp = None
        if pool is not None and pool.written:                                    # "epilogue": the last block's store phase pooled
            hp = pool.tensor
        elif pool is not None:
            ws.give(pool.tensor)                                                 # ... or its launch did not qualify: the loader
        plain = hp is not None or (self.plain_down(smp) and net.pool_route == "pass")
        if hp is None and (plain or f != 2):
            hp = ops.maxpool_f(h, f, out=ws.take((self.B, h.shape[1], Ho, Wo), self.dev))
        # max |maxpool(h)| <= max |h|: the producer's row of the unpooled h stays a valid exponent bound.  plain: the persistent
        # kernel takes the raw-input launch where the shape is its own; factor 2 otherwise: the convolution's loader pools
        kw = {"load_mode": DS_LOAD_MAXPOOL2} if hp is None else ({"pc_raw": True} if plain else {})
        y = net._conv(ds, h if hp is None else hp, self.pk, tile_stats=hs, out=ws.take((self.B, ds.out_channels, Ho, Wo), self.dev),
                      in_amax=self.amax_of(a), **kw)
        if hp is not None:
            ws.give(hp)
        return y, hs, None

    def up(self, smp, a, skip, to):
        """UpSampler (nearest -> conv) + skip; factor 2 upsamples in the convolution's loader."""
        net, ws, f, h = self.net, self.ws, self.net.factor, a[0]
        hs = self.stats(to, *skip.shape[1:])
        # a copy keeps max |h|: the producer's row bounds the upsampled tensor too
        hu = None if f == 2 else ops.upsample_f(h, f, out=ws.take((self.B, h.shape[1]) + tuple(skip.shape[2:]), self.dev))
        y = net._conv(smp.conv, h if hu is None else hu, self.pk, res1=skip, tile_stats=hs, out=ws.take(skip.shape, self.dev),
                      in_amax=self.amax_of(a), **({"load_mode": DS_LOAD_UPSAMPLE2} if hu is None else {}))
        if hu is not None:
            ws.give(hu)
        return y, hs, None

    def attn(self, att, a, to, res2=None):
        hs, ha = self.stats(to, *a[0].shape[1:]), self.row(to)
        return self.net._attention(att, a[0], self.pk, self.ws, res2=res2, tile_stats=hs, in_amax=self.amax_of(a), out_amax=ha), hs, ha

    def out(self, a, out):
        net = self.net
        return net._out_conv(net.convout, a[0], self.pk, out, net.circular_arg, in_amax=None if self.direct_out else self.amax_of(a))


class _Volumes:
    """What PUNetG._walk launches on [B, C, D, H, W] volumes (punetg.py:217-236,389-416 with Conv3d / MaxPool3d / Upsample /
    ThreeDimensionalAttention).  Convolutions: with the default fp16x3 precision three launches of the 2-D matrix-core kernels per
    3x3x3 convolution over a slice-major copy of the volume (ops.conv3d_mfma, which measures activation exponents per slice: no
    amax rows here); otherwise, and for the <= 4-channel output layer, the exact-fp32 direct kernel (ops.conv3d) -- both with the
    pooling / upsampling / skip / residual / time-shift fusions of the 2-D path.  Per-(sample, channel) norms over D*H*W, attention
    over the flattened voxels.

    Norm folding (fp16x3, 3x3x3 kernels, zero or periodic padding): every activation travels with the partial sums its producer's
    slice -> volume copy left; a block whose input has them runs ops.resblock3d_fused -- norm1 inside the volume -> slice copy,
    the intermediate slice-major with norm2 in conv2's loader -- 20 instead of 52 bytes per element of norm / copy traffic per
    block.  Without statistics (after the thin input layer or the attention) the block runs the standalone norms and leaves
    statistics for its successor.  Every producer but the one before the output layer leaves them.  Not with a field of shifts:
    resblock3d_fused adds one shift per channel, so those blocks run the standalone norms."""

    def __init__(self, net, x, shifts, row):
        if x.dim() != 5:
            raise ValueError("a dimension=3 network takes [B, C, D, H, W] volumes")
        self.net, self.pk, self.ws = net, net.packed_weights(), net._ws
        self.B, self.dev = x.shape[0], x.device
        self.sh = _shift_source(shifts, row, self.B)
        self.field = shifts if isinstance(shifts, _FieldShifts) else None
        k1, k2 = net.norm_kinds
        self.fold = (net._fused() and net.extra_residual is None and k1 != 3 and k2 != 3 and net.config.kernel_size == 3
                     and self.field is None)

    def stats_buf(self, shape):
        Bc, C, D, H, W = shape
        return self.ws.take((Bc, C, ops.volume_stat_tiles(D, H * W), 4), self.dev)

    def conv(self, m, h, load_mode=0, dst=None, fresh=False, want_stats=False, normalised=False, **kw):
        """-> an activation.  Every buffer comes from the workspace (a captured loop must not allocate); fresh: the caller's
        result.  normalised: h is a norm + SiLU output inside the fp16x3 window; otherwise the matrix-core route measures
        per-slice activation exponents on its slice copy (ops.conv3d_mfma)."""
        net, pk = self.net, self.pk
        f = {0: (1, 1), DS_LOAD_MAXPOOL2: (1, 2), DS_LOAD_UPSAMPLE2: (2, 1)}[load_mode]
        shape = (h.shape[0], m.out_channels) + tuple(v * f[0] // f[1] for v in h.shape[2:])
        if dst is None and not fresh:
            dst = self.ws.take(shape, self.dev)
        packs = pk.get((id(m), "3d"))
        # fp16x3 (default): three 2-D MFMA launches per convolution -- 0.30 vs 1.33 ms at 64 -> 64 channels, 8 x 32^3;
        # the thin input / output layers stay on the direct kernel (0.08 vs 0.14 ms for 1 -> 64)
        k = m.weight.shape[-1]
        if packs is None and k != 3:
            raise NotImplementedError(f"{k}x{k}x{k} kernels on volumes are implemented on the fp16x3 convolution only "
                                      f"(conv_precision={net.conv_precision!r})")
        if packs is not None and ((m.out_channels > 4 and m.in_channels > 4) or k != 3):
            st = self.stats_buf(shape) if (self.fold and want_stats) else None
            return ops.conv3d_mfma(h, packs, bias=m.bias, circular=net.circular_arg, load_mode=load_mode, out=dst, ws=self.ws,
                                   out_stats=st, in_amax=ops.NORMALISED if normalised else None, **kw), st, None
        return ops.conv3d(h, pk.get((id(m), "eff"), m.weight), bias=m.bias, circular=net.circular_arg, load_mode=load_mode,
                          out=dst, **kw), None, None

    def conv_in(self, x, to):
        return self.conv(self.net.convin, x, want_stats=True)

    def res(self, blk, a, to, res2=None):                                         # ResnetBlockC.forward; the input untouched
        net, pk, ws, B, dev = self.net, self.pk, self.ws, self.B, self.dev
        h, hs, _ = a
        want_stats = to is not net.convout                                        # no norm follows
        k1, k2 = net.norm_kinds
        w1, b1 = getattr(blk.gnorm1, "weight", None), getattr(blk.gnorm1, "bias", None)
        w2, b2 = getattr(blk.gnorm2, "weight", None), getattr(blk.gnorm2, "bias", None)
        C = h.shape[1]
        p1, p2 = pk.get((id(blk.conv1), "3d")), pk.get((id(blk.conv2), "3d"))
        windowed = k1 in (0, 1) and k2 in (0, 1) and net._norms_in_window(blk)
        if (self.fold and windowed and hs is not None and p1 is not None and p2 is not None and C > 4
                and (C + 63) // 64 <= net.fuse_max_cot):
            tab = ops.inorm_table(hs, w1, b1, k1, h[0, 0].numel(), eps=1e-5, out=ws.take((B, ops.table_channels(C), 4), dev))
            os_ = self.stats_buf(h.shape) if want_stats else None
            y = ops.resblock3d_fused(h, tab, p1, blk.conv1.bias, self.sh(), p2, blk.conv2.bias, w2, b2, k2, res2=res2,
                                     out=ws.take(h.shape, dev), out_stats=os_, ws=ws, circular=net.circular_arg)
            ws.give(tab)
            return y, os_, None
        act = ops.inorm_silu(h, w1, b1, kind=k1, eps=1e-5, out=ws.take(h.shape, dev))
        if self.field is not None:     # every block evaluates its own per-voxel shift and adds it as conv1's residual
            yt = net._field_shift(blk, self.field, *h.shape[2:])
            y = self.conv(blk.conv1, act, res1=yt.view((B, blk.conv1.out_channels) + tuple(h.shape[2:])), normalised=windowed)[0]
            ws.give(yt)
        else:
            y = self.conv(blk.conv1, act, shift=self.sh(), normalised=windowed)[0]
        ops.inorm_silu(y, w2, b2, kind=k2, eps=1e-5, out=act)
        if net.extra_residual is None:
            os_ = self.conv(blk.conv2, act, res1=h, res2=res2, dst=y, want_stats=want_stats, normalised=windowed)[1]
        else:
            self.conv(blk.conv2, act, res1=h, dst=y, normalised=windowed)
            ops.add(y, net.extra_residual(h).contiguous(), out=y)
            if res2 is not None:
                ops.add(y, res2, out=y)
            os_ = None
        ws.give(act)
        return y, os_, None

    def down(self, smp, a, to):
        h, f = a[0], self.net.factor
        if f == 2:
            return self.conv(smp.conv, h, load_mode=DS_LOAD_MAXPOOL2, want_stats=True)
        hp = ops.maxpool_f(h, f, out=self.ws.take(tuple(h.shape[:2]) + tuple(v // f for v in h.shape[2:]), self.dev))
        y = self.conv(smp.conv, hp, want_stats=True)                              # pooled volume, then the plain convolution
        self.ws.give(hp)
        return y

    def up(self, smp, a, skip, to):
        h, f = a[0], self.net.factor
        if f == 2:
            return self.conv(smp.conv, h, load_mode=DS_LOAD_UPSAMPLE2, res1=skip, want_stats=True)
        hu = ops.upsample_f(h, f, out=self.ws.take(tuple(h.shape[:2]) + tuple(skip.shape[2:]), self.dev))
        y = self.conv(smp.conv, hu, res1=skip, want_stats=True)
        self.ws.give(hu)
        return y

    def attn(self, att, a, to, res2=None):                                        # ThreeDimensionalAttention
        h = a[0]
        Bq, E, D, H, W = h.shape
        r2 = None if res2 is None else res2.view(Bq, E, D * H, W)
        y = self.net._attention(att, h.view(Bq, E, D * H, W), self.pk, self.ws, res2=r2)
        o = self.ws.take(h.shape, self.dev)
        o.copy_(y.view(h.shape))
        self.ws.give(y)
        return o, None, None

    def out(self, a, out):
        return self.conv(self.net.convout, a[0], dst=out, fresh=out is None)[0]


class PUNetGCond(PUNetG):
    """PUNetG with channel-concatenated conditioning (punetg.py:706-735): the fields y[item] for item in
    ``channel_conditional_items`` are appended to x as input channels (config.input_channels counts them);
    the remaining entries of y go to the conditional embedding.  Like the reference it needs y on every call,
    so it cannot run the unconditional branch of classifier-free guidance (guidance must be 1)."""

    def __init__(self, config: PUNetGConfig, conditional_embedding: torch.nn.Module | None = None,
                 channel_conditional_items: list[str] | None = False, extra_residual: torch.nn.Module | None = None):
        super().__init__(config, conditional_embedding, extra_residual=extra_residual)
        self.channel_conditional_items = channel_conditional_items
        self._ycat = None
        self._ycat_static = {}       # (shape, device) -> buffer holding the concatenated channel fields

    def drop_caches(self):
        super().drop_caches()
        self._ycat, self._ycat_static = None, {}

    def export_description(self) -> dict[str, Any]:
        args = super().export_description()
        args["channel_conditional_items"] = self.channel_conditional_items
        return args

    def _split_condition(self, y):
        if y is None:
            raise TypeError("PUNetGCond needs the condition dictionary y on every call (punetg.py:721-723)")
        fields = [y[item] for item in self.channel_conditional_items]
        rest = {k: v for k, v in y.items() if k not in self.channel_conditional_items}
        for f in fields:
            ops.require_device(f, "channel condition")
            if f.dim() < 3 or tuple(f.shape[2:]) != tuple(fields[0].shape[2:]) or f.shape[0] != fields[0].shape[0]:
                raise ValueError("channel condition fields must be [B or 1, C_i, *spatial] with equal batch and spatial sizes")
        # torch.cat([y[item] ...], dim=1) of punetg.py:724-727 INTO a buffer the network owns: a captured sampling
        # loop reads the fields at this address on every replay, so the caller's tensors (new ones on every call of
        # autoregressive_sample; temporaries of torch.cat) must never be what the graph points at.  One buffer per
        # (shape, device); every call -- eager or as the refresh before a replay -- rewrites it.
        shape = (fields[0].shape[0], sum(f.shape[1] for f in fields)) + tuple(fields[0].shape[2:])
        key = (shape, str(fields[0].device))
        buf = self._ycat_static.get(key)
        if buf is None:                  # never evicted: captured plans keep reading the buffer of their shape
            with torch.inference_mode(False):          # a normal tensor: written under inference_mode and outside it
                buf = torch.empty(shape, dtype=torch.float32, device=fields[0].device)
            self._ycat_static[key] = buf
        c0 = 0
        for f in fields:
            buf[:, c0:c0 + f.shape[1]].copy_(f)
            c0 += f.shape[1]
        return (rest if len(rest) else None), buf

    def _with_condition(self, x, ycat, ws):
        B = x.shape[0]
        yexp = None
        if ycat.shape[0] == 1 and B > 1:
            # broadcast into a WORKSPACE buffer: a temporary from torch's allocator would be freed right after the
            # capture while the graph keeps writing to its address on every replay
            yexp = ws.take((B,) + tuple(ycat.shape[1:]), x.device)
            yexp.copy_(ycat.expand(B, *ycat.shape[1:]))
            ycat = yexp
        elif ycat.shape[0] != B:
            raise ValueError("channel condition batch must be 1 or match x")
        out = ops.concat2(x, ycat, out=ws.take((B, x.shape[1] + ycat.shape[1]) + tuple(x.shape[2:]), x.device))
        if yexp is not None:
            ws.give(yexp)
        return out

    @ops.device_guard
    def forward(self, x, t, y=None):
        out = self.forward_unguarded(x, t, y)
        if precision.needs_escalation(self, out, x, self._ycat):
            precision.escalate(self)
            out = self.forward_unguarded(x, t, y)
        return out

    @ops.device_guard
    def forward_unguarded(self, x, t, y=None):
        ops.require_device(x, "x")
        self.check_field_size(x.shape)
        rest, self._ycat = self._split_condition(y)
        shifts = self._eager_shifts(x, t, PUNetG.embed_condition(self, rest))
        return self.forward_with_shifts(x.contiguous(), shifts, row=None)

    def embed_condition(self, y):
        """Planned sampler entry: remember the channel fields, embed what is left of y."""
        rest, self._ycat = self._split_condition(y)
        return PUNetG.embed_condition(self, rest)

    def forward_with_shifts(self, x, shifts, row=None, out=None):
        if self._ycat is None:
            raise TypeError("PUNetGCond needs the condition dictionary y on every call (punetg.py:721-723)")
        self.check_field_size(x.shape)
        xc = self._with_condition(x, self._ycat, self._ws)
        try:
            return super().forward_with_shifts(xc, shifts, row=row, out=out)
        finally:
            self._ws.give(xc)
