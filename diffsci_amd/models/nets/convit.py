"""ConVit score network on HIP kernels (reference: diffsci/models/nets/convit.py).

Same constructors, public attributes, ``net(x, t, y)`` protocol and state_dict keys as the reference's ``ConVit`` / ``ConVitBlock``
/ ``ConVitConfig`` (convit.py:15-98, 536-735), so its checkpoints load with strict=True (the ``attention.scale`` buffer included).
The torch.nn layers are parameter containers only; every tensor operation of a block is a launch into libdiffsci_hip.so on
[B, E, H, W] fp32:

  norm_1 / norm_2 / normout + the embedding row (+ AvgPool(f))   ds_channel_rmsnorm
  q | k | v, out projection, pointwise_conv, ffn, convin/convout ds_conv1x1_h3 / ds_conv2d_h3 (fp16x3) or ds_conv2d (exact fp32)
  rope_layer on q and k                                          ds_rope2d
  attention core                                                 ds_attention_h3_heads / ds_attention_heads_generic
  upsample (bilinear x f)                                        ds_upsample_bilinear
  conv_activation(depthwise_conv)                                ds_depthwise_conv_silu
  SiLU(linear_in) * linear_gate                                  ds_swiglu
  (1 - s) * x + s * x_conv + x0                                  ds_convit_blend
  time_embedding, embedding_projection                           ds_fourier_features, ds_linear (+ torch's RMSNorm arithmetic, once per run)

One reference quirk is kept: ``ConVit(config)`` with ``has_conditional_embedding=False`` raises TypeError
(``isinstance(conditional_embedding, None)``, convit.py:715) -- the reference can only be built with a conditional embedding
module, and runs unconditionally with ``y=None``.

The embedding path depends on the noise level and the condition only, so KarrasModule evaluates it once per run for all
evaluations (``embed_condition`` -> ``embed_time`` -> ``time_shifts``: one [M, E] table per block) and the captured sampler calls
``forward_with_shifts`` with a row index.  Every fp16x3 launch takes a per-sample activation exponent from the kernel that
produced its input (``out_amax`` of the norms, RoPE, the attention, the depthwise SiLU, the gate); the slots are rows of one arena
per forward pass, zeroed by one launch."""
import math
import pathlib
from typing import Any, Optional

import torch
import yaml

from ... import ops
from . import runtime
from .punetg import _Fourier
from .runtime import AmaxArena, Workspace, weights_signature


class ConVitConfig(object):
    def __init__(self,
                 in_channels: int = 1,
                 embed_dim: int = 64,
                 num_pos_dims: int = 2,
                 out_channels: Optional[int] = None,
                 num_layers: int = 6,
                 num_heads: int = 8,
                 ffn_expansion_factor: int = 4,
                 attn_compression_factor: int = 2,
                 rope_freq: float = 1.0,
                 with_conv_on_upsample: bool = False,
                 with_conv_on_downsample: bool = False,
                 kernel_size_conv: int = 1,
                 kernel_size_in_out: int = 1,
                 kernel_size_depthwise: int = 3,
                 has_time_embedding: bool = False,
                 has_conditional_embedding: bool = False,
                 fourier_projection_scale: float = 30.0,
                 relative_positioning: bool = False,
                 linear_attention: bool = False,
                 input_batch_norm: bool = False,
                 condition_dropout: float = 0.1):
        self.in_channels = in_channels
        self.embed_dim = embed_dim
        self.num_pos_dims = num_pos_dims
        self.out_channels = out_channels
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.ffn_expansion_factor = ffn_expansion_factor
        self.attn_compression_factor = attn_compression_factor
        self.rope_freq = rope_freq
        self.with_conv_on_upsample = with_conv_on_upsample
        self.with_conv_on_downsample = with_conv_on_downsample
        self.kernel_size_conv = kernel_size_conv
        self.kernel_size_in_out = kernel_size_in_out
        self.kernel_size_depthwise = kernel_size_depthwise
        self.has_time_embedding = has_time_embedding
        self.has_conditional_embedding = has_conditional_embedding
        self.fourier_projection_scale = fourier_projection_scale
        self.relative_positioning = relative_positioning
        self.linear_attention = linear_attention
        self.input_batch_norm = input_batch_norm
        self.condition_dropout = condition_dropout

    def export_description(self) -> dict[str, Any]:
        return dict(
            in_channels=self.in_channels,
            embed_dim=self.embed_dim,
            num_pos_dims=self.num_pos_dims,
            out_channels=self.out_channels,
            num_layers=self.num_layers,
            num_heads=self.num_heads,
            ffn_expansion_factor=self.ffn_expansion_factor,
            attn_compression_factor=self.attn_compression_factor,
            rope_freq=self.rope_freq,
            with_conv_on_upsample=self.with_conv_on_upsample,
            with_conv_on_downsample=self.with_conv_on_downsample,
            kernel_size_conv=self.kernel_size_conv,
            kernel_size_depthwise=self.kernel_size_depthwise,
            kernel_size_in_out=self.kernel_size_in_out,
            has_time_embedding=self.has_time_embedding,
            has_conditional_embedding=self.has_conditional_embedding,
            fourier_projection_scale=self.fourier_projection_scale,
            relative_positioning=self.relative_positioning,
            linear_attention=self.linear_attention,
            input_batch_norm=self.input_batch_norm,
            condition_dropout=self.condition_dropout,
        )

    @property
    def has_embedding(self):
        return self.has_time_embedding or self.has_conditional_embedding

    @classmethod
    def from_description(cls, description: dict):
        return cls(**description)

    @classmethod
    def from_config_file(cls, config_file: pathlib.Path | str):
        with open(config_file, "r") as f:
            description = yaml.safe_load(f)
        return cls.from_description(description)


# ---------------------------------------------------------------------------------------------------- what the HIP path refuses
def _refuse_options(num_pos_dims, with_conv_on_upsample, with_conv_on_downsample, linear_attention, kernel_sizes):
    """The options of convit.py that have no HIP path: raised when the layer is built, before any launch."""
    if num_pos_dims != 2:
        raise NotImplementedError(f"num_pos_dims={num_pos_dims}: the HIP path implements the 2-D ConVit (num_pos_dims=2)")
    if linear_attention:
        raise NotImplementedError("linear_attention=True is outside the HIP sampling path (softmax attention only)")
    if with_conv_on_upsample:
        raise NotImplementedError("with_conv_on_upsample=True (a strided transposed convolution) is outside the HIP sampling "
                                  "path: bilinear upsampling only")
    if with_conv_on_downsample:
        raise NotImplementedError("with_conv_on_downsample=True (a strided convolution) is outside the HIP sampling path: "
                                  "average pooling only")
    for name, k in kernel_sizes.items():
        if int(k) != k or k < 1 or k % 2 == 0:
            raise NotImplementedError(f"{name}={k}: 'same' convolutions with odd kernel sizes are implemented")


def _check_heads(embed_dim, num_heads, dim_per_head=None):
    """The reference's asserts (convit.py:422-423, 359), as ValueErrors that name the argument."""
    if num_heads < 1 or embed_dim % num_heads:
        raise ValueError(f"embed_dim={embed_dim} is not a multiple of num_heads={num_heads}")
    d = embed_dim // num_heads if dim_per_head is None else dim_per_head
    if d % 2:
        raise ValueError(f"the head width embed_dim / num_heads = {d} must be even (RoPE rotates pairs of channels)")
    return d


# ---------------------------------------------------------------------------------------------------- parameter containers
class ConditionDropout(torch.nn.Module):
    """convit.py:101-122: zeroes whole samples of the embedded condition in training mode; the identity in eval mode, the only
    mode the sampling path implements (ConVit refuses a training-mode call that would draw a mask)."""

    def __init__(self, p: float = 0.5):
        super().__init__()
        self.p = p


class ChannelRMSNorm(torch.nn.Module):
    """ChannelRMSNorm parameters (convit.py:226-243): x / sqrt(mean_c(x^2) + finfo(dtype).eps) * weight."""

    def __init__(self, channel_dim: int, element_wise_affine: bool = True):
        super().__init__()
        self.element_wise_affine = element_wise_affine
        self.channel_dim = channel_dim
        if self.element_wise_affine:
            self.weight = torch.nn.Parameter(torch.ones(channel_dim))
        else:
            self.register_parameter("weight", None)


class Upsample(torch.nn.Module):
    """convit.py:246-271 without a convolution: bilinear interpolation by expansion_factor (ops.upsample_bilinear)."""

    def __init__(self, num_pos_dims, channels_in, channels_out=None, expansion_factor=2, with_conv=False):
        super().__init__()
        _refuse_options(num_pos_dims, with_conv, False, False, {})
        self.num_pos_dims = num_pos_dims
        self.channels_in = channels_in
        self.channels_out = channels_in if channels_out is None else channels_out
        self.expansion_factor = expansion_factor
        if expansion_factor % 2:
            raise ValueError(f"expansion_factor={expansion_factor} must be even (convit.py:256)")


class Downsample(torch.nn.Module):
    """convit.py:274-302 without a convolution: AvgPool(compression_factor), fused into ds_channel_rmsnorm."""

    def __init__(self, num_pos_dims, channels_in, channels_out=None, compression_factor=2, with_conv=False):
        super().__init__()
        _refuse_options(num_pos_dims, False, with_conv, False, {})
        self.num_pos_dims = num_pos_dims
        self.channels_in = channels_in
        self.compression_factor = compression_factor
        if compression_factor % 2:
            raise ValueError(f"compression_factor={compression_factor} must be even (convit.py:287)")


class ConvSwiGLU(torch.nn.Module):
    """ConvSwiGLU parameters (convit.py:305-329): linear_out(SiLU(linear_in(x)) * linear_gate(x)), 'same' convolutions."""

    def __init__(self, embed_dim: int, num_pos_dims: int, expansion_factor: int = 4, kernel_size: int = 1, final_rms: bool = False):
        super().__init__()
        _refuse_options(num_pos_dims, False, False, False, {"kernel_size": kernel_size})
        self.embed_dim = embed_dim
        self.linear_in = torch.nn.Conv2d(embed_dim, embed_dim * expansion_factor, kernel_size, padding="same")
        self.linear_gate = torch.nn.Conv2d(embed_dim, embed_dim * expansion_factor, kernel_size, padding="same")
        self.swish = torch.nn.SiLU()
        self.linear_out = torch.nn.Conv2d(embed_dim * expansion_factor, embed_dim, kernel_size, padding="same")
        if final_rms:
            raise NotImplementedError("ConvSwiGLU(final_rms=True) is not used by ConVit and has no HIP path")


class SwiGLU(torch.nn.Module):
    """SwiGLU parameters (convit.py:332-348); final_rms: torch.nn.RMSNorm(embed_dim) with eps=None, i.e. finfo(dtype).eps."""

    def __init__(self, embed_dim: int, final_rms: bool = False):
        super().__init__()
        self.embed_dim = embed_dim
        self.linear_in = torch.nn.Linear(embed_dim, embed_dim * 4)
        self.linear_gate = torch.nn.Linear(embed_dim, embed_dim * 4)
        self.swish = torch.nn.SiLU()
        self.linear_out = torch.nn.Linear(embed_dim * 4, embed_dim)
        self.final_rms = final_rms
        if final_rms:
            self.rms = torch.nn.RMSNorm(embed_dim)

    def rows(self, te):
        """[M, E] -> [M, E] on the device: three ds_linear launches, the product and the RMS norm in torch (once per run)."""
        with torch.no_grad():
            a = ops.linear(te, self.linear_in.weight, self.linear_in.bias, act=1)
            g = ops.linear(te, self.linear_gate.weight, self.linear_gate.bias, act=0)
            h = ops.linear((a * g).contiguous(), self.linear_out.weight, self.linear_out.bias, act=0)
            if self.final_rms:
                h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + ops.RMS_EPS) * self.rms.weight.detach()
            return h.contiguous()


class LearnedRoPE(torch.nn.Module):
    """LearnedRoPE parameters (convit.py:351-388): angles [num_pos_dims, embed_dim / 2]."""

    def __init__(self, embed_dim: int, num_pos_dims: int = 1, base_freq: float = 1.0, relative_positioning: bool = False):
        super().__init__()
        if embed_dim % 2:
            raise ValueError(f"LearnedRoPE: embed_dim={embed_dim} must be even")
        self.embed_dim = embed_dim
        self.half_dim = embed_dim // 2
        self.base_freq = base_freq
        self.num_pos_dims = num_pos_dims
        self.relative_positioning = relative_positioning
        self.angles = torch.nn.Parameter(torch.randn(self.num_pos_dims, self.half_dim) * self.base_freq)

    def cos_sin(self, grid):
        """[L, half_dim, 2] fp32 on the angles' device for the positions of `grid` = (H, W) in meshgrid 'ij' order, each divided
        by its axis length when relative_positioning (convit.py:370-381): computed in fp64 from the fp32 angles, then rounded."""
        with torch.no_grad():
            ang = self.angles.detach().double()
            axes = [torch.arange(n, dtype=torch.float64, device=ang.device) / (n if self.relative_positioning else 1) for n in grid]
            pos = torch.stack(torch.meshgrid(axes, indexing="ij"), dim=-1).reshape(-1, len(grid))        # [L, num_pos_dims]
            a = pos @ ang                                                                                 # [L, half_dim]
            return torch.stack([torch.cos(a), torch.sin(a)], dim=-1).float().contiguous()


class MultiheadAttention(torch.nn.Module):
    """MultiheadAttention parameters (convit.py:406-456): four [embed_dim, dim_per_head, num_heads] tensors, the RoPE layer and
    the `scale` buffer sqrt(dim_per_head) (the attention kernels' own 1/sqrt(d))."""

    def __init__(self, embed_dim: int, num_heads: int, dim_per_head: int | None = None, num_pos_dims: int = 1, rope_freq: float = 1.0,
                 relative_positioning: bool = False, linear_attention: bool = False):
        super().__init__()
        if linear_attention:
            raise NotImplementedError("linear_attention=True is outside the HIP sampling path (softmax attention only)")
        dim_per_head = _check_heads(embed_dim, num_heads, dim_per_head)
        if dim_per_head * num_heads != embed_dim:
            raise NotImplementedError(f"dim_per_head={dim_per_head}: the HIP path takes dim_per_head = embed_dim / num_heads")
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.dim_per_head = dim_per_head
        self.linear_attention = linear_attention
        self.q_proj_tensor = torch.nn.Parameter(torch.empty((embed_dim, dim_per_head, num_heads)))
        self.k_proj_tensor = torch.nn.Parameter(torch.empty((embed_dim, dim_per_head, num_heads)))
        self.v_proj_tensor = torch.nn.Parameter(torch.empty((embed_dim, dim_per_head, num_heads)))
        self.out_proj_tensor = torch.nn.Parameter(torch.empty((embed_dim, dim_per_head, num_heads)))
        self.reset_parameters()
        self.rope_layer = LearnedRoPE(embed_dim=dim_per_head, num_pos_dims=num_pos_dims, base_freq=rope_freq,
                                      relative_positioning=relative_positioning)
        self.register_buffer("scale", torch.sqrt(torch.tensor(dim_per_head, dtype=torch.float32)))

    def reset_parameters(self):
        bound = 6 / math.sqrt(self.embed_dim + self.dim_per_head)
        for t in (self.q_proj_tensor, self.k_proj_tensor, self.v_proj_tensor, self.out_proj_tensor):
            torch.nn.init.uniform_(t, -bound, bound)

    def qkv_weight(self):
        """[3E, E, 1, 1]: row h*dh + dv of the q third is q_proj_tensor[:, dv, h] (likewise k, v), so head h owns rows
        [h*dh, (h+1)*dh) of each third, as ops.attention(heads=) reads them."""
        E = self.embed_dim
        return torch.cat([t.detach().permute(2, 1, 0).reshape(E, E) for t in (self.q_proj_tensor, self.k_proj_tensor, self.v_proj_tensor)],
                         dim=0).reshape(3 * E, E, 1, 1).contiguous()

    def out_weight(self):
        """[E, E, 1, 1]: W[d, h*dh + dv] = out_proj_tensor[d, dv, h]."""
        E = self.embed_dim
        return self.out_proj_tensor.detach().permute(0, 2, 1).reshape(E, E, 1, 1).contiguous()


class ConVitBlock(torch.nn.Module):
    """ConVitBlock parameters (convit.py:536-603); ConVit.forward_with_shifts runs the launch sequence of its forward."""

    def __init__(self,
                 embed_dim: int,
                 num_pos_dims: int,
                 ffn_expansion_factor: int = 4,
                 attn_compression_factor: int = 2,
                 num_heads: int = 8,
                 rope_freq: float = 1.0,
                 with_conv_on_upsample: bool = False,
                 with_conv_on_downsample: bool = False,
                 kernel_size_conv: int = 3,
                 kernel_size_depthwise: int = 3,
                 has_embedding: bool = False,
                 relative_positioning: bool = False,
                 linear_attention: bool = False):
        super().__init__()
        _refuse_options(num_pos_dims, with_conv_on_upsample, with_conv_on_downsample, linear_attention,
                        {"kernel_size_conv": kernel_size_conv, "kernel_size_depthwise": kernel_size_depthwise})
        if kernel_size_depthwise > ops.DEPTHWISE_MAX_KERNEL:
            raise NotImplementedError(f"kernel_size_depthwise={kernel_size_depthwise}: the depthwise kernel takes sizes up to "
                                      f"{ops.DEPTHWISE_MAX_KERNEL}")
        _check_heads(embed_dim, num_heads)
        self.embed_dim = embed_dim
        self.num_pos_dims = num_pos_dims
        self.ffn_expansion_factor = ffn_expansion_factor
        self.attn_compression_factor = attn_compression_factor
        self.num_heads = num_heads
        self.rope_freq = rope_freq
        self.kernel_size_conv = kernel_size_conv
        self.kernel_size_depthwise = kernel_size_depthwise
        self.linear_attention = linear_attention

        self.norm_1 = ChannelRMSNorm(channel_dim=embed_dim)
        self.norm_2 = ChannelRMSNorm(channel_dim=embed_dim)
        self.attention = MultiheadAttention(embed_dim=embed_dim, num_heads=num_heads, num_pos_dims=num_pos_dims, rope_freq=rope_freq,
                                            relative_positioning=relative_positioning, linear_attention=linear_attention)
        self.upsample = Upsample(num_pos_dims=num_pos_dims, channels_in=embed_dim, channels_out=embed_dim,
                                 expansion_factor=attn_compression_factor, with_conv=with_conv_on_upsample)
        self.downsample = Downsample(num_pos_dims=num_pos_dims, channels_in=embed_dim, channels_out=embed_dim,
                                     compression_factor=attn_compression_factor, with_conv=with_conv_on_downsample)
        self.ffn = ConvSwiGLU(embed_dim=embed_dim, num_pos_dims=num_pos_dims, expansion_factor=ffn_expansion_factor,
                              kernel_size=kernel_size_conv)
        self.depthwise_conv = torch.nn.Conv2d(embed_dim, embed_dim, kernel_size=kernel_size_depthwise, groups=embed_dim, padding="same")
        self.pointwise_conv = torch.nn.Conv2d(embed_dim, embed_dim, kernel_size=1)
        self.conv_activation = torch.nn.SiLU()
        self.fusion_weight = torch.nn.Parameter(torch.tensor(0.0))
        self.has_embedding = has_embedding
        if has_embedding:
            self.embedding_projection = SwiGLU(embed_dim=embed_dim, final_rms=True)


_ROWS_PER_BLOCK = 7      # amax rows a block takes: norm_1, q k | v, attention, depthwise SiLU, norm_2, the gate


class ConVit(torch.nn.Module):
    capturable = True

    def __init__(self, config: ConVitConfig, conditional_embedding: None | torch.nn.Module = None):
        super().__init__()
        self.config = config
        self.in_channels = config.in_channels
        self.embed_dim = config.embed_dim
        out_channels = config.out_channels if config.out_channels is not None else config.in_channels
        self.out_channels = out_channels
        self.num_pos_dims = config.num_pos_dims
        self.num_layers = config.num_layers
        self.num_heads = config.num_heads
        self.ffn_expansion_factor = config.ffn_expansion_factor
        self.attn_compression_factor = config.attn_compression_factor
        self.rope_freq = config.rope_freq
        self.with_conv_on_upsample = config.with_conv_on_upsample
        self.with_conv_on_downsample = config.with_conv_on_downsample
        self.kernel_size_conv = config.kernel_size_conv
        self.kernel_size_depthwise = config.kernel_size_depthwise
        self.kernel_size_in_out = config.kernel_size_in_out
        self.has_embedding = config.has_embedding
        self.has_conditional_embedding = config.has_conditional_embedding
        self.fourier_projection_scale = config.fourier_projection_scale
        self.relative_positioning = config.relative_positioning
        self.linear_attention = config.linear_attention
        self.input_batch_norm = config.input_batch_norm
        self.condition_dropout = config.condition_dropout

        _refuse_options(self.num_pos_dims, self.with_conv_on_upsample, self.with_conv_on_downsample, self.linear_attention,
                        {"kernel_size_conv": self.kernel_size_conv, "kernel_size_in_out": self.kernel_size_in_out,
                         "kernel_size_depthwise": self.kernel_size_depthwise})
        if self.input_batch_norm:
            raise NotImplementedError("input_batch_norm=True is outside the HIP sampling path")
        _check_heads(self.embed_dim, self.num_heads)
        self.normin = torch.nn.Identity()
        self.convin = torch.nn.Conv2d(self.in_channels, self.embed_dim, self.kernel_size_in_out, padding="same")
        self.convout = torch.nn.Conv2d(self.embed_dim, self.out_channels, self.kernel_size_in_out, padding="same")
        self.normout = ChannelRMSNorm(channel_dim=self.embed_dim)
        self.blocks = torch.nn.ModuleList([
            ConVitBlock(embed_dim=self.embed_dim,
                        num_pos_dims=self.num_pos_dims,
                        ffn_expansion_factor=self.ffn_expansion_factor,
                        attn_compression_factor=self.attn_compression_factor,
                        num_heads=self.num_heads,
                        rope_freq=self.rope_freq,
                        with_conv_on_upsample=self.with_conv_on_upsample,
                        with_conv_on_downsample=self.with_conv_on_downsample,
                        kernel_size_conv=self.kernel_size_conv,
                        kernel_size_depthwise=self.kernel_size_depthwise,
                        has_embedding=self.has_embedding,
                        relative_positioning=self.relative_positioning,
                        linear_attention=self.linear_attention)
            for _ in range(self.num_layers)
        ])
        if self.condition_dropout > 0.0:
            self.condition_dropout_module = ConditionDropout(self.condition_dropout)
        else:
            self.condition_dropout_module = torch.nn.Identity()
        if config.has_time_embedding:
            self.time_embedding = _Fourier(self.embed_dim, self.fourier_projection_scale)
        if config.has_conditional_embedding:
            assert isinstance(conditional_embedding, torch.nn.Module)
            self.conditional_embedding = conditional_embedding
        else:
            # Reference quirk, kept (convit.py:715): isinstance(x, None) raises TypeError, so a ConVit can only be built with
            # has_conditional_embedding=True and a module; it then runs unconditionally with y=None
            isinstance(conditional_embedding, None)
        self.conv_precision = "fp16x3"       # see PUNetG.conv_precision; "fp32": the exact-fp32 MFMA convolutions and attention
        self.auto_precision = True           # see PUNetG.auto_precision
        self._packed = None
        self._packed_sig = None
        self._rope = {}
        self._ws = Workspace()
        self._arena_rows = max(8, _ROWS_PER_BLOCK * len(self.blocks) + 2)

    # ------------------------------------------------------------------ reference surface
    def check_input(self, shape):
        """Raised on the host before any launch (the reference fails at the residual add, convit.py:631)."""
        if len(shape) != 4:
            raise ValueError(f"ConVit takes [B, {self.in_channels}, H, W] fields; got a {len(shape)}-D tensor")
        if shape[1] != self.in_channels:
            raise ValueError(f"expected in_channels={self.in_channels} input channels, got {shape[1]}")
        f = self.attn_compression_factor
        if shape[2] % f or shape[3] % f or min(shape[2], shape[3]) < f:
            raise ValueError(f"a {shape[2]}x{shape[3]} field does not pool by attn_compression_factor={f}: "
                             f"choose H and W multiples of {f}")

    @ops.device_guard
    def forward(self, x, t=None, y=None):
        """convit.py:721-735.  Top-level call: guarded (see PUNetG.forward)."""
        return runtime.guarded_forward(self, self.forward_unguarded, x, t, y)

    @ops.device_guard
    def forward_unguarded(self, x, t=None, y=None):
        if torch.is_tensor(x):
            self.check_input(x.shape)
        if y is not None:
            self._require_eval()
        ops.require_device(x, "x")
        ye = self.embed_condition(y) if y is not None else None
        te = None
        if t is not None or ye is not None:
            te = self.embed_time(None if t is None else t.reshape(-1).to(x), ye)
        return self.forward_with_shifts(x.contiguous(), None if te is None else self.time_shifts(te), row=None)

    # ------------------------------------------------------------------ conditioning
    def _require_eval(self):
        if self.training and self.condition_dropout > 0.0:
            raise NotImplementedError(f"condition_dropout={self.condition_dropout} in training mode draws a per-sample mask: the HIP "
                                      "sampling path implements eval mode only, call .eval()")

    def embed_condition(self, y):
        """conditional_embedding(y) (convit.py:723-725), the user's module run as given -> [rows, embed_dim]."""
        self._require_eval()
        with torch.no_grad():
            ye = self.conditional_embedding(y)
        ops.require_device(ye, "conditional_embedding(y)")
        return ye.reshape(-1, self.embed_dim).contiguous()

    def embed_time(self, cn, ye=None):
        """time_embedding(t) [+ ye] (convit.py:722-726) -> [M, embed_dim]; cn=None: ye alone."""
        if cn is None:
            return ye
        ops.require_device(cn, "t")
        return ops.fourier_features(cn.contiguous(), self.time_embedding.W, add=ye)

    def time_shifts(self, te):
        """Per-block embedding_projection(te) (convit.py:612, 345-348): one [M, embed_dim] table per block."""
        te = te.contiguous()
        return [b.embedding_projection.rows(te) for b in self.blocks]

    # ------------------------------------------------------------------ weights
    def packed_weights(self):
        """The convolution weights in the kernels' layouts, and what else a forward pass reads that is derived from parameters:
        the concatenated ffn biases and s = sigmoid(fusion_weight) as a device scalar.  Rebuilt when a parameter it was built from
        changed (address, version, device) or conv_precision did."""
        src = [self.convin.weight, self.convout.weight]
        for b in self.blocks:
            a = b.attention
            src += [a.q_proj_tensor, a.k_proj_tensor, a.v_proj_tensor, a.out_proj_tensor, a.rope_layer.angles, b.pointwise_conv.weight,
                    b.ffn.linear_in.weight, b.ffn.linear_gate.weight, b.ffn.linear_in.bias, b.ffn.linear_gate.bias, b.ffn.linear_out.weight,
                    b.fusion_weight]
        sig = weights_signature(src, self.conv_precision)
        if self._packed is not None and sig == self._packed_sig:
            return self._packed
        if self.conv_precision not in ops.CONV_PRECISIONS:
            raise ValueError(f"unknown conv_precision {self.conv_precision!r}; choose from {ops.CONV_PRECISIONS}")
        prec = "fp16x3" if self.conv_precision == "fp16x3" else "fp32"
        pk = {}
        with torch.no_grad():
            pk["in"] = ops.pack_conv(self.convin.weight.detach(), prec)
            pk["out"] = ops.pack_conv(self.convout.weight.detach(), prec)
            for i, b in enumerate(self.blocks):
                pk["qkv", i] = ops.pack_conv(b.attention.qkv_weight(), prec)
                pk["proj", i] = ops.pack_conv(b.attention.out_weight(), prec)
                pk["pw", i] = ops.pack_conv(b.pointwise_conv.weight.detach(), prec)
                pk["ffn_in", i] = ops.pack_conv(torch.cat([b.ffn.linear_in.weight.detach(), b.ffn.linear_gate.weight.detach()], 0), prec)
                pk["ffn_in_b", i] = torch.cat([b.ffn.linear_in.bias.detach(), b.ffn.linear_gate.bias.detach()], 0).contiguous()
                pk["ffn_out", i] = ops.pack_conv(b.ffn.linear_out.weight.detach(), prec)
                pk["s", i] = torch.sigmoid(b.fusion_weight.detach()).reshape(1).contiguous()
        self._packed, self._packed_sig = pk, sig
        self._rope = {}
        return pk

    def _cos_sin(self, i, grid):
        """The RoPE table of block i on `grid`, cached with the packed weights (packed_weights() clears it)."""
        key = (i,) + tuple(grid)
        cs = self._rope.get(key)
        if cs is None:
            cs = self._rope[key] = self.blocks[i].attention.rope_layer.cos_sin(grid)
        return cs

    # ------------------------------------------------------------------ the network
    def _block(self, i, blk, x, mod, row, pk, ws, am):
        """ConVitBlock.forward (convit.py:605-636) on x [B, E, H, W]; mod: the block's [rows, E] embedding table or None.
        Returns the block's output (a pool buffer; x goes back to the pool)."""
        B, E, H, W = x.shape
        f, heads = blk.attn_compression_factor, blk.num_heads
        Hp, Wp = H // f, W // f
        L = Hp * Wp
        dev = x.device
        h3 = am is not None

        def amax_kw(**kw):                                              # in_amax / out_amax are arguments of the fp16x3 kernels only
            return kw if h3 else {}

        def row_():
            return am.row() if h3 else None

        # attention(downsample(norm_1(x) + y)) on the pooled grid
        a_n = row_()
        full = ws.take((B, E, H, W), dev)                               # later: u
        n = ops.channel_rmsnorm(x, blk.norm_1.weight, mod, row, pool=f, out=ws.take((B, E, Hp, Wp), dev), out_amax=a_n,
                                scratch=None if f in ops.RMS_FUSED_POOLS else full)
        qkv = ops.conv(n, pk["qkv", i], out=ws.take((B, 3 * E, Hp, Wp), dev), **amax_kw(in_amax=a_n))
        a_qkv = am.rows(2) if h3 else None
        ops.rope2d(qkv.view(B, 3 * E, L), E, heads, self._cos_sin(i, (Hp, Wp)), out_amax=a_qkv)
        nws = ops.attention_workspace_floats(B, E, L, self.conv_precision, heads=heads)
        aws = ws.take((nws,), dev) if nws else None
        a_o = row_()
        o = ops.attention(qkv.view(B, 3 * E, L), E, out=n.view(B, E, L), precision=self.conv_precision, workspace=aws, heads=heads,
                          **amax_kw(in_amax=a_qkv, out_amax=a_o))       # the attention output overwrites the norm buffer
        if aws is not None:
            ws.give(aws)
        y = ops.conv(o.view(B, E, Hp, Wp), pk["proj", i], out=ws.take((B, E, Hp, Wp), dev), **amax_kw(in_amax=a_o))
        ws.give(qkv)
        ws.give(n)
        u = ops.upsample_bilinear(y, f, out=full)
        ws.give(y)
        # the convolution pathway and the fusion: x <- (1 - s) u + s pointwise(SiLU(depthwise(u))) + x
        a_d = row_()
        d = ops.depthwise_conv_silu(u, blk.depthwise_conv.weight, blk.depthwise_conv.bias, out=ws.take((B, E, H, W), dev), out_amax=a_d)
        xc = ops.conv(d, pk["pw", i], bias=blk.pointwise_conv.bias, out=ws.take((B, E, H, W), dev), **amax_kw(in_amax=a_d))
        ops.convit_blend(u, xc, x, pk["s", i], out=x)
        ws.give(xc)
        # x + ffn(norm_2(x) + y)
        a_n = row_()
        ops.channel_rmsnorm(x, blk.norm_2.weight, mod, row, out=d, out_amax=a_n)
        F2 = 2 * E * blk.ffn_expansion_factor
        ag = ops.conv(d, pk["ffn_in", i], bias=pk["ffn_in_b", i], out=ws.take((B, F2, H, W), dev), **amax_kw(in_amax=a_n))
        a_h = row_()
        hg = ops.swiglu(ag, out=ws.take((B, F2 // 2, H, W), dev), out_amax=a_h)
        out = ops.conv(hg, pk["ffn_out", i], bias=blk.ffn.linear_out.bias, res1=x, out=u, **amax_kw(in_amax=a_h))
        ws.give(hg)
        ws.give(ag)
        ws.give(d)
        ws.give(x)
        return out

    def forward_with_shifts(self, x, shifts, row=None, out=None):
        """The network body given the per-block embedding tables.  shifts: None (no embedding row: t and y both absent), or one
        table per block: [M, E] with row `row` serving the batch (the sampler's table of all evaluations), [1 or B, E] with
        row=None, or [M, B, E] with per-sample rows of evaluation `row`."""
        self.check_input(x.shape)
        ops.require_device(x, "x")
        if shifts is not None and len(shifts) != len(self.blocks):
            raise ValueError("one embedding table per block")
        pk = self.packed_weights()
        ws = self._ws
        B, C, H, W = x.shape
        E = self.embed_dim
        dev = x.device
        h3 = self.conv_precision == "fp16x3"
        am = AmaxArena(ws, B, dev, rows=self._arena_rows) if h3 else None                  # one fill launch zeroes every slot of the pass
        try:
            kw = dict(in_amax=am.of(x)) if h3 else {}
            h = ops.conv(x, pk["in"], bias=self.convin.bias, out=ws.take((B, E, H, W), dev), **kw)
            for i, blk in enumerate(self.blocks):
                s, r = (None, None) if shifts is None else (shifts[i], row)
                if s is not None and s.dim() == 3:
                    s, r = s[row], None
                h = self._block(i, blk, h, s, r, pk, ws, am)
            a_n = am.row() if h3 else None
            n = ops.channel_rmsnorm(h, self.normout.weight, out=ws.take((B, E, H, W), dev), out_amax=a_n)
            kw = dict(in_amax=a_n) if h3 else {}
            y = ops.conv(n, pk["out"], bias=self.convout.bias, out=out, **kw)
            ws.give(n)
            ws.give(h)
            return y
        finally:
            if am is not None:
                am.release()
