"""DiffusionTransformer score network on HIP kernels (reference: diffsci/models/nets/difftransformer.py).

Same constructor, public attributes, ``net(x, t)`` protocol and state_dict keys as the reference's ``DiffusionTransformer``
(difftransformer.py:200-236), so its checkpoints load with strict=True.  The torch.nn layers are parameter containers only;
every tensor operation is a launch into libdiffsci_hip.so.  Tokens live channel-major, [B, nembed, L] with the L = (H/p)(W/p)
tokens contiguous, which is the layout the 1x1 convolution (a Linear applied to every token) and the attention kernels read:

  patcher + embed, unembed + patcher.inverse                    ds_patch_embed, ds_patch_unembed
  norm1 / norm2 + adaln_modulate                                ds_token_layernorm
  attn.attn in_proj / out_proj, mlp.0 / mlp.2                   ds_conv1x1_h3 (fp16x3) or ds_conv2d (exact fp32), 1x1
  attention core                                                ds_attention_h3_heads / ds_attention_heads_generic
  SiLU inside the MLP                                           ds_silu_amax
  x + gate * branch                                             ds_token_gate
  time_embed, resnet_time_block, every adaln_modulation         ds_fourier_features, ds_linear, ds_add, ds_add_act

Two reference quirks are kept: the core is built with ``nblocks`` and ``mlp_factor`` swapped (see ``__init__``), and
``positional_encoding`` is constructed (its ``div_term`` buffer is a state_dict entry) and never applied
(difftransformer.py:220, 226-236).

The time path depends on the noise level only, so KarrasModule evaluates it once per run for all evaluations (``embed_time`` ->
``time_shifts``: one [M, 6*nembed] modulation table per block) and the captured sampler calls ``forward_with_shifts`` with a row
index.  Every fp16x3 launch takes a per-sample activation exponent from the kernel that produced its input (``out_amax`` of the
LayerNorm, the in-projection, the attention, the SiLU); the slots are rows of one arena per forward pass, zeroed by one launch."""
import torch

from ... import ops
from . import runtime
from .punetg import _Fourier
from .runtime import AmaxArena, Workspace, weights_signature


class _ResnetTimeBlock(torch.nn.Module):
    """ResnetTimeBlock parameters (difftransformer.py:31-67): te + net(te)."""

    def __init__(self, embed_channels):
        super().__init__()
        c = embed_channels
        self.net = torch.nn.Sequential(torch.nn.Linear(c, 4 * c), torch.nn.Identity(), torch.nn.Linear(4 * c, 4 * c),
                                       torch.nn.Identity(), torch.nn.Linear(4 * c, c))


class _PositionalEncoding2d(torch.nn.Module):
    """PositionalEncoding2d's buffer (difftransformer.py:97-105); the reference never applies the encoding."""

    def __init__(self, dembed, denominator=10000.0):
        super().__init__()
        dembed1d = dembed // 2
        indexes = torch.arange(start=0, end=dembed1d, step=2)
        self.register_buffer("div_term", denominator ** (indexes / dembed1d))


class _SelfAttention(torch.nn.Module):
    """SelfAttention parameters (difftransformer.py:124-136); constructing the MultiheadAttention applies torch's own rule for
    nembed % nheads."""

    def __init__(self, nembed, nheads):
        super().__init__()
        self.attn = torch.nn.MultiheadAttention(nembed, nheads, batch_first=True)


class _DiTBlock(torch.nn.Module):
    """DiTBlock parameters (difftransformer.py:139-160)."""

    def __init__(self, nembed, nheads, mlp_factor=4):
        super().__init__()
        self.nmlp = mlp_factor * nembed
        self.norm1 = torch.nn.LayerNorm(nembed)
        self.norm2 = torch.nn.LayerNorm(nembed)
        self.attn = _SelfAttention(nembed, nheads)
        self.mlp = torch.nn.Sequential(torch.nn.Linear(nembed, self.nmlp), torch.nn.Identity(), torch.nn.Linear(self.nmlp, nembed))
        self.adaln_modulation = torch.nn.Sequential(torch.nn.Identity(), torch.nn.Linear(nembed, 6 * nembed))


class _DiTCore(torch.nn.Module):
    def __init__(self, nembed, nheads, nblocks, mlp_factor=4):
        super().__init__()
        self.blocks = torch.nn.ModuleList([_DiTBlock(nembed, nheads, mlp_factor) for _ in range(nblocks)])


# chunk6 of adaln_modulation's output (difftransformer.py:163-168)
SHIFT_MSA, SCALE_MSA, GATE_MSA, SHIFT_MLP, SCALE_MLP, GATE_MLP = range(6)
_ROWS_PER_BLOCK = 6      # amax rows a block takes: norm1, q k | v, attention, norm2, SiLU


class DiffusionTransformer(torch.nn.Module):
    capturable = True

    def __init__(self, nembed=64, nheads=4, mlp_factor=4, nblocks=6, patch_size=4, nchannels=1):
        super().__init__()
        self.nembed = nembed
        self.nheads = nheads
        self.mlp_factor = mlp_factor
        self.nblocks = nblocks
        self.patch_size = patch_size
        self.nchannels = nchannels
        # Reference quirk, kept so that its checkpoints load: DiffusionTransformer hands (nembed, nheads, mlp_factor, nblocks) to
        # DiTCore positionally, whose parameters are (nembed, nheads, nblocks, mlp_factor) (difftransformer.py:179-183, 216-219) --
        # the core has `mlp_factor` blocks whose MLPs are `nblocks` times nembed wide (the defaults: 4 blocks, hidden width 6 * 64)
        self.core = _DiTCore(nembed, nheads, nblocks=mlp_factor, mlp_factor=nblocks)
        self.positional_encoding = _PositionalEncoding2d(nembed)
        self.embed = torch.nn.Linear(nchannels * patch_size ** 2, nembed)
        self.unembed = torch.nn.Linear(nembed, nchannels * patch_size ** 2)
        self.time_embed = _Fourier(nembed, 30.0)
        self.resnet_time_block = _ResnetTimeBlock(nembed)
        self.conv_precision = "fp16x3"       # see PUNetG.conv_precision; "fp32": the exact-fp32 MFMA 1x1 convolution and attention
        self.auto_precision = True           # see PUNetG.auto_precision
        self._packed = None
        self._packed_sig = None
        self._ws = Workspace()
        self._arena_rows = max(8, _ROWS_PER_BLOCK * len(self.core.blocks))

    # ------------------------------------------------------------------ reference surface
    def check_input(self, shape):
        """Raised on the host before any launch (the reference fails inside einops)."""
        if len(shape) != 4:
            raise ValueError(f"DiffusionTransformer takes [B, {self.nchannels}, H, W] images; got a {len(shape)}-D tensor")
        p = self.patch_size
        if shape[1] != self.nchannels:
            raise ValueError(f"expected nchannels={self.nchannels} input channels, got {shape[1]}")
        if shape[2] % p or shape[3] % p:
            raise ValueError(f"a {shape[2]}x{shape[3]} image does not divide into patches of patch_size={p}: "
                             f"choose H and W multiples of {p}")

    @ops.device_guard
    def forward(self, x, t):
        """difftransformer.py:226-236.  Top-level call: guarded (see PUNetG.forward)."""
        return runtime.guarded_forward(self, self.forward_unguarded, x, t)

    @ops.device_guard
    def forward_unguarded(self, x, t):
        if torch.is_tensor(x):
            self.check_input(x.shape)
        ops.require_device(x, "x")
        te = self.embed_time(t.reshape(-1).to(x))
        return self.forward_with_shifts(x.contiguous(), self.time_shifts(te), row=None)

    # ------------------------------------------------------------------ conditioning
    def embed_time(self, cn, ye=None):
        """resnet_time_block(time_embed(t)) (difftransformer.py:230, 53-67) -> [M, nembed]."""
        if ye is not None:
            raise ValueError("DiffusionTransformer is unconditional (the reference's takes no y)")
        ops.require_device(cn, "t")
        g = ops.fourier_features(cn.contiguous(), self.time_embed.W)
        net = self.resnet_time_block.net
        h = ops.linear(g, net[0].weight, net[0].bias, act=1)
        h = ops.linear(h, net[2].weight, net[2].bias, act=1)
        h = ops.linear(h, net[4].weight, net[4].bias, act=0)
        return ops.add(g, h)

    def time_shifts(self, te):
        """Per-block adaln_modulation(te) (difftransformer.py:157-168): list of [M, 6*nembed] tables, the six chunks in the
        reference's order (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp)."""
        s = ops.add_act(te.contiguous(), act=1)
        return [ops.linear(s, b.adaln_modulation[1].weight, b.adaln_modulation[1].bias, act=0) for b in self.core.blocks]

    # ------------------------------------------------------------------ weights
    def packed_weights(self):
        lin = []
        for b in self.core.blocks:
            lin += [b.attn.attn.in_proj_weight, b.attn.attn.out_proj.weight, b.mlp[0].weight, b.mlp[2].weight]
        sig = weights_signature(lin, self.conv_precision)
        if self._packed is not None and sig == self._packed_sig:
            return self._packed
        if self.conv_precision not in ops.CONV_PRECISIONS:
            raise ValueError(f"unknown conv precision {self.conv_precision!r}; choose from {ops.CONV_PRECISIONS}")
        prec ="fp16x3" if self.conv_precision == "fp16x3" else "fp32"      # 1x1: fp16x3 or the exact-fp32 MFMA kernel
        with torch.no_grad():
            pk = {id(w): ops.pack_conv(w.detach().reshape(w.shape[0], w.shape[1], 1, 1), prec) for w in lin}
        self._packed, self._packed_sig = pk, sig
        return pk

    # ------------------------------------------------------------------ the network
    def _block(self, blk, x, mod, row, pk, ws, am, grid):
        """DiTBlock.forward (difftransformer.py:162-175) in place on x [B, E, L]; mod: the block's [rows, 6E] table."""
        B, E, L = x.shape
        Hp, Wp = grid
        dev = x.device
        mh = blk.attn.attn
        h3 = am is not None

        def amax_kw(**kw):                                              # in_amax / out_amax are arguments of the fp16x3 kernels only
            return kw if h3 else {}

        def g4(t):
            return t.view(B, t.shape[1], Hp, Wp)

        # x += gate_msa * attn(modulate(norm1(x), shift_msa, scale_msa))
        a_n = am.row() if h3 else None
        a = ops.token_layernorm(x, blk.norm1.weight, blk.norm1.bias, mod, SHIFT_MSA, SCALE_MSA, row, eps=blk.norm1.eps,
                                out=ws.take((B, E, L), dev), out_amax=a_n)
        y = runtime.attention(g4(a), pk[id(mh.in_proj_weight)], mh.in_proj_bias, pk[id(mh.out_proj.weight)], mh.out_proj.bias,
                              E=E, heads=mh.num_heads, precision=self.conv_precision, ws=ws, am=am, in_amax=a_n,
                              attn_out=a)                             # the attention output overwrites the norm buffer
        ops.token_gate(x, y.view(B, E, L), mod, GATE_MSA, row, out=x)
        # x += gate_mlp * mlp(modulate(norm2(x), shift_mlp, scale_mlp))
        a_n = am.row() if h3 else None
        ops.token_layernorm(x, blk.norm2.weight, blk.norm2.bias, mod, SHIFT_MLP, SCALE_MLP, row, eps=blk.norm2.eps, out=a, out_amax=a_n)
        h = ops.conv(g4(a), pk[id(blk.mlp[0].weight)], bias=blk.mlp[0].bias, out=ws.take((B, blk.nmlp, Hp, Wp), dev),
                     **amax_kw(in_amax=a_n))
        a_h = am.row() if h3 else None
        ops.silu_amax(h, out=h, out_amax=a_h)
        ops.conv(h, pk[id(blk.mlp[2].weight)], bias=blk.mlp[2].bias, out=y, **amax_kw(in_amax=a_h))
        ws.give(h)
        ops.token_gate(x, y.view(B, E, L), mod, GATE_MLP, row, out=x)
        ws.give(a)
        ws.give(y)

    def forward_with_shifts(self, x, shifts, row=None, out=None):
        """The network body given the per-block modulation tables.  shifts[i]: [M, 6E] with row `row` serving the batch (the
        sampler's table of all evaluations), or [1 or B, 6E] with row=None, or [M, B, 6E] with per-sample rows of evaluation `row`."""
        self.check_input(x.shape)
        ops.require_device(x, "x")
        if len(shifts) != len(self.core.blocks):
            raise ValueError("one modulation table per block")
        pk = self.packed_weights()
        ws = self._ws
        B, C, H, W = x.shape
        p, E = self.patch_size, self.nembed
        Hp, Wp = H // p, W // p
        dev = x.device
        h3 = self.conv_precision == "fp16x3"
        am = AmaxArena(ws, B, dev, rows=self._arena_rows) if h3 else None                  # one fill launch zeroes every slot of the pass
        try:
            tok = ops.patch_embed(x, self.embed.weight, self.embed.bias, p, out=ws.take((B, E, Hp * Wp), dev))
            for blk, s in zip(self.core.blocks, shifts):
                r = row
                if s.dim() == 3:
                    s, r = s[row], None
                self._block(blk, tok, s, r, pk, ws, am, (Hp, Wp))
            y = ops.patch_unembed(tok, self.unembed.weight, self.unembed.bias, p, (B, C, H, W), out=out)
            ws.give(tok)
            return y
        finally:
            if am is not None:
                am.release()
