"""What the networks of the HIP sampling path share on the host: the buffer pool and the amax arena of a forward pass, the
"repack when a weight changed" signature, the row selection of a tabulated shift, the guarded top-level forward, and the
attention launch sequence.  Plain functions and two small classes; every network keeps its own walk and its own caches."""
import math

import torch

from ... import ops
from . import precision


def require_eval(net, *rates):
    """Dropout, condition dropout and ConditionDrop are the identity in eval mode -- the only mode the sampling path
    implements.  A network left in training mode with a non-zero rate would silently differ from the reference."""
    if net.training and any(r for r in rates if r):
        raise NotImplementedError("dropout / cond_dropout / cond_drop > 0 in training mode are outside the HIP sampling "
                                  "path: call .eval() (the reference samples under eval() too)")


class Workspace:
    """Shape-keyed pool of device buffers.  A forward pass takes and gives buffers in a fixed
    order, so after the first pass no allocation happens -- a requirement for hipGraph capture."""

    def __init__(self):
        self.free = {}
        self.frozen = False
        self.bytes = 0

    def take(self, shape, device):
        key = (tuple(shape), str(device))
        lst = self.free.get(key)
        if lst:
            return lst.pop()
        if self.frozen:
            raise RuntimeError(f"workspace is frozen (graph captured) but a new buffer {shape} was requested")
        with torch.inference_mode(False):    # a normal tensor even when the sampler runs under inference_mode: the pool
            t = torch.empty(shape, dtype=torch.float32, device=device)   # outlives the call and serves eager forwards too
        self.bytes += t.numel() * 4
        return t

    def give(self, t):
        self.free.setdefault((tuple(t.shape), str(t.device)), []).append(t)


class AmaxArena:
    """Per-forward rows of "amax" slots (ops.py: per-sample max |x| as float bits, the activation exponents of the fp16x3
    kernels' raw-input launches), taken from the workspace and zeroed by ONE fill launch; producers' epilogues merge into a
    row (out_amax), the raw-input consumer reads it (in_amax).  rows: how many the pass may take (the count is part of the
    arena's workspace key)."""
    ROWS = 256

    def __init__(self, ws, B, dev, zero=True, rows=None):
        self.nrows = self.ROWS if rows is None else rows
        self.ws, self.buf = ws, ws.take((self.nrows, max(B, 1)), dev)
        self.i32 = self.buf.view(torch.int32)
        if zero:                                  # zero=False: the caller's first act is of_input(), which zeroes the arena itself
            ops.amax_zero(self.i32)
        self.zeroed = zero
        self.n = 0

    def row(self):
        if not self.zeroed:
            ops.amax_zero(self.i32)
            self.zeroed = True
        if self.n >= self.nrows:
            raise RuntimeError("amax arena exhausted")
        self.n += 1
        return self.i32[self.n - 1]

    def rows(self, n):
        """n consecutive rows as one [n * B] tensor."""
        if not self.zeroed:
            ops.amax_zero(self.i32)
            self.zeroed = True
        if self.n + n > self.nrows:
            raise RuntimeError("amax arena exhausted")
        self.n += n
        return self.i32[self.n - n:self.n].view(-1)

    def of(self, x, rows=None):
        """Slots filled by a reduction over x (a tensor no epilogue of ours produced)."""
        return ops.absmax_rows(x, rows, out=self.row())

    def of_input(self, x, flag, wmax):
        """The same for a network input x [B, C, ...] (c_in * x next to raw user fields): per-channel maxima first, `flag` raised
        when one exponent per sample cannot serve the input layer given its weights (ops.absmax_channels; precision.input_layer_flag)."""
        C = x.shape[1]
        if not self.zeroed:
            if self.n == 0 and C <= 64 and x[0].numel() <= ops.INPUT_AMAX_MAX_FLOATS and x.shape[0] == self.i32.shape[1]:
                self.n, self.zeroed = 1, True
                return ops.input_amax(self.i32, 0, x, flag, wmax)      # one launch: zero the arena, reduce, apply the channel criterion
            ops.amax_zero(self.i32)
            self.zeroed = True
        if self.n + C + 1 > self.nrows:
            return self.of(x)
        out = self.row()
        scratch = self.i32[self.n:self.n + C].view(-1)
        self.n += C
        return ops.absmax_channels(x, out, scratch, flag, wmax)

    def release(self):
        self.ws.give(self.buf)


def tensor_version(t):
    """A tensor's in-place update count; inference tensors (a module built under torch.inference_mode) carry no version
    counter and cannot be written in place."""
    return 0 if t.is_inference() else t._version


def weights_signature(tensors, *extra):
    """What a cache of packed weights is valid for: `extra` (the switches that select the packing), then the address, version
    and device of every tensor.  The owner repacks when the signature differs from the one it stored."""
    return extra + tuple((t.data_ptr(), tensor_version(t), str(t.device)) for t in tensors)


def shift_rows(s, row, B):
    """The rows of one block's tabulated shift that serve a batch of B: a field [B, C, He, We] passes through; with `row`,
    s[row] of [n_evals, B, C] (per-sample conditions in the planned sampler) or row `row` of [M, C] (one row for the whole
    batch: sigma is a per-step constant); without, [1 or B, C] as it is."""
    if s.dim() == 4:
        return s
    if row is not None:
        if s.dim() == 3:
            if s.shape[1] != B:
                raise ValueError("time embedding batch does not match x")
            return s[row]
        return s[row:row + 1]
    if s.shape[0] not in (1, B):
        raise ValueError("time embedding batch does not match x")
    return s


def guarded_forward(net, run, *inputs):
    """A top-level call run(*inputs) of `net`, inputs[0] being the field x: the result is checked by the domain guards
    (nets/precision.py: one device reduction and a host read) and recomputed once if one fires."""
    out = run(*inputs)
    if precision.needs_escalation(net, out, inputs[0]):
        precision.escalate(net)
        out = run(*inputs)
    return out


def _amax_kw(pack, **kw):
    """in_amax / out_amax / amax_split are arguments of the fp16x3 kernels only."""
    return kw if pack.kind == "fp16x3" else {}


class FoldedAttention:
    """The projections of a single-head block with K and V folded away: w_q, b_q = the packed M = Wk^T Wq and
    c = Wk^T bq of the E -> E in-projection whose output q' attends over x itself; w_out, b_out = the packed W' = Wo Wv and
    b' = Wo bv + bo of the out-projection.  Biases may be None (a block without biases)."""
    __slots__ = ("w_q", "b_q", "w_out", "b_out")

    def __init__(self, w_q, b_q, w_out, b_out):
        self.w_q, self.b_q, self.w_out, self.b_out = w_q, b_q, w_out, b_out


def fold_attention_weights(w_in, b_in, w_out, b_out):
    """(M, c, W', b') in fp64 from the in-projection [3E, E] (rows q, k, v; bias [3E] or None) and the out-projection [E, E]
    (bias [E] or None) of a single-head block:
        scores  (Wq x_i + bq).(Wk x_j + bk) = (Wk^T Wq x_i + Wk^T bq).x_j + a term without j, which the softmax over j removes
        values  Wo (sum_j p_ij (Wv x_j + bv)) + bo = (Wo Wv)(sum_j p_ij x_j) + (Wo bv + bo), the p_ij summing to 1."""
    E = w_out.shape[0]
    w_in, w_out = w_in.detach().double().reshape(3 * E, E), w_out.detach().double().reshape(E, E)
    wq, wk, wv = w_in[:E], w_in[E:2 * E], w_in[2 * E:]
    M, Wp = wk.t() @ wq, w_out @ wv
    c = bp = None
    if b_in is not None:
        b_in = b_in.detach().double()
        c, bp = wk.t() @ b_in[:E], w_out @ b_in[2 * E:]
    if b_out is not None:
        bp = b_out.detach().double() + (0 if bp is None else bp)
    return M, c, Wp, bp


def attention_folds(folded, E, L, heads, precision, cosine):
    """Whether attention() takes the folded route: a bundle of fp16x3 packings, one head, plain (not cosine) logits, and the
    image form of the attention core -- the only one with a pre-pass for x to feed."""
    return (folded is not None and folded.w_q.kind == "fp16x3" and folded.w_out.kind == "fp16x3" and heads == 1 and not cosine
            and ops._attention_uses_images(E, L, precision))


def attention(x4, w_in, b_in, w_out, b_out, *, E, heads, precision, ws=None, am=None, in_amax=None, out_amax=None,
              res1=None, res2=None, tile_stats=None, cosine=False, attn_out=None, folded=None):
    """Self-attention over the positions of x4 [B, E, H, W], channel-major throughout: in-projection (w_in, b_in: the packed
    [3E, E] 1x1 convolution), the attention core with `heads` heads, out-projection (w_out, b_out) + res1 + res2, leaving
    tile_stats / out_amax of the result where asked.  The three launches read raw tensors: x4 (in_amax: its producer's row;
    None: reduced into a row of `am`, or by the convolution itself), qkv and the attention output, whose exponents travel from
    epilogue to loader through rows of the arena `am` (None: fresh slots).  Buffers come from the pool `ws` (None: torch's
    allocator); attn_out: a [B, E, L] buffer of the caller's for the attention output.  cosine: unit queries and keys.
    folded: a FoldedAttention of the same block; where attention_folds() holds, the in-projection is its E -> E one, x4 itself
    serves as keys and values under its own exponent row, and the out-projection is the folded one -- same result up to
    rounding, a third of the in-projection's work.  Every other case launches what it launches without the bundle."""
    B, _, Hh, Ww = x4.shape
    L = Hh * Ww
    dev = x4.device

    def take(shape):
        return torch.empty(shape, dtype=torch.float32, device=dev) if ws is None else ws.take(shape, dev)

    def give(t):
        if ws is not None and t is not None:
            ws.give(t)

    if attention_folds(folded, E, L, heads, precision, cosine):
        a_q, a_o = (ops.amax_new(B, dev), ops.amax_new(B, dev)) if am is None else (am.row(), am.row())
        if in_amax is None:                                           # x4's own row: the in-projection's, the keys' and the values'
            in_amax = ops.absmax_rows(x4, B) if am is None else am.of(x4)
        q = ops.conv(x4, folded.w_q, bias=folded.b_q, out=take((B, E, Hh, Ww)), in_amax=in_amax, out_amax=a_q)
        aws = take((ops.attention_workspace_floats(B, E, L, precision),))
        o = ops.attention_xkv(q.view(B, E, L), x4.view(B, E, L), E, out=take((B, E, L)) if attn_out is None else attn_out,
                              workspace=aws, q_amax=a_q, x_amax=in_amax, out_amax=a_o)
        give(aws)
        y = ops.conv(o.view(B, E, Hh, Ww), folded.w_out, bias=folded.b_out, res1=res1, res2=res2, tile_stats=tile_stats,
                     out=take(x4.shape), in_amax=a_o, out_amax=out_amax)
        give(q)
        give(None if attn_out is not None else o)
        return y
    a_qkv = a_o = None
    if w_in.kind == "fp16x3":
        a_qkv, a_o = (ops.amax_new(2 * B, dev), ops.amax_new(B, dev)) if am is None else (am.rows(2), am.row())
        if in_amax is None and am is not None:
            in_amax = am.of(x4)
    split = 2 * E if E % 32 == 0 else 0                               # one exponent for q and k, one for v (E % 32: a channel tile of the epilogue)
    direct = split > 0 and not cosine
    qkv = ops.conv(x4, w_in, bias=b_in, out=take((B, 3 * E, Hh, Ww)),
                   **_amax_kw(w_in, in_amax=in_amax, out_amax=a_qkv if direct else None, amax_split=split if direct else 0))
    if cosine:
        # cosine_similarity (attention.py:362-372): unit queries and keys, logits without 1/sqrt(E) -- the
        # attention kernels scale by 1/sqrt(E), which the queries' gain cancels
        ops.token_l2_normalize(qkv.view(B, 3 * E, L), 0, E, eps=1e-8, gain=math.sqrt(E))
        ops.token_l2_normalize(qkv.view(B, 3 * E, L), E, E, eps=1e-8, gain=1.0)
    if a_qkv is not None and not direct:                              # q and k were rewritten, or a width the epilogue cannot split: measure
        ops.absmax_rows(qkv[:, :2 * E], out=a_qkv[:B])
        ops.absmax_rows(qkv[:, 2 * E:], out=a_qkv[B:])
    nws = ops.attention_workspace_floats(B, E, L, precision, heads=heads)
    aws = take((nws,)) if nws else None
    o = ops.attention(qkv.view(B, 3 * E, L), E, out=take((B, E, L)) if attn_out is None else attn_out, precision=precision,
                      workspace=aws, heads=heads, **_amax_kw(w_in, in_amax=a_qkv, out_amax=a_o))
    give(aws)
    y = ops.conv(o.view(B, E, Hh, Ww), w_out, bias=b_out, res1=res1, res2=res2, tile_stats=tile_stats, out=take(x4.shape),
                 **_amax_kw(w_out, in_amax=a_o, out_amax=out_amax))
    give(qkv)
    give(None if attn_out is not None else o)
    return y
