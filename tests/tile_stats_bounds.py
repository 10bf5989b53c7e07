"""The error model of the convolutions' tile statistics (ds_conv_epilogue.h, ds_conv3p.hip, ds_convup.hip, k_from_slices_stats of
ds_conv3d.hip), the data families that put an outlier at a pivot, and a numpy-fp32 emulation of the kernels' summation order (plain
numpy / torch, no GPU).  The vocabulary of tests/norm_bounds.py: u = 2^-24, k_tree(n) = ceil(log2 n) + 2, and every reference is fp64
of the fp32 values AS STORED by the convolution and read back, so the convolution's own accuracy is no part of the question.

A statistics entry t holds (K, sum(x - K), sum((x - K)^2), n) of n_t pixels; m_t is the entry's fp64 mean.  For a group of pixels
(a plane, GroupNorm's group, a sample) covered by entries t, N = sum n_t, m the group's fp64 mean:
    k_t  = k_tree(n_t) + 4
    dm_t = k_t u mean_t |x - m_t|
    |mean - mean64| <= dm = (1 / N) sum_t n_t dm_t
    |var  - var64 | <= dv = (1 / N) sum_t [k_t u sum_{x in t} (x - m_t)^2 + 2 n_t |m_t - m| dm_t] + 2^-51 mean64(x^2)
    rstd / table A:    rho = RHO0 + dv / (2 (var64 + eps))
    table M:           dm (+ u |mean64| where the mean is STORED as fp32: half an ulp of the result's own format)
  The bound is DEVIATION-based: a shift K that is an ordinary value of the entry leaves sums of deviations, whose fp32 tree carries
  k_tree(n_t) u of their magnitude; + 4 for the subtraction x - K, the square, and the two roundings of the recombination of the
  waves' partials about the entry's K.  It does not grow when the pivot is bad -- that is the point.  2 n_t |m_t - m| dm_t: an
  entry's contribution to the group's second moment about m moves by 2 (m_t - m) times the error of its sum.  The last term is
  norm_bounds' c64: the table kernels form q/n - mean^2 in fp64.

Entry geometry (entry_labels): 8 x 32 or 16 x 16 tiles as ds_conv_tile_count chooses, for the one-shot, persistent and 1x1 kernels;
four entries per low-resolution tile for ds_conv2d_h3_up (entry 4 t + 2 pa holds the rows of parity pa, entry 4 t + 2 pa + 1 is
empty); ds_volume_stat_tiles entries of a volume (workgroup bx of slice z visits the 256-value rows bx, bx + gx, ...).

The emulation (emulate_tile_stats) follows the 16-byte path (four-element vector sums, then the 16-lane pairwise tree per wave) or
the element-wise path (a 64-lane butterfly), then the fp32 recombination of the four waves about the tile's K, with the pivot rule
given: "first" (the wave's first pixel, the tile's K = wave 0's: what shipped before DESIGN 4.28), "med3" (full waves: the median of
three spread-out pixels (0, 0), (0, 20), (1, 8) of the wave's 2 x 32 block, ragged waves: the fp32 mean of the valid pixels; the
tile's K = the median of waves 0-2's, absent waves replaced by wave 0's: what ships now) or "mean" (the fp32 mean for every wave).
The first-pixel order sums a lane's four squares as four products and three sums, the others as one product and three fused
multiply-adds (ds_epi::sumsq4), each as its library does.
"""
import numpy as np
import torch

from tests import norm_bounds as nb
from tests.norm_bounds import U, RHO0, k_tree

f32 = np.float32


# ------------------------------------------------------------------------------------------------ geometry
def conv_geometry(H, W):
    """(TH, TW, rows per wave) of the one-shot, persistent and 1x1 kernels: mirrors ds_conv_tile_count."""
    pad32 = (W + 31) // 32 * 32 * ((H + 7) // 8 * 8)
    pad16 = (W + 15) // 16 * 16 * ((H + 15) // 16 * 16)
    return (16, 16, 4) if pad16 < pad32 else (8, 32, 2)


def up_geometry(Hl, Wl):
    """(TH, TW, rows per wave) of ds_conv2d_h3_up in LOW-resolution pixels."""
    if Hl % 8 == 0 and Wl % 32 == 0:
        return 8, 32, 2
    assert Hl % 16 == 0 and Wl % 16 == 0, "ds_conv2d_h3_up: whole 8 x 32 or 16 x 16 tiles"
    return 16, 16, 4


class Entries:
    """labels [H, W] (entry index of every pixel), n (entries per channel, empty ones included), first[e] = (y, x) of the entry's
    first pixel (None for an empty entry), wave_first[e][w] = first pixel of wave w of the entry (None where the wave has none)."""

    def __init__(self, labels, n, first, wave_first):
        self.labels, self.n, self.first, self.wave_first = labels, n, first, wave_first


def entry_labels(kind, H, W):
    """kind "conv": an H x W output of ds_conv2d_h3 / ds_conv2d_h3_pc / ds_conv1x1_h3; "up": an H x W OUTPUT of ds_conv2d_h3_up
    (H / 2 x W / 2 input); "volume": D = H slices of W = H' W' values each (k_from_slices_stats), labels [D, HW]."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    if kind == "conv":
        TH, TW, rw = conv_geometry(H, W)
        tx, ty = (W + TW - 1) // TW, (H + TH - 1) // TH
        labels = (yy // TH) * tx + xx // TW
        first = [(t // tx * TH, t % tx * TW) for t in range(tx * ty)]
        waves = [[(y + rw * w, x) if y + rw * w < H else None for w in range(4)] for y, x in first]
        return Entries(labels, tx * ty, first, waves)
    if kind == "up":
        TH, TW, rw = up_geometry(H // 2, W // 2)
        tx, ty = W // 2 // TW, H // 2 // TH
        labels = 4 * ((yy // 2 // TH) * tx + (xx // 2) // TW) + 2 * (yy & 1)
        first, waves = [], []
        for e in range(4 * tx * ty):
            t, pa, odd = e // 4, (e % 4) // 2, e % 2
            f = None if odd else (2 * (t // tx * TH) + pa, 2 * (t % tx * TW))
            first.append(f)
            waves.append([None] * 4 if odd else [(f[0] + 2 * rw * w, f[1]) for w in range(4)])
        return Entries(labels, 4 * tx * ty, first, waves)
    assert kind == "volume"
    D, HW = H, W
    gx = min(64, (HW + 1023) // 1024)
    labels = yy * gx + (xx // 256) % gx
    first = [(e // gx, (e % gx) * 256) for e in range(D * gx)]
    return Entries(labels, D * gx, first, [[f, None, None, None] for f in first])


# ------------------------------------------------------------------------------------------------ the bound
class TileStats(nb.Stats):
    """norm_bounds.Stats of groups x [..., N] whose pixels carry entry ids lab [..., N] (broadcast against x; ids need only be
    distinct inside a group), with the deviation-based dm, dv and rho of the module docstring.  stored32: the mean is judged as an
    fp32 number (tables, statistics rows): + u |mean64|."""

    def __init__(self, x, lab, eps, stored32=False):
        super().__init__(x, eps, 2, True)
        x = x.double()
        shape = x.shape
        N = shape[-1]
        x2 = x.reshape(-1, N)
        G = x2.shape[0]
        lab2 = lab.expand(shape).reshape(G, N).long()
        L = int(lab2.max()) + 1
        flat = (lab2 + L * torch.arange(G)[:, None]).reshape(-1)
        cnt = torch.zeros(G * L, dtype=torch.float64).index_add_(0, flat, torch.ones(G * N, dtype=torch.float64))
        sm = torch.zeros(G * L, dtype=torch.float64).index_add_(0, flat, x2.reshape(-1))
        m_t = sm / cnt.clamp_min(1.0)
        dev = x2.reshape(-1) - m_t[flat]
        a_t = torch.zeros(G * L, dtype=torch.float64).index_add_(0, flat, dev.abs())
        s_t = torch.zeros(G * L, dtype=torch.float64).index_add_(0, flat, dev * dev)
        k_t = torch.tensor([k_tree(int(c)) + 4 if c > 0 else 0 for c in cnt.tolist()], dtype=torch.float64)
        cnt, m_t, a_t, s_t, k_t = (v.reshape(G, L) for v in (cnt, m_t, a_t, s_t, k_t))
        m = self.mean.reshape(G, 1)
        n_dm_t = k_t * U * a_t                                                     # n_t dm_t
        self.dm = (n_dm_t.sum(-1) / N).reshape(self.mean.shape)
        self.dv = ((k_t * U * s_t + 2.0 * (m_t - m).abs() * n_dm_t).sum(-1) / N).reshape(self.mean.shape) + 2.0 ** -51 * self.ms
        if stored32:
            self.dm = self.dm + U * self.mean.abs()
        self.rho = RHO0 + self.dv / (2.0 * (self.var + self.eps))

    def var_ratio(self, var):
        err = (var.double() - self.var).abs()
        return float(torch.where(err == 0, torch.zeros_like(err), err / self.dv.clamp_min(1e-300)).max())

    def var_rel(self, var):
        return float(((var.double() - self.var).abs() / self.var.clamp_min(1e-300)).max())


def tile_sums(ts):
    """(K, S, Q, n) per entry [..., ntiles, 4] -> sums of x and x^2 and the count over the entries, in fp64 (as the table kernels)."""
    K, S, Q, n = torch.as_tensor(ts).double().unbind(-1)
    return (n * K + S).sum(-1), (Q + 2 * K * S + n * K * K).sum(-1), n.sum(-1)


# ------------------------------------------------------------------------------------------------ the pivot-outlier families
P_FAMILIES = ("P00", "Pw2", "Pt", "Plast", "Pblock")
CONTROLS = ("Pnext", "Pmid")
EDGES = ("Ecol", "Erow", "Eboth")


def outlier_pixels(name, ent):
    """The (y, x) pixels of a plane that family `name` replaces, for the entry geometry ent."""
    live = [e for e in range(ent.n) if ent.first[e] is not None]
    if name == "P00":
        return [(0, 0)]
    if name == "Pw2":
        return [ent.wave_first[live[0]][2]]
    if name == "Pt":
        return [ent.first[e] for e in live]
    if name == "Plast":
        return [ent.first[live[-1]]]
    if name == "Pblock":
        return [(0, 0), (0, 1), (1, 0), (1, 1)]
    if name == "Pnext":
        return [(0, 1)]
    assert name == "Pmid"
    return [(1, 5)]


def place(name, x, ent, M):
    """Family `name` on planes x [..., H, W] (fp32, changed in place and returned).  P / control families: the named pixels = M;
    Ecol / Erow: + 30 on the first column / row; Eboth: first row and column scaled by 0.66 (the signature of zero padding)."""
    if name == "Ecol":
        x[..., :, 0] += 30.0
    elif name == "Erow":
        x[..., 0, :] += 30.0
    elif name == "Eboth":
        x[..., 0, :] *= 0.66
        x[..., 1:, 0] *= 0.66
    else:
        for y, xx in outlier_pixels(name, ent):
            x[..., y, xx] = M
    return x


# ------------------------------------------------------------------------------------------------ the emulation
def _med3(a, b, c):
    return f32(max(min(a, b), min(max(a, b), c)))


def _pairwise(v):
    """Adjacent pairwise tree of a power-of-two fp32 vector: the 16-lane DPP tree (quad 1, quad 2, half mirror, ror 8)."""
    v = v.astype(f32)
    while v.size > 1:
        v = (v[0::2] + v[1::2]).astype(f32)
    return f32(v[0])


def _butterfly(v):
    """__shfl_xor 32, 16, ..., 1 over 64 lanes."""
    v = v.astype(f32)
    while v.size > 1:
        h = v.size // 2
        v = (v[:h] + v[h:]).astype(f32)
    return f32(v[0])


def _wave(block, valid, order, pivot):
    """One wave's (K, S, Q, n) of its [2][32] block (fp32) with validity mask."""
    n = int(valid.sum())
    if n == 0:
        return f32(0), f32(0), f32(0), f32(0)
    zero = np.where(valid, block, f32(0)).astype(f32)
    if order == "vec":
        total = _pairwise(((zero[:, 0::4] + zero[:, 1::4]) + (zero[:, 2::4] + zero[:, 3::4])).reshape(-1))
    else:
        total = _butterfly(zero.reshape(-1))
    if pivot == "first":
        K = block[0, 0]
    elif pivot == "med3" and n == 64:
        K = _med3(block[0, 0], block[0, 20], block[1, 8])
    else:
        K = f32(total * f32(f32(1) / f32(n)))
    d = np.where(valid, (block - K).astype(f32), f32(0)).astype(f32)
    q = (d * d).astype(f32)
    if order == "vec":
        S = _pairwise(((d[:, 0::4] + d[:, 1::4]) + (d[:, 2::4] + d[:, 3::4])).reshape(-1))
        if pivot == "first":                                              # as shipped then: four products, three sums
            Q = _pairwise(((q[:, 0::4] + q[:, 1::4]) + (q[:, 2::4] + q[:, 3::4])).reshape(-1))
        else:                                                             # sumsq4: one product, three fused multiply-adds
            acc = q[:, 3::4]
            for j in (2, 1, 0):
                acc = (d[:, j::4].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(f32)
            Q = _pairwise(acc.reshape(-1))
    else:
        S, Q = _butterfly(d.reshape(-1)), _butterfly(q.reshape(-1))
    return f32(K), S, Q, f32(n)


def emulate_tile_stats(plane, order="vec", pivot="first"):
    """plane [H, W] fp32 (numpy) -> [ntiles, 4] fp32 as the one-shot kernels leave them."""
    plane = np.asarray(plane, dtype=f32)
    H, W = plane.shape
    assert order in ("vec", "elem") and pivot in ("first", "med3", "mean") and (order == "elem" or W % 4 == 0)
    TH, TW, rw = conv_geometry(H, W)
    tx, ty = (W + TW - 1) // TW, (H + TH - 1) // TH
    out = np.zeros((tx * ty, 4), dtype=f32)
    r, x = np.meshgrid(np.arange(2), np.arange(32), indexing="ij")
    for t in range(tx * ty):
        y0, x0 = t // tx * TH, t % tx * TW
        p = []
        for w in range(4):
            gy = y0 + rw * w + (r if rw == 2 else 2 * r + (x >> 4))
            gx = x0 + (x if rw == 2 else (x & 15))
            valid = (gy < H) & (gx < W)
            block = np.where(valid, plane[np.minimum(gy, H - 1), np.minimum(gx, W - 1)], f32(0)).astype(f32)
            p.append(_wave(block, valid, order, pivot))
        if pivot == "first":
            K = p[0][0]
        else:
            K = _med3(p[0][0], p[1][0] if p[1][3] > 0 else p[0][0], p[2][0] if p[2][3] > 0 else p[0][0])
        S = Q = n = f32(0)
        for Kw, Sw, Qw, nw in p:
            dk = f32(Kw - K) if nw > 0 else f32(0)
            S = f32(S + f32(Sw + f32(nw * dk)))
            Q = f32(Q + f32(f32(Qw + f32(f32(f32(2) * dk) * Sw)) + f32(f32(nw * dk) * dk)))
            n = f32(n + nw)
        out[t] = (K, S, Q, n)
    return out
