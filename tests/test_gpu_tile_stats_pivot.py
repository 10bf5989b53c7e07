"""The convolutions' tile statistics (K, sum(x - K), sum((x - K)^2), n) with an outlier where the shift K is taken: the default norm
route of PUNetG, ADM and the LDM / VAENet decoders (ds_inorm_table, ds_gnorm1_table, ds_gnorm1_stats_tiles, ds_groupnorm_stats_tiles,
ds_groupnorm_table and the fused loaders), which no other test feeds such data.  The error model, the entry geometry and the
families: tests/tile_stats_bounds.py (checked on the CPU by tests/test_tile_stats_bounds.py); DESIGN 4.28.  Every reference is fp64
of the stored output as read back.  Every case prints its ratios (pytest -s).

The outliers are placed through the residual: the statistics are of the stored value, which includes it, so a residual that is zero
except at chosen pixels puts M (plus the convolution's own value) exactly where it is wanted.  They go into every second channel, so
that hit and clean channels sit side by side; entries without an outlier must be bit-equal to the launch without the residual.

The kernel selections behind DS_CONV_SHAPE, DS_CONV_WAVES16 and DS_CONV_TWO are read once per process: test_switched_selections
runs this file's __main__ (the one-shot and 1x1 cases) in one child process per setting.
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from tests import norm_bounds as nb  # noqa: E402
from tests import tile_stats_bounds as tb  # noqa: E402
from tests.norm_bounds import U, RHO0, rel_l2  # noqa: E402

EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


class Findings:
    """Prints every ratio, remembers those above 1, and fails at the end of the case with all of them."""

    def __init__(self):
        self.bad = []

    def report(self, what, **ratios):
        print(f"{what}: " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in ratios.items()))
        self.bad += [(what, k, round(v, 3)) for k, v in ratios.items() if not v <= 1.0]

    def require(self, ok, what):
        if not ok:
            print(f"{what}: FAILED")
            self.bad.append(what)

    def done(self):
        assert not self.bad, self.bad


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ producers
# prod: "3x3" ds_conv2d_h3 one-shot, "1x1" ds_conv1x1_h3, "pc" ds_conv2d_h3_pc persistent, "up" ds_conv2d_h3_up.
# opts: prenorm (the producer's own loader normalises), mode2 (nearest-upsampling load), via ("res1" | "res2" | "res1_up"), big
# (check samples 0 and B - 1 only).  The instantiation each shape reaches: DESIGN 4.28.
def _case(prod, B, Cin, Cout, H, W, fams, **opts):
    name = f"{prod} B{B} {Cin}->{Cout} {H}x{W}" + "".join(f" {k}={v}" for k, v in opts.items())
    return pytest.param((prod, B, Cin, Cout, H, W, fams, opts), id=name.replace(" ", "-"))


ALL = ("P00:1e6", "P00:1e2", "P00:-3e4", "Pw2:1e6", "Pt:1e6", "Pt:1e2", "Plast:1e6", "Pblock:1e6", "Pblock:1e2", "Pnext:1e6",
       "Pmid:1e6", "Ecol", "Erow", "Eboth", "P00:1e6@B1e3", "Pt:1e6@B1e3")
FEW = ("P00:1e6", "Pw2:1e6", "Pt:1e2", "Plast:1e6", "Pblock:1e6", "Pmid:1e6", "Ecol", "Erow", "Eboth")
BIG = ("P00:1e6", "Pw2:1e6", "Pt:1e6", "Pblock:1e2", "Ecol")

ONE_SHOT = [
    _case("3x3", 2, 16, 16, 16, 32, ALL),                                 # 8 x 32 tiles, two tiles; one chunk: 32x32x16, four waves
    _case("3x3", 2, 64, 64, 16, 16, ALL),                                 # 16 x 16 geometry, four rows per wave; 16x16x32
    _case("3x3", 1, 40, 40, 20, 36, ALL),                                 # ragged tiles and channels
    _case("3x3", 1, 8, 8, 9, 13, ALL),                                    # W & 3 != 0: the element-wise path
    _case("3x3", 1, 32, 72, 16, 32, FEW),                                 # Cout > 64: two channel tiles; 16x16x32, 16-byte staging
    _case("3x3", 2, 16, 16, 16, 32, FEW, prenorm=True),                   # fused prenorm: the eight-wave 32x32x16 kernel (MT = 1)
    _case("3x3", 1, 32, 32, 16, 64, FEW, prenorm=True),                   # fused prenorm, 16x16x32
    _case("3x3", 1, 16, 16, 16, 32, FEW, mode2=True),                     # nearest-upsampling load
    _case("3x3", 2, 16, 16, 16, 32, FEW, via="res2"),
    _case("3x3", 2, 16, 16, 16, 32, ("Pblock:1e6", "Pblock:1e2", "Pt:1e6"), via="res1_up"),
    _case("1x1", 2, 16, 16, 16, 32, ALL),
    _case("1x1", 2, 64, 64, 16, 16, FEW),
    _case("1x1", 1, 40, 40, 20, 36, FEW),
    _case("1x1", 1, 8, 8, 9, 13, FEW),
    _case("1x1", 1, 32, 128, 16, 32, FEW),
]
OTHERS = [
    _case("pc", 32, 64, 64, 32, 64, BIG, big=True),                       # persistent, raw input (pc_raw)
    _case("pc", 32, 64, 64, 32, 64, BIG, big=True, prenorm=True),         # persistent, fused prenorm
    _case("3x3", 32, 32, 128, 32, 64, BIG, big=True, prenorm=True),       # two channel tiles per workgroup (chosen by shape: 256 workgroups)
    _case("up", 2, 16, 16, 16, 64, ALL),                                  # Hl x Wl = 8 x 32
    _case("up", 2, 32, 32, 32, 32, ALL),                                  # Hl x Wl = 16 x 16
    _case("up", 1, 32, 72, 16, 64, FEW, via="res2"),
]


def _residual(fam, base, M, B, C, H, W, ent, low):
    """The residual that turns the base output into family fam: [B, C, H, W] (low: [B, C, H / 2, W / 2], added nearest-upsampled).
    Every second channel (0, 2, ...) is hit."""
    r = torch.zeros(B, C, H // 2 if low else H, W // 2 if low else W)
    hit = torch.arange(0, C, 2)
    if fam == "Ecol":
        r[:, hit, :, 0] = 30.0
    elif fam == "Erow":
        r[:, hit, 0, :] = 30.0
    elif fam == "Eboth":                                                    # base B(1e3): 1000 -> 660 on the first row and column
        r[:, hit, 0, :] = -340.0
        r[:, hit, :, 0] = -340.0
    else:
        pix = tb.outlier_pixels(fam, ent)
        if low:
            pix = sorted({(y // 2, x // 2) for y, x in pix})
        for b in range(B):
            for c in hit.tolist():
                for y, x in pix:
                    r[b, c, y, x] = M[b, c]
    return r, hit


def _produce(ops, dev, case, g):
    """-> launch(res) that runs the producer with the given residual (or None) and returns (y, tile_stats)."""
    prod, B, Cin, Cout, H, W, fams, opts = case
    k = 1 if prod == "1x1" else 3
    lowin = prod == "up" or opts.get("mode2", False)
    Hin, Win = (H // 2, W // 2) if lowin else (H, W)
    x = (torch.randn(B, Cin, Hin, Win, generator=g) * 1.5 + 0.2).to(dev)
    wt = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    kw = {}
    if opts.get("prenorm"):
        w0 = torch.randn(Cin, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
        ts0 = torch.zeros(B, Cin, ops.conv_tile_count(Hin, Win), 4, device=dev)
        x = ops.conv(x, ops.pack_conv(w0.to(dev), "fp16x3"), tile_stats=ts0)
        wn, bn = torch.randn(Cin, generator=g).to(dev), torch.randn(Cin, generator=g).to(dev)
        kw["prenorm"] = ops.inorm_table(ts0, wn, bn, 0, Hin * Win, eps=EPS)
    if lowin:
        kw["load_mode"] = 2
    if prod == "pc" and not opts.get("prenorm"):
        kw["pc_raw"] = True
    via = opts.get("via", "res1")

    def launch(res, scale, offset):
        """y = scale-d convolution + offset (+ residual): family A is scale 3, offset 0.7; B(1e3) scale 1, offset 1000."""
        pws = ops.pack_conv((wt * scale).to(dev), "fp16x3", upsampled=prod == "up")
        ts = torch.full((B, Cout, ops.conv_tile_count(H, W), 4), float("nan"), device=dev)
        rk = {}
        if res is not None:
            rk = {"res2": res.to(dev)} if via == "res2" else {"res1": res.to(dev), "res1_upsampled": via == "res1_up"}
        y = ops.conv(x, pws, bias=torch.full((Cout,), offset, device=dev), tile_stats=ts, **rk, **kw)
        return y, ts

    return launch


BASES = {"A": (3.0, 0.7), "B1e3": (1.0, 1000.0)}


def _magnitudes(mname, B, C, g):
    if mname == "1e6":
        return 1e6 * (1.0 + 0.1 * torch.rand(B, C, generator=g))
    return torch.full((B, C), float(mname))


# ------------------------------------------------------------------------------------------------ the checks
def _a_ratio(A, want, rho):
    """Table column A against rstd64 w: rho plus two u for the products with w and the FiLM factor."""
    return float(((A.double() / want - 1.0).abs() / (rho + 2.0 * U)).max())


def _check_exponent(f, what, tab, y64, C):
    """Fourth column: 2^-k, one per sample, max |(y - M) A + C| 2^k inside (2^5, 2^14) unless |k| = 80 clamps."""
    t = tab.cpu().double()
    inv = t[..., 3]
    f.require(bool((inv == inv[:, :1]).all() and (torch.log2(inv[:, 0]) % 1 == 0).all()), f"{what}: one power of two per sample")
    t = t[:, :C]
    arg = ((y64 - t[..., 0, None, None]) * t[..., 1, None, None] + t[..., 2, None, None]).abs().amax(dim=(1, 2, 3))
    scaled, k = arg / inv[:, 0], -torch.log2(inv[:, 0])
    f.require(bool((scaled < 2.0 ** 14).all() and ((scaled > 2.0 ** 5) | (k.abs() == 80)).all()),
              f"{what}: max |arg| 2^k = 2^{[round(math.log2(max(float(v), 1e-300)), 2) for v in scaled]} outside (2^5, 2^14)")


def _check_statistics(f, ops, tag, y, ts, yb, tsb, lab, erow, g):
    """Everything the issue lists, of y [B, C, H, W] (device) with tile statistics ts against fp64 of y; (yb, tsb): the launch
    without the residual, the second source of the two-source table.  erow: the border-row family, held to 1e-5 only."""
    dev = y.device
    B, C, H, W = y.shape
    n = H * W
    yc, ybc = y.cpu().double(), yb.cpu().double()
    nt = ts.shape[2]
    f.require(bool(torch.isfinite(ts).all() and torch.isfinite(y).all()), f"{tag}: finite")
    sx, sxx, cnt = tb.tile_sums(ts.cpu())
    f.require(bool((cnt == n).all()), f"{tag}: counts")
    want_n = torch.bincount(lab.reshape(-1), minlength=nt).float()
    f.require(bool((ts[..., 3].cpu() == want_n).all()), f"{tag}: the count of every entry")
    plab = lab.reshape(1, 1, n)
    planes = tb.TileStats(yc.reshape(B, C, n), plab, EPS)
    planes32 = tb.TileStats(yc.reshape(B, C, n), plab, EPS, stored32=True)
    var = sxx / n - (sx / n) ** 2
    print(f"{tag}: plane variance from the tiles, relative error {planes.var_rel(var):.2e}")
    if erow:
        print(f"{tag}: [reported] plane mean error / bound = {planes.mean_ratio(sx / n):.3f}, variance error / bound = {planes.var_ratio(var):.3f}")
        f.report(f"{tag} plane variance against 1e-5", variance=planes.var_rel(var) / 1e-5)
    else:
        f.report(f"{tag} plane from the tiles", mean=planes.mean_ratio(sx / n), variance=planes.var_ratio(var))
    w, b, film = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(B, 2 * C, generator=g) * 0.5
    w = torch.where(w.abs() < 0.1, torch.full_like(w, 0.5), w)
    wd, bd, fd = w.to(dev), b.to(dev), film.to(dev)

    def rows(what, tab, st, w64, kind, c_want):
        """Table rows [B, C, 0:3]: M to dm (kind 0; zero for kind 1), A to rho, C exact."""
        t = tab[:, :C].cpu()
        if kind == 0:
            got = {"M": st.mean_ratio(t[..., 0]), "A": _a_ratio(t[..., 1], st.rstd * w64, st.rho)}
        else:
            f.require(not t[..., 0].any(), f"{what}: M = 0")
            got = {"A": _a_ratio(t[..., 1], w64 / st.rms_den, st.rho_rms)}
        if erow:
            print(f"{what}: [reported] " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in got.items()))
            a_want = (st.rstd if kind == 0 else 1.0 / st.rms_den) * w64
            f.report(f"{what} against 1e-5", A=float(((t[..., 1].double() / a_want - 1).abs()).max()) / 1e-5)
        else:
            f.report(what, **got)
        f.require(torch.equal(t[..., 2], c_want.float().expand(B, C)), f"{what}: C exact")
        f.require(not tab[:, C:, :3].any(), f"{what}: zero rows pad the last chunk")

    # one row of statistics per sample, entries = (channel, tile)
    slab = (lab.reshape(1, n) + nt * torch.arange(C)[:, None]).reshape(1, C * n)
    sample = _with_rms(tb.TileStats(yc.reshape(B, C * n), slab, EPS, stored32=True))
    planes32 = _with_rms(planes32)
    for kind in (0, 1):
        tab = ops.inorm_table(ts, wd, bd, kind, n, eps=EPS)
        rows(f"{tag} inorm_table kind {kind}", tab, planes32, w.double()[None, :], kind, b)
        _check_exponent(f, f"{tag} inorm_table kind {kind}", tab, yc, C)
        for fl in (None, fd):
            tab = ops.gnorm1_table(ts, wd, bd, kind, C * n, film=fl, eps=EPS)
            t1 = film[:, :C] if fl is not None else torch.ones(B, C)
            t2 = film[:, C:] if fl is not None else torch.zeros(B, C)
            what = f"{tag} gnorm1_table kind {kind} film {fl is not None}"
            rows(what, tab, _expand(sample, C), (w * t1).double(), kind, b * t1 + t2)
            _check_exponent(f, what, tab, yc, C)
        st_t = ops.gnorm1_stats_tiles(ts, kind, C * n, eps=EPS).cpu()
        st_x = ops.gnorm1_stats(y, kind, eps=EPS).cpu()
        own = nb.Stats(yc.reshape(B, C * n), EPS, 2, True)
        if kind == 0:
            got = {"mean": sample.mean_ratio(st_t[:, 0]), "rstd": sample.rstd_ratio(st_t[:, 1])}
            if erow:
                print(f"{tag} gnorm1_stats_tiles: [reported] " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in got.items()))
                f.report(f"{tag} gnorm1_stats_tiles against 1e-5", rstd=float((st_t[:, 1].double() / sample.rstd - 1).abs().max()) / 1e-5)
            else:
                f.report(f"{tag} gnorm1_stats_tiles", **got)
            f.report(f"{tag} gnorm1_stats", mean=own.mean_ratio(st_x[:, 0]), rstd=own.rstd_ratio(st_x[:, 1]))
        else:
            f.require(not st_t[:, 0].any() and not st_x[:, 0].any(), f"{tag}: RMS statistics have no mean")
            r = float(((st_t[:, 1].double() / sample.rms_den - 1.0).abs() / sample.rho_rms).max())
            if erow:
                print(f"{tag} gnorm1_stats_tiles kind 1: [reported] rms error / bound = {r:.3f}")
            else:
                f.report(f"{tag} gnorm1_stats_tiles kind 1", rms=r)
            f.report(f"{tag} gnorm1_stats kind 1", rms=own.rms_ratio(st_x[:, 1]))
    # two sources: the statistics of a channel concatenation with the launch without the residual
    ycat = torch.cat([yc, ybc], 1)
    clab = (lab.reshape(1, n) + nt * torch.arange(2 * C)[:, None]).reshape(1, 2 * C * n)
    both = _with_rms(tb.TileStats(ycat.reshape(B, 2 * C * n), clab, EPS, stored32=True))
    w2, b2 = torch.cat([w, -w]), torch.cat([b, b + 1])
    for kind in (0, 1):
        tab = ops.gnorm1_table(ts, w2.to(dev), b2.to(dev), kind, 2 * C * n, stats_b=tsb, eps=EPS)
        what = f"{tag} gnorm1_table of two sources kind {kind}"
        t = tab[:, :2 * C].cpu()
        st = _expand(both, 2 * C)
        if kind == 0:
            got = {"M": st.mean_ratio(t[..., 0]), "A": _a_ratio(t[..., 1], st.rstd * w2.double(), st.rho)}
        else:
            got = {"A": _a_ratio(t[..., 1], w2.double() / st.rms_den, st.rho_rms)}
        if erow:
            print(f"{what}: [reported] " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in got.items()))
        else:
            f.report(what, **got)
        _check_exponent(f, what, tab, ycat, 2 * C)
    # GroupNorm(C / 4, C)
    if C % 4 == 0:
        G = C // 4
        glab = (lab.reshape(1, n) + nt * torch.arange(4)[:, None]).reshape(1, 1, 4 * n)
        grp = tb.TileStats(yc.reshape(B, G, 4 * n), glab, 1e-6, stored32=True)
        gt = ops.groupnorm_stats_tiles(ts, G, n, eps=1e-6).cpu()
        got = {"mean": grp.mean_ratio(gt[..., 0]), "rstd": grp.rstd_ratio(gt[..., 1])}
        if erow:
            print(f"{tag} groupnorm_stats_tiles: [reported] " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in got.items()))
            f.report(f"{tag} groupnorm_stats_tiles against 1e-5", rstd=float((gt[..., 1].double() / grp.rstd - 1).abs().max()) / 1e-5)
        else:
            f.report(f"{tag} groupnorm_stats_tiles", **got)
        tab = ops.groupnorm_table(wd, bd, G, n, tile_stats=ts, eps=1e-6)
        t = tab[:, :C].cpu().reshape(B, G, 4, 4)
        got = {"M": max(grp.mean_ratio(t[:, :, i, 0]) for i in range(4)),
               "A": max(_a_ratio(t[:, :, i, 1], grp.rstd * w.double().reshape(1, G, 4)[:, :, i], grp.rho) for i in range(4))}
        if erow:
            print(f"{tag} groupnorm_table: [reported] " + ", ".join(f"{k} error / bound = {v:.3f}" for k, v in got.items()))
        else:
            f.report(f"{tag} groupnorm_table", **got)
        _check_exponent(f, f"{tag} groupnorm_table", tab, yc, C)


def _with_rms(st):
    """The RMS kinds from the tiles: mean(x^2) = var + mean^2 moves by dv + 2 |mean| dm."""
    d_ms = st.dv + 2.0 * st.mean.abs() * st.dm
    st.rho_rms = RHO0 + d_ms / (2.0 * (st.ms + st.eps))
    return st


class _Rows:
    pass


def _expand(st, C):
    """Per-sample statistics [B] as per-channel rows [B, C]."""
    r = _Rows()
    for k in ("mean", "var", "ms", "rstd", "rms_den", "dm", "dv", "rho", "rho_rms"):
        setattr(r, k, getattr(st, k)[:, None].expand(-1, C))
    r.mean_ratio = lambda m: nb.Stats.mean_ratio(r, m)
    return r


def _check_pivots(f, tag, prod, y, ts, ent):
    """The shift of a tile whose first three waves are full is one of nine stored values: the median of the medians of three
    pixels of each wave (pins the geometry this file assumes and the rule of DESIGN 4.28)."""
    B, C, H, W = y.shape
    yc, K = y.cpu(), ts[..., 0].cpu()
    if prod == "up":
        TH, TW, rw = tb.up_geometry(H // 2, W // 2)
        offs = [(0, 0), (0, 20), (0, 40)] if rw == 2 else [(0, 0), (0, 20), (2, 8)]
    else:
        TH, TW, rw = tb.conv_geometry(H, W)
        offs = [(0, 0), (0, 20), (1, 8)] if rw == 2 else [(0, 0), (1, 4), (2, 8)]
    if W % 4:
        return
    checked = 0
    for e in range(ent.n):
        if ent.first[e] is None:
            f.require(not ts[:, :, e].any(), f"{tag}: empty entry {e} is zero")
            continue
        y0, x0 = ent.first[e]
        span = 2 if prod == "up" else 1
        if y0 + span * TH > H or x0 + span * TW > W:
            continue
        cand = torch.stack([yc[:, :, wy + dy, wx + dx] for wy, wx in ent.wave_first[e][:3] for dy, dx in offs], -1)
        f.require(bool((cand.view(torch.int32) == K[:, :, e, None].view(torch.int32)).any(-1).all()), f"{tag}: K of entry {e} is one of its candidates")
        checked += 1
    assert checked


def _run(ops, dev, case, seed=0):
    prod, B, Cin, Cout, H, W, fams, opts = case
    g = torch.Generator().manual_seed(1000 + seed + B + Cin + Cout + H + W)
    f = Findings()
    ent = tb.entry_labels("up" if prod == "up" else "conv", H, W)
    launch = _produce(ops, dev, case, g)
    sel = [0, B - 1] if opts.get("big") else list(range(B))
    clean = {}
    low = opts.get("via") == "res1_up"
    for fam_spec in fams:
        fam, _, base = fam_spec.partition("@")
        fam, _, mname = fam.partition(":")
        base = base or ("B1e3" if fam == "Eboth" else "A")
        if base not in clean:
            y0, ts0 = launch(None, *BASES[base])
            clean[base] = (y0[sel].contiguous(), ts0[sel].contiguous())
        yb, tsb = clean[base]
        M = _magnitudes(mname, B, Cout, g) if mname else None
        res, hit = _residual(fam, base, M, B, Cout, H, W, ent, low)
        y, ts = launch(res, *BASES[base])
        y, ts = y[sel].contiguous(), ts[sel].contiguous()
        tag = f"{prod} {B}x{Cin}->{Cout}x{H}x{W}{' ' + str(opts) if opts else ''} {fam_spec}"
        # entries that hold no outlier: bit-equal to the launch without the residual
        touched = torch.zeros(ent.n, dtype=torch.bool)
        rs = F.interpolate(res[0, 0][None, None], scale_factor=2.0, mode="nearest")[0, 0] if low else res[0, 0]
        touched[ent.labels[rs != 0].unique()] = True
        keep = torch.ones(Cout, ent.n, dtype=torch.bool)
        keep[hit[:, None], touched.nonzero().reshape(1, -1)] = False
        f.require(same_bits(ts.cpu()[:, keep], tsb.cpu()[:, keep]), f"{tag}: entries without an outlier are bit-equal to the clean launch")
        f.require(not same_bits(ts.cpu()[:, ~keep], tsb.cpu()[:, ~keep]), f"{tag}: the residual reached the statistics")
        _check_pivots(f, tag, prod, y, ts, ent)
        _check_statistics(f, ops, tag, y, ts, yb, tsb, ent.labels, fam == "Erow", g)
        if fam in ("P00", "Pblock"):
            _check_fused_loader(f, ops, tag, y, ts, yb, tsb, ent.labels, g)
    f.done()


def _check_fused_loader(f, ops, tag, y, ts, yb, tsb, lab, g):
    """conv(y, prenorm = table) against fp64 conv(SiLU(norm64(y))), norm64 from the fp64 statistics of y; the same for the clean
    launch, whose figure replaces 3e-6 where it is already larger."""
    dev = y.device
    B, C, H, W = y.shape
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    wt = torch.randn(8, C, 3, 3, generator=g) / math.sqrt(9 * C)
    pw = ops.pack_conv(wt.to(dev), "fp16x3")
    errs = []
    for yy, tt in ((yb, tsb), (y, ts)):
        yc = yy.cpu().double()
        mean, var = yc.mean(dim=(2, 3), keepdim=True), yc.var(dim=(2, 3), unbiased=False, keepdim=True)
        act = nb.silu64((yc - mean) / torch.sqrt(var + EPS) * w.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1))
        want = F.conv2d(act, wt.double(), padding=1)
        got = ops.conv(yy, pw, prenorm=ops.inorm_table(tt, w.to(dev), b.to(dev), 0, H * W, eps=EPS))
        f.require(bool(torch.isfinite(got).all()), f"{tag}: fused loader finite")
        errs.append(rel_l2(got.cpu(), want))
    bound = max(3e-6, errs[0])
    print(f"{tag}: fused loader rel-L2 {errs[1]:.2e} (clean launch {errs[0]:.2e}), bound {bound:.1e}, ratio {errs[1] / bound:.3f}")
    f.require(errs[1] <= bound, f"{tag}: fused loader rel-L2 {errs[1]:.2e} above {bound:.1e}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", ONE_SHOT)
def test_one_shot_and_1x1(dev, ops, case):
    _run(ops, dev, case.values[0] if hasattr(case, "values") else case)


@pytest.mark.parametrize("case", OTHERS)
def test_persistent_two_tile_and_parity(dev, ops, case):
    _run(ops, dev, case.values[0] if hasattr(case, "values") else case)


@pytest.mark.parametrize("HW", [(8, 32), (40, 40)], ids=["one workgroup per slice", "two workgroups per slice"])
def test_volume_statistics(dev, ops, HW):
    """The contrast: k_from_slices_stats (ds_conv3d.hip) shifts by the mean of a workgroup's first 256 values.  The outlier is the
    first value of a workgroup's first 256."""
    B, C, D = 1, 16, 2
    H, W = HW
    n = D * H * W
    f = Findings()
    g = torch.Generator().manual_seed(43 + H)
    x = torch.randn(B, C, D, H, W, generator=g).to(dev)
    wt = 3.0 * torch.randn(C, C, 3, 3, 3, generator=g) / math.sqrt(27 * C)
    packs = ops.pack_conv3d(wt.to(dev))
    bias = torch.full((C,), 0.7, device=dev)
    ent = tb.entry_labels("volume", D, H * W)
    nt = ops.volume_stat_tiles(D, H * W)
    assert nt == ent.n
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    for mname in ("1e6", "1e2", "-3e4"):
        M = _magnitudes(mname, B, C, g)
        res = torch.zeros(B, C, D, H * W)
        for e in (0, ent.n - 1):
            z, i = ent.first[e]
            res[:, 0::2, z, i] = M[:, 0::2]
        st = torch.full((B, C, nt, 4), float("nan"), device=dev)
        h = ops.conv3d_mfma(x, packs, bias=bias, res1=res.reshape(B, C, D, H, W).to(dev), out_stats=st)
        hc = h.cpu().double().reshape(B, C, n)
        tag = f"volume {D}x{H}x{W} first-of-256 M={mname}"
        f.require(bool(torch.isfinite(st).all()), f"{tag}: finite")
        want_n = torch.bincount(ent.labels.reshape(-1), minlength=nt).float()
        f.require(bool((st[..., 3].cpu() == want_n).all()), f"{tag}: the count of every entry")
        sx, sxx, cnt = tb.tile_sums(st.cpu())
        planes = tb.TileStats(hc, ent.labels.reshape(1, 1, n), EPS)
        f.report(f"{tag} from the entries", mean=planes.mean_ratio(sx / n), variance=planes.var_ratio(sxx / n - (sx / n) ** 2))
        p32 = _with_rms(tb.TileStats(hc, ent.labels.reshape(1, 1, n), EPS, stored32=True))
        for kind in (0, 1):
            t = ops.inorm_table(st, w.to(dev), b.to(dev), kind, n, eps=EPS)[:, :C].cpu()
            if kind == 0:
                f.report(f"{tag} inorm_table kind 0", M=p32.mean_ratio(t[..., 0]), A=_a_ratio(t[..., 1], p32.rstd * w.double(), p32.rho))
            else:
                f.report(f"{tag} inorm_table kind 1", A=_a_ratio(t[..., 1], w.double() / p32.rms_den, p32.rho_rms))
    f.done()


SWITCHES = [{"DS_CONV_SHAPE": "32"}, {"DS_CONV_WAVES16": "8"}, {"DS_CONV_TWO": "2", "DS_CONV1_TWO": "2"},
            {"DS_CONV_TWO": "0", "DS_CONV1_TWO": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=["mfma-32x32x16", "16x16x32-eight-waves", "two-channel-tiles-everywhere", "one-channel-tile"])
def test_switched_selections(env):
    """The one-shot and 1x1 cases with the kernel selections the library keeps behind environment switches, which are read once
    per process: hence the child process."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all switched cases passed" in r.stdout


def _main():
    from diffsci_amd import ops
    dev = torch.device("cuda:0")
    short = ("P00:1e6", "Pw2:1e6", "Pt:1e2", "Plast:1e6", "Pblock:1e6", "Ecol")
    extra = [("3x3", 1, 32, 128, 16, 32, short, {}), ("3x3", 1, 32, 128, 16, 32, short, {"prenorm": True}),
             ("3x3", 1, 64, 64, 16, 16, short, {"prenorm": True})]
    bad = []
    for case in [c.values[0][:6] + (short, c.values[0][7]) for c in ONE_SHOT] + extra:
        try:
            _run(ops, dev, case)
        except AssertionError as e:
            bad.append((case[:6], case[7], str(e)[:2000]))
    for b in bad:
        print("FAILED", b)
    if bad:
        sys.exit(1)
    print("all switched cases passed")


if __name__ == "__main__":
    _main()
