"""The error model of tests/tile_stats_bounds.py must discriminate, and must do so without a GPU: a numpy-fp32 emulation of the
convolution epilogue's tile statistics with the FIRST-PIXEL pivot (what shipped before DESIGN 4.28) misses the bound by a wide
margin wherever an outlier sits at a pivot, the same order with a robust pivot (the shipped median of three spread-out pixels, or
the mean) stays far inside it, and both stay inside it on the data the suite fed them before.  Run with -s for the ratios."""
import numpy as np
import pytest
import torch

from tests import norm_bounds as nb
from tests import tile_stats_bounds as tb

EPS = 1e-5
PLANES = [(8, 32), (16, 64), (32, 96), (16, 16), (20, 36)]            # one tile, 8 x 32 tiles, more tiles, 16 x 16 geometry, ragged
C = 6                                                                 # channels of a sample: the ratios are the worst channel's
MS = ("1e2", "1e6", "-3e4")


def _plane(fam, H, W, seed=0):
    return nb.family(fam, (C, H, W), seed)


def _magnitude(mname):
    """M per channel: 1e2, 1e6 (1 + 0.1 rand) or -3e4."""
    if mname == "1e6":
        return 1e6 * (1.0 + 0.1 * torch.rand(C, generator=torch.Generator().manual_seed(41)))
    return torch.full((C,), float(mname))


def _ratios(x, order, pivot):
    """(mean error / dm, variance error / dv, relative variance error), the worst channel's, of the plane statistics of x [C, H, W]
    recombined from the emulated tiles."""
    _, H, W = x.shape
    ent = tb.entry_labels("conv", H, W)
    ts = torch.from_numpy(np.stack([tb.emulate_tile_stats(p.numpy(), order, pivot) for p in x]))
    sx, sxx, cnt = tb.tile_sums(ts)
    assert (cnt == H * W).all() and torch.isfinite(ts).all()
    st = tb.TileStats(x.reshape(C, -1), ent.labels.reshape(1, -1), EPS)
    mean, var = sx / cnt, sxx / cnt - (sx / cnt) ** 2
    return st.mean_ratio(mean), st.var_ratio(var), st.var_rel(var)


def _orders(W):
    return ("vec", "elem") if W % 4 == 0 else ("elem",)


def test_bound_of_exact_statistics_is_met():
    """fp64 statistics meet the bound trivially, and the bound does not depend on where an outlier sits inside an entry."""
    H, W = 16, 64
    ent = tb.entry_labels("conv", H, W)
    a = tb.place("P00", _plane("A", H, W), ent, 1e6)
    b = tb.place("Pmid", _plane("A", H, W), ent, 1e6)
    sa = tb.TileStats(a.reshape(C, -1), ent.labels.reshape(1, -1), EPS)
    sb = tb.TileStats(b.reshape(C, -1), ent.labels.reshape(1, -1), EPS)
    assert sa.mean_ratio(sa.mean) == 0 and sa.var_ratio(sa.var) == 0
    assert ((sa.dv / sb.dv - 1).abs() < 0.1).all() and ((sa.dm / sb.dm - 1).abs() < 0.1).all()


def test_entry_geometry():
    assert tb.conv_geometry(16, 32) == (8, 32, 2) and tb.conv_geometry(16, 16) == (16, 16, 4) and tb.conv_geometry(9, 13)[0] == 16
    e = tb.entry_labels("conv", 20, 36)
    assert e.n == 6 and e.first[5] == (16, 32) and e.wave_first[5] == [(16, 32), (18, 32), None, None]
    e = tb.entry_labels("conv", 16, 16)
    assert e.n == 1 and e.wave_first[0][2] == (8, 0)
    u = tb.entry_labels("up", 16, 64)
    assert u.n == 4 and u.first == [(0, 0), None, (1, 0), None] and u.wave_first[2][1] == (5, 0)
    assert int(u.labels[3, 7]) == 2 and int(u.labels[4, 63]) == 0
    u = tb.entry_labels("up", 32, 32)
    assert u.n == 4 and u.wave_first[0][2] == (16, 0)
    v = tb.entry_labels("volume", 4, 8 * 32)
    assert v.n == 4 and int(v.labels[2, 255]) == 2
    v = tb.entry_labels("volume", 2, 2048 + 300)
    assert v.n == 6 and int(v.labels[1, 1024]) == 4 and int(v.labels[1, 3 * 256]) == 3 and int(v.labels[1, 2048]) == 5


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("fam", ["A", "B1e3", "B1e4", "C", "E40", "F"])
def test_plain_families_are_admitted(plane, fam):
    H, W = plane
    x = _plane(fam, H, W)
    for order in _orders(W):
        for pivot in ("first", "med3", "mean"):
            m, v, rel = _ratios(x, order, pivot)
            print(f"{fam} {H}x{W} {order} {pivot}: mean error / bound = {m:.3f}, variance error / bound = {v:.3f}")
            if pivot != "first" or fam in ("A", "B1e3"):
                assert max(m, v) <= 0.5, (fam, plane, order, pivot, m, v)


@pytest.mark.parametrize("mname", MS)
@pytest.mark.parametrize("fam", tb.P_FAMILIES)
def test_pivot_outliers_discriminate(fam, mname):
    """The robust orders are admitted at 0.5 at most in every case.  The first-pixel order is rejected in EVERY case (ratio > 1) and by
    at least 5x on every family and magnitude (the worst plane's ratio): single cases land between 1.4 and 5 where the outlier is the
    pivot of one late wave only (Pw2) or of a ragged tile of 16 or 64 pixels (Plast) -- DESIGN 4.28 lists them."""
    family_worst = 0.0
    for H, W in PLANES:
        ent = tb.entry_labels("conv", H, W)
        assert ent.wave_first[0][2] is not None
        for base in ("A", "B1e3"):
            x = tb.place(fam, _plane(base, H, W), ent, _magnitude(mname))
            for order in _orders(W):
                worst = {}
                for pivot in ("first", "med3", "mean"):
                    m, v, rel = _ratios(x, order, pivot)
                    worst[pivot] = max(m, v)
                    print(f"{fam} M={mname} on {base} {H}x{W} {order} {pivot}: mean error / bound = {m:.3f}, variance error / bound = {v:.3f}")
                assert worst["first"] > 1.0, (fam, mname, base, (H, W), order, worst)
                assert worst["med3"] <= 0.5 and worst["mean"] <= 0.5, (fam, mname, base, (H, W), order, worst)
                family_worst = max(family_worst, worst["first"])
    print(f"{fam} M={mname}: the first-pixel order's worst ratio {family_worst:.1f}")
    assert family_worst >= 5.0, (fam, mname, family_worst)


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("fam", tb.CONTROLS)
def test_controls_are_admitted(plane, fam):
    """The same outliers one pixel off a pivot: every order is admitted."""
    H, W = plane
    ent = tb.entry_labels("conv", H, W)
    for mname in MS:
        x = tb.place(fam, _plane("A", H, W), ent, _magnitude(mname))
        for order in _orders(W):
            for pivot in ("first", "med3", "mean"):
                m, v, rel = _ratios(x, order, pivot)
                print(f"{fam} M={mname} {H}x{W} {order} {pivot}: mean error / bound = {m:.3f}, variance error / bound = {v:.3f}")
                assert max(m, v) <= 0.5, (fam, mname, plane, order, pivot, m, v)


@pytest.mark.parametrize("plane", PLANES)
def test_border_column_and_padding_signature(plane):
    """Ecol and Eboth put every wave's first pixel into the border: the robust orders are admitted."""
    H, W = plane
    ent = tb.entry_labels("conv", H, W)
    for fam, base in (("Ecol", "A"), ("Ecol", "B1e3"), ("Eboth", "B1e3")):
        x = tb.place(fam, _plane(base, H, W), ent, 0.0)
        for order in _orders(W):
            for pivot in ("first", "med3", "mean"):
                m, v, rel = _ratios(x, order, pivot)
                print(f"{fam} on {base} {H}x{W} {order} {pivot}: mean error / bound = {m:.3f}, variance error / bound = {v:.3f}")
                if pivot != "first":
                    assert max(m, v) <= 0.5, (fam, base, plane, order, pivot, m, v)


@pytest.mark.parametrize("plane", PLANES)
def test_border_row_is_reported(plane):
    """Erow: half of wave 0 sits at another level, no pivot centres both halves.  Reported against the new bound, asserted against
    the project's 1e-5 relative variance tolerance only."""
    H, W = plane
    ent = tb.entry_labels("conv", H, W)
    for base in ("A", "B1e3"):
        x = tb.place("Erow", _plane(base, H, W), ent, 0.0)
        for order in _orders(W):
            for pivot in ("first", "med3", "mean"):
                m, v, rel = _ratios(x, order, pivot)
                print(f"Erow on {base} {H}x{W} {order} {pivot}: mean error / bound = {m:.3f}, variance error / bound = {v:.3f}, "
                      f"relative variance error {rel:.2e}")
                assert rel <= 1e-5, (base, plane, order, pivot, rel)
