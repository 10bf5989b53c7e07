"""ops.py is the only place where tensors become raw pointers, so (1) for valid calls it must launch exactly what its parent
launched -- tests/golden/abi_trace.json, recorded from the parent commit's ops.py by tools/make_abi_trace_golden.py -- and
(2) a buffer a kernel would overrun or misread must be refused before anything is launched.  Host only, by construction: the
library is replaced by a recorder (tests/abi_trace.py), because on a GPU a missing check of (2) would be an out-of-bounds write.
Each gap test fails at the parent commit, whose wrappers reach their launch with these arguments."""
import json
import os

import pytest
import torch

from diffsci_amd import ops

from . import abi_trace

GOLD = os.path.join(os.path.dirname(__file__), "golden", "abi_trace.json")


@pytest.fixture
def on_host(monkeypatch):
    """Host tensors pass for device tensors: the one device predicate of ops.py says so."""
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    return monkeypatch.setattr


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)["cases"]


def test_case_table_reaches_every_launch_entry_point(gold):
    assert set(gold) == set(abi_trace.CASES)
    reached = {c[0] for t in gold.values() for c in t["calls"]}
    assert reached == set(abi_trace.LAUNCHES)


@pytest.mark.parametrize("case", sorted(abi_trace.CASES))
def test_launches_equal_the_parents(case, gold, on_host):
    got = json.loads(json.dumps(abi_trace.trace_of(ops, on_host, abi_trace.CASES[case])))
    want = gold[case]
    assert got["pools"] == want["pools"]                     # as many pool buffers taken, none kept
    assert all(kept == 0 for _, kept in got["pools"])
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"launch {i} of {case!r} differs from the parent's"
    assert len(got["calls"]) == len(want["calls"])


def _gaps(c):
    """(id, call) for every buffer that used to reach a launch unchecked; B = 2, C = 8, 8x8."""
    o = c.ops
    B, C = 2, 8
    x, stats, w, b = c.f("x", B, C, 8, 8), c.f("stats", B, 2), c.f("w", C), c.f("b", C)
    wide = c.f("wide", B, 4 * C)
    film = wide[:, :2 * C]                                   # a strided view of a wider table: rows 4C apart, not 2C
    ta = c.f("ta", B, C, o.conv_tile_count(8, 8), 4)
    small = c.f("small", 3)
    h, t, W = c.f("h", B, 16), c.f("t", B), c.f("W", 8)
    return [
        ("gnorm1_apply-out", lambda: o.gnorm1_apply(x, stats, w, b, 0, out=c.f("o1", B, C, 4, 4))),
        ("gnorm1_apply-stats", lambda: o.gnorm1_apply(x, c.f("s1", 1, 2), w, b, 0)),
        ("gnorm1_apply-w", lambda: o.gnorm1_apply(x, stats, small, b, 0)),
        ("gnorm1_apply-b", lambda: o.gnorm1_apply(x, stats, w, small, 0)),
        ("gnorm1_apply-film", lambda: o.gnorm1_apply(x, stats, w, b, 0, film=film)),
        ("gnorm1_apply_poolf-film", lambda: o.gnorm1_apply_poolf(x, stats, w, b, 0, 2, film=film)),
        ("gnorm1_table-film", lambda: o.gnorm1_table(ta, w, b, 0, 64, film=film)),
        ("gnorm1_apply_images-film", lambda: o.gnorm1_apply_images(x, stats, w, b, 0, film=film)),
        ("gnorm1_stats-stats", lambda: o.gnorm1_stats(x, 0, stats=c.f("s2", 1, 2))),
        ("inorm_table-w", lambda: o.inorm_table(ta, small, b, 0, 64)),
        ("inorm_table-b", lambda: o.inorm_table(ta, w, small, 0, 64)),
        ("concat2-out", lambda: o.concat2(x, x, out=c.f("o2", B, C, 8, 8))),
        ("concat2-batch", lambda: o.concat2(x, c.f("x1", 1, C, 8, 8))),
        ("concat2-spatial", lambda: o.concat2(x, c.f("x4", B, C, 4, 4))),
        ("linear-out", lambda: o.linear(h, c.f("lw", 24, 16), out=c.f("o3", B, 16))),
        ("linear-b", lambda: o.linear(h, c.f("lw2", 24, 16), small)),
        ("fourier_features-out", lambda: o.fourier_features(t, W, out=c.f("o4", B, 8))),
        ("fourier_features-add", lambda: o.fourier_features(t, W, add=c.f("ye", B, 8))),
        ("fourier_channels-out", lambda: o.fourier_channels(x, c.f("Wc", C, 4), out=c.f("o5", B, 4, 8, 8))),
        ("conv_direct-bias", lambda: o.conv_direct(x, c.f("wd", 2, C, 3, 3), small)),
        ("div_scalar-out", lambda: o.div_scalar(x, 2.0, out=c.f("o6", B, C, 4, 4))),
        ("mask_blend-out", lambda: o.mask_blend(x, x, c.f("mask", C, 8, 8), out=c.f("o7", B, C, 4, 4))),
        ("lerp_stack-x2", lambda: o.lerp_stack(x, c.f("x2", B, C, 4, 4), 3)),
        ("add_act-out", lambda: o.add_act(h, out=c.f("o8", B, 8))),
    ]


GAP_IDS = ["gnorm1_apply-out", "gnorm1_apply-stats", "gnorm1_apply-w", "gnorm1_apply-b", "gnorm1_apply-film",
           "gnorm1_apply_poolf-film", "gnorm1_table-film", "gnorm1_apply_images-film", "gnorm1_stats-stats", "inorm_table-w",
           "inorm_table-b", "concat2-out", "concat2-batch", "concat2-spatial", "linear-out", "linear-b", "fourier_features-out",
           "fourier_features-add", "fourier_channels-out", "conv_direct-bias", "div_scalar-out", "mask_blend-out", "lerp_stack-x2",
           "add_act-out"]


@pytest.mark.parametrize("gap", GAP_IDS)
def test_unchecked_extent_is_refused_before_any_launch(gap, on_host):
    def run(c):
        calls = dict(_gaps(c))
        assert list(calls) == GAP_IDS
        with pytest.raises(ValueError):
            calls[gap]()
    rec, _ = abi_trace.traced(ops, on_host, run)
    assert rec.calls == []


def test_strided_film_is_what_the_gap_tests_think_it_is():
    wide = torch.zeros(2, 32)
    assert not wide[:, :16].is_contiguous() and wide[:, :16].shape == (2, 16)
