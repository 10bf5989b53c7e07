"""Chunked volume decode on a real MI355X: the box copy of ds_window.hip against a torch restatement of its formula (a copy:
torch.equal, and nothing outside the box touched), at offsets past 2^31, and diffsci_amd.extra.chunk_decode_strategy_b_3d
against what the reference's chunked decode produced for the same tilings (tests/golden/chunk_decode_*.npz).

Bounds.  The decode: the referee rule of tests/test_gpu_vaenet.py -- rel-L2 < 1e-5 against the reference's fp32 output and,
against its fp64 output, within max(4 x the reference's own fp32-vs-fp64 distance, 2e-6).  A single-tile plan runs the launches
of decoder(z) on a copy of z: torch.equal.  A tiled plan is a different function from decoder(z) (GroupNorm statistics are
tile-local): the tiled, zero-padded plan of case a must differ from decoder(z) by rel-L2 > 1e-3 (the reference differs from its
own full decode by 7.6e-2 there) while meeting the referee rule against its own fixture."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import chunk_decode_cases as cases  # noqa: E402
from tests.golden_util import rel_l2  # noqa: E402

REL = 1e-5
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def referee(got, want32, want64, what=""):
    e32, e64, ref = rel_l2(got, want32), rel_l2(got, want64), rel_l2(want32, want64)
    print(f"{what}: vs fp32 {e32:.2e}; vs fp64 {e64:.2e}; reference fp32 vs fp64 {ref:.2e}")
    assert e32 < REL, (what, e32)
    assert e64 < max(4 * ref, 2e-6), (what, e64, ref)


def restated(src, start, size):
    """src[..., (s0 + i) mod S0, (s1 + j) mod S1, (s2 + k) mod S2] by index tensors (torch's % of an integer tensor by a positive
    int is the Euclidean one)."""
    idx = [(s + torch.arange(n, device=src.device)) % S for s, n, S in zip(start, size, src.shape[-3:])]
    return src[..., idx[0], :, :][..., idx[1], :][..., idx[2]]


# source sides, source start, box, destination sides, destination start
BOXES = [
    ((3, 5, 7), (-4, -11, -3), (10, 23, 9), (10, 23, 9), (0, 0, 0)),      # several periods on every axis, a ragged inner length
    ((4, 8, 64), (0, 0, 0), (4, 8, 64), (4, 8, 64), (0, 0, 0)),           # the aligned 16-byte path
    ((4, 8, 64), (1, -2, -6), (4, 8, 64), (4, 8, 64), (0, 0, 0)),         # a wrap inside the inner axis, at an offset not % 4
    ((5, 6, 10), (2, 1, 3), (2, 3, 5), (7, 9, 13), (5, 6, 8)),            # a scatter to the far corner
    ((2, 2, 1), (0, 0, -1), (2, 2, 3), (2, 2, 3), (0, 0, 0)),             # an inner axis of size 1
]


@pytest.mark.parametrize("case", range(len(BOXES)))
def test_box_copy_equals_the_formula(dev, case):
    from diffsci_amd import ops
    S, start, size, D, at = BOXES[case]
    torch.manual_seed(700 + case)
    src = torch.randn(2, 3, *S, device=dev)                               # 6 planes
    dst = torch.full((2, 3) + D, SENTINEL, device=dev)
    want = dst.clone()
    want[..., at[0]:at[0] + size[0], at[1]:at[1] + size[1], at[2]:at[2] + size[2]] = restated(src, start, size)
    assert ops.box_copy3d(src, start, dst, at, size) is dst
    assert torch.equal(dst, want)
    assert int((dst == SENTINEL).sum()) == dst.numel() - 6 * size[0] * size[1] * size[2]


def test_box_copy_empty_box_and_flat_planes(dev):
    from diffsci_amd import ops
    src = torch.randn(6, 3, 5, 7, device=dev)                             # the planes as one axis
    dst = torch.full((6, 4, 4, 4), SENTINEL, device=dev)
    ops.box_copy3d(src, (1, 1, 1), dst, (4, 0, 0), (0, 4, 4))
    assert bool((dst == SENTINEL).all())
    ops.box_copy3d(src, (-1, 4, 6), dst, (1, 0, 1), (3, 4, 2))
    assert torch.equal(dst[:, 1:4, :, 1:3], restated(src, (-1, 4, 6), (3, 4, 2)))


def test_box_copy_offsets_past_2_31(dev):
    """8.6 GB, nothing filled: a tile into the last corner of plane 1 (element offsets up to 2.15e9 > 2^31), read back through
    windows that wrap around that corner.  tools/box_index_check.cpp covers the same geometry on the host."""
    from diffsci_amd import ops
    big = torch.empty(1, 2, 1024, 1024, 1025, device=dev)
    assert big.numel() > 1 << 31
    torch.manual_seed(710)
    tile = torch.randn(1, 2, 2, 3, 5, device=dev)
    corner = (1022, 1021, 1020)
    ops.box_copy3d(tile, (0, 0, 0), big, corner, (2, 3, 5))
    assert torch.equal(big[..., 1022:, 1021:, 1020:], tile)
    window = torch.full((1, 2, 4, 6, 10), SENTINEL, device=dev)
    ops.box_copy3d(big, corner, window, (0, 0, 0), (4, 6, 10))            # runs past the corner, on to index 0 of every axis
    assert torch.equal(window[..., :2, :3, :5], tile)
    back = torch.full((1, 2, 2, 3, 5), SENTINEL, device=dev)
    ops.box_copy3d(big, (-2, -3, -5), back, (0, 0, 0), (2, 3, 5))         # the same corner from a negative start
    assert torch.equal(back, tile)


def test_box_copy_refusals(dev):
    from diffsci_amd import ops
    src, dst = torch.zeros(6, 5, 6, 10, device=dev), torch.full((6, 7, 9, 13), SENTINEL, device=dev)
    with pytest.raises(ValueError, match="leaves dst"):
        ops.box_copy3d(src, (0, 0, 0), dst, (5, 6, 8), (2, 3, 6))
    with pytest.raises(ValueError, match="share storage"):
        ops.box_copy3d(dst[:3], (0, 0, 0), dst[3:], (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="planes"):
        ops.box_copy3d(src[:5], (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="fp32"):
        ops.box_copy3d(src.half(), (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    assert bool((dst == SENTINEL).all())


@pytest.fixture(scope="module")
def decoder(dev):
    from diffsci_amd.models.nets.vaenet import VAEDecoder
    cache = {}

    def get(tag):
        if tag not in cache:
            dec = VAEDecoder(cases.config(tag))
            dec.load_state_dict(cases.load(tag)[1], strict=True)
            cache[tag] = dec.eval().to(dev)
        return cache[tag]
    return get


def chunked(decoder, tag, i, z=None, **kw):
    from diffsci_amd.extra import chunk_decode_strategy_b_3d
    vals, _, info = cases.load(tag)
    chunk, cap, periodic = info["tilings"][i]
    return chunk_decode_strategy_b_3d(decoder(tag), vals["z"] if z is None else z, chunk, max_stage_out_chunk=cap,
                                      periodicity=periodic, **kw)


@pytest.mark.parametrize("tag,i", cases.CASES)
def test_chunked_decode_against_the_reference(decoder, tag, i):
    vals = cases.load(tag)[0]
    got = chunked(decoder, tag, i)
    assert got.device.type == "cpu" and got.shape == vals[f"t{i}/out_f32"].shape and bool(torch.isfinite(got).all())
    referee(got, vals[f"t{i}/out_f32"], vals[f"t{i}/out_f64"], f"chunk_decode {tag} tiling {i}")


@pytest.mark.parametrize("tag", cases.TAGS)
def test_single_tile_equals_the_full_decode(dev, decoder, tag):
    vals = cases.load(tag)[0]
    full = decoder(tag)(vals["z"].to(dev))
    got = chunked(decoder, tag, 0, output_device=dev)
    assert got.device == full.device and torch.equal(got, full)
    referee(full.cpu(), vals["full_f32"], vals["t0/out_f64"], f"decoder(z) {tag}")


def test_tilings_are_told_apart(dev, decoder):
    vals = cases.load("a")[0]
    full = decoder("a")(vals["z"].to(dev)).cpu()
    got = chunked(decoder, "a", 1)
    d, ref = rel_l2(got, full), rel_l2(vals["t1/out_f32"], vals["full_f32"])
    print(f"tiled vs full decode: {d:.2e} (the reference: {ref:.2e})")
    assert d > 1e-3
    referee(got, vals["t1/out_f32"], vals["t1/out_f64"], "chunk_decode a tiling 1")


def test_input_and_output_placement(dev, decoder):
    vals = cases.load("b")[0]
    dec = decoder("b")
    on_cpu = chunked(decoder, "b", 1)
    assert on_cpu.device.type == "cpu" and not dec.training
    kept = chunked(decoder, "b", 1, output_device="cuda:0")
    assert kept.device == dev and torch.equal(kept.cpu(), on_cpu)
    from_dev = chunked(decoder, "b", 1, z=vals["z"].to(dev), device="cuda:0")
    assert from_dev.device.type == "cpu" and torch.equal(from_dev, on_cpu)
    dec.train()
    try:
        assert torch.equal(chunked(decoder, "b", 1), on_cpu) and dec.training
    finally:
        dec.eval()


def test_conv_precision_fp32(decoder):
    vals = cases.load("a")[0]
    dec = decoder("a")
    dec.conv_precision = "fp32"
    try:
        got = chunked(decoder, "a", 3)
    finally:
        dec.conv_precision = "fp16x3"
    referee(got, vals["t3/out_f32"], vals["t3/out_f64"], "chunk_decode a tiling 3 fp32")
