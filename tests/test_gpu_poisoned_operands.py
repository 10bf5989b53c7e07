"""Every kernel on hostile memory (tests/guarded.py): each operand a view between poisoned guard bands of at least its own size,
outputs and scratch poison-filled, amax slots seeded; the oracle is the same call on clean operands (zero-backed allocations of
their own), and every output, statistic, slot and pooled tensor must agree bit for bit, for both poisons.  What this sees and
the rest of the suite cannot: a read of something no launch wrote (the pad rows of a norm table, the last chunk of a ragged Cin,
the border of an image, a depth-pad slice, a stale statistic), which fresh device memory hides by being zero, and a store a few
elements outside an output, which the allocator's slack hides.

Shapes are the smallest at which the indexing can still go wrong: B = 2, Cin = 24 (a chunk and a half; 40: an odd number of
chunks), Cout = 40 (a ragged 64-channel tile), planes 9 x 13 (16 x 16 pixel tiles: pad16 = 256 < pad32 = 512) and 20 x 36 (8 x 32
tiles, 3 x 2 of them: pad32 = pad16 = 1536), and the first shape past one tile where a kernel loops.  The comment at each case
names the instantiation it reaches (diffsci_amd/csrc/ds_conv3h.hip launch_conv3h_c and friends)."""
import math

import pytest
import torch

from tests import guarded as G
from tests.test_guarded import FAULTS, _case as emulated_fault

pytestmark = pytest.mark.gpu
B = 2
POISON = list(G.POISONS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


@pytest.fixture(scope="module")
def N():
    from diffsci_amd import _native
    return _native


def rnd(seed, *shape, scale=1.0, shift=0.0):
    """Seeded host data; sample 0 is 2^-7 of the others (the per-sample exponents differ)."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift
    if x.dim() >= 3:
        x[0] *= 2.0 ** -7
    return x


def conv_w(seed, Cout, Cin, *k):
    fan = Cin * math.prod(k)
    return torch.randn(Cout, Cin, *k, generator=torch.Generator().manual_seed(seed)) / math.sqrt(fan)


def guard_pack(o, pw):
    """The packed streams of an ops.PackedConv (or a list of them) moved between guard bands: weights are inputs like any other."""
    if isinstance(pw, (list, tuple)):
        return [guard_pack(o, p) for p in pw]
    if pw.data is not None:
        pw.data = o.inp(pw.data)
    if pw.up is not None:
        pw.up = o.inp(pw.up)
    for _, _, sub in pw.subs or ():
        guard_pack(o, sub)
    return pw


class Pool:
    """take / give of runtime.Workspace over hostile scratch: every buffer a composed op takes is poisoned and banded."""

    def __init__(self, o):
        self.o, self.out = o, 0

    def take(self, shape, device):
        self.out += 1
        return self.o.scratch(*shape)

    def give(self, t):
        self.out -= 1


def run(case, dev, poison):
    G.assert_clean(case, dev, G.POISONS[poison])


# ========================================================================================= the harness itself, on device memory
@pytest.mark.parametrize("fault,poison", [(None, p) for p in POISON] + [(f, p) for f, ps in FAULTS.items() for p in ps])
def test_harness_on_the_device(dev, fault, poison):
    """tests/test_guarded.py's emulated faults, committed with torch on device tensors: rejected here as on the CPU."""
    assert bool(G.check(emulated_fault(fault), dev, G.POISONS[poison])) == (fault is not None)


# =============================================================================================== fp16x3 3x3: ops.conv (ds_conv2d_h3)
def conv3_case(ops, N, *, Cin=24, Cout=40, plane=(9, 13), load="plain", source="raw", shift=None, res=(), res1_up=False,
               circular=False, ks=3, upsampled=False, bias=True, stats=True, B=B):
    """plane: the INPUT plane.  source: "raw" (in_amax from absmax_rows into guarded slots), "inorm" / "gnorm1" (a prenorm table
    from the tile statistics a ragged producer convolution left).  -> the case function."""
    Hi, Wi = plane
    mode = {"plain": N.DS_LOAD_PLAIN, "maxpool": N.DS_LOAD_MAXPOOL2, "up": N.DS_LOAD_UPSAMPLE2}[load]
    H, W = {"plain": (Hi, Wi), "maxpool": (Hi // 2, Wi // 2), "up": (2 * Hi, 2 * Wi)}[load]

    def case(o):
        d = o.device
        kw = {}
        if source == "raw":
            x = o.inp(rnd(1, B, Cin, Hi, Wi, scale=3.0))
            kw["in_amax"] = ops.absmax_rows(x, out=o.zeroed(B))
        else:
            # the producer: a ragged fp16x3 3x3 convolution that leaves the tile statistics of what it stored
            xp = o.inp(rnd(2, B, 24, Hi, Wi))
            pp = guard_pack(o, ops.pack_conv(conv_w(3, Cin, 24, 3, 3).to(d), "fp16x3"))
            ts = o.out(B, Cin, ops.conv_tile_count(Hi, Wi), 4)
            x = ops.conv(xp, pp, bias=o.inp(rnd(4, Cin)), tile_stats=ts, in_amax=ops.absmax_rows(xp, out=o.zeroed(B)),
                         out=o.out(B, Cin, Hi, Wi))
            wn, bn = o.inp(1 + 0.25 * rnd(5, Cin)), o.inp(0.25 * rnd(6, Cin))
            tab = o.out(B, ops.table_channels(Cin), 4)
            if source == "inorm":
                ops.inorm_table(ts, wn, bn, 0, Hi * Wi, out=tab)
            else:
                ops.gnorm1_table(ts, wn, bn, 1, Hi * Wi, film=o.inp(0.25 * rnd(7, B, 2 * Cin)), out=tab)
            kw["prenorm"] = tab
        pw = guard_pack(o, ops.pack_conv(conv_w(8, Cout, Cin, ks, ks).to(d), "fp16x3", upsampled=upsampled))
        if bias:
            kw["bias"] = o.inp(rnd(9, Cout))
        if shift is not None:
            kw["shift"] = o.inp(rnd(10, B if shift == "per_sample" else 1, Cout))
        if res:
            kw["res1"] = o.inp(rnd(11, B, Cout, *((H // 2, W // 2) if res1_up else (H, W))))
            if res1_up:
                kw["res1_upsampled"] = True
        if len(res) > 1:
            kw["res2"] = o.inp(rnd(12, B, Cout, H, W))
        if stats:
            kw["tile_stats"] = o.out(B, Cout, ops.conv_tile_count(H, W), 4)
        ops.conv(x, pw, load_mode=mode, circular=circular, out=o.out(B, Cout, H, W), out_amax=o.slots(B), **kw)
    return case


CONV3 = {
    # k_conv3h<PLAIN, W16, PRE=false, CIRC=false, NW=4, S16> (two chunks: the 16x16x32 kernel)
    "plain_9x13": dict(shift="per_sample", res=(1, 2)),
    # k_conv3h<PLAIN, !W16, ..., S16>: 3 x 2 tiles of 8 x 32, the last of each ragged
    "plain_20x36": dict(plane=(20, 36), shift="broadcast", res=(1,)),
    # Cin = 40: three chunks, k_conv3h<PLAIN, W16 / !W16, false, false, 4> (the 32x32x16 kernel)
    "plain_9x13_cin40": dict(Cin=40),
    "plain_20x36_cin40": dict(Cin=40, plane=(20, 36), res=(1, 2)),
    # VEC: W % 32 == 0, Cin % 16 == 0, no tap offset: the 16-byte patch loads; H = 9: a ragged second tile row
    "plain_vec_9x64": dict(Cin=32, plane=(9, 64)),
    # two channel tiles (Cout = 72) on either geometry
    "plain_cout72": dict(Cout=72, plane=(20, 36), shift="per_sample"),
    # DS_LOAD_MAXPOOL2: k_conv3h<MAXPOOL2, W16 / !W16, false, false, 4(, S16)>
    "maxpool_18x26": dict(load="maxpool", plane=(18, 26), res=(1,)),
    "maxpool_40x72": dict(load="maxpool", plane=(40, 72)),
    "maxpool_40x72_cin40": dict(load="maxpool", plane=(40, 72), Cin=40),
    # DS_LOAD_UPSAMPLE2 through the loader (no parity packing): 5 x 7 -> 10 x 14 (W16), 10 x 18 -> 20 x 36
    "up_5x7": dict(load="up", plane=(5, 7), res=(1,)),
    "up_10x18": dict(load="up", plane=(10, 18), shift="per_sample"),
    "up_10x18_cin40": dict(load="up", plane=(10, 18), Cin=40),
    # the fused norm + SiLU loader: PRE = true.  The table's rows 24 .. 31 and the input's channels 24 .. 31 are nobody's
    "inorm_9x13": dict(source="inorm", res=(1,)),
    "inorm_20x36": dict(source="inorm", plane=(20, 36), shift="per_sample"),
    "inorm_20x36_cin40": dict(source="inorm", plane=(20, 36), Cin=40),             # PRE on the 32x32x16 kernel: eight waves
    "gnorm1_9x13": dict(source="gnorm1"),
    "gnorm1_20x36": dict(source="gnorm1", plane=(20, 36), res=(1, 2)),
    "gnorm1_up_10x18": dict(source="gnorm1", load="up", plane=(10, 18)),
    # res1 at half resolution (DS_RES1_UPSAMPLED)
    # two channel tiles per workgroup (TWO: the fused loader at exactly two channel tiles and at least 256 workgroups after halving;
    # H % 8 != 0 or W % 32 != 0 keeps the launch off the persistent kernel): 12 x 32 with the 16-byte patch loads (VEC), 8 x 48 without
    "two_tiles_vec_12x32": dict(source="inorm", Cin=128, Cout=128, plane=(12, 32), B=128, res=(1,)),
    "two_tiles_8x48": dict(source="gnorm1", Cin=128, Cout=128, plane=(8, 48), B=128, shift="per_sample"),
    "res1_upsampled_20x36": dict(plane=(20, 36), res=(1,), res1_up=True),
    "res1_upsampled_inorm_10x14": dict(source="inorm", plane=(10, 14), res=(1,), res1_up=True),
    # periodic padding: CIRC = true; one axis and both
    "circular_h_9x13": dict(circular=(True, False)),
    "circular_w_20x36": dict(circular=(False, True), plane=(20, 36)),
    "circular_both_9x13": dict(circular=True, res=(1,)),
    "circular_both_20x36": dict(circular=True, plane=(20, 36), source="inorm"),
    # a 5 x 5 kernel: four shifted 3 x 3 blocks with non-zero DS_TAP_OFFSET, accumulated in place
    "k5_9x13": dict(ks=5, shift="per_sample", res=(1,)),
    "k5_20x36": dict(ks=5, plane=(20, 36)),
    "k5_circular_20x36": dict(ks=5, plane=(20, 36), circular=True),
    # the parity kernel (upsampled=True packing): 8 x 32 (geometry 1) and 16 x 16 (geometry 2) low-resolution inputs take
    # ds_conv2d_h3_up; 9 x 13 is not whole tiles and falls back to the upsampling loader
    "parity_8x32": dict(load="up", plane=(8, 32), upsampled=True, shift="per_sample", res=(1, 2)),
    "parity_16x16": dict(load="up", plane=(16, 16), upsampled=True, res=(1,)),
    "parity_16x16_cin40": dict(load="up", plane=(16, 16), upsampled=True, Cin=40),
    "parity_inorm_16x16": dict(load="up", plane=(16, 16), upsampled=True, source="inorm"),
    "parity_unsupported_9x13": dict(load="up", plane=(9, 13), upsampled=True, res=(1,)),
    "parity_circular_8x32": dict(load="up", plane=(8, 32), upsampled=True, circular=True),
}


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("name", list(CONV3))
def test_conv3x3_fp16x3(ops, N, dev, name, poison):
    run(conv3_case(ops, N, **CONV3[name]), dev, poison)


# ==================================================================== the persistent kernel (ds_conv3p.hip), pc_raw and pool=PoolOut
# conv3p_try_launch: H % 8 == 0, W % 32 == 0, Cout % 64 == 0, Cin % 64 == 0 and at least one item per workgroup (256 CUs): 2
# channel tiles x (2 x 2) pixel tiles x 33 samples = 264 items over 256 workgroups: eight workgroups take two items, the rest one
PC = dict(B=33, Cin=64, Cout=128, H=16, W=64)


def pc_case(ops, form):
    Bp, Cin, Cout, H, W = (PC[k] for k in ("B", "Cin", "Cout", "H", "W"))

    def case(o):
        d = o.device
        x = rnd(21, Bp, Cin, H, W, scale=2.0)
        for b in range(Bp):
            x[b] *= 2.0 ** (b % 5 - 2)
        pw = guard_pack(o, ops.pack_conv(conv_w(22, Cout, Cin, 3, 3).to(d), "fp16x3"))
        kw = dict(bias=o.inp(rnd(23, Cout)), tile_stats=o.out(Bp, Cout, ops.conv_tile_count(H, W), 4), out_amax=o.slots(Bp),
                  out=o.out(Bp, Cout, H, W))
        if form == "raw":                                     # launch_conv3p<PRE=false>: pc_raw asks for it
            xd = o.inp(x)
            ops.conv(xd, pw, in_amax=ops.absmax_rows(xd, out=o.zeroed(Bp)), pc_raw=True, shift=o.inp(rnd(24, Bp, Cout)), **kw)
            return
        res1 = o.inp(rnd(25, Bp, Cout, H, W))
        pool = ops.PoolOut(o.out(Bp, Cout, H // 2, W // 2))
        if form == "pool":                                    # launch_conv3p_r<PRE, !CIRC, 1, POOL>: fused loader, pooled output
            xd = o.inp(x)
            v = x.double()
            tab = torch.zeros(Bp, ops.table_channels(Cin), 4)
            tab[:, :Cin, 0] = v.mean(dim=(2, 3)).float()
            tab[:, :Cin, 1] = (1 / torch.sqrt(v.var(dim=(2, 3), unbiased=False) + 1e-5)).float()
            tab[:, :Cin, 2] = 0.1
            ops.conv(xd, pw, prenorm=o.inp(tab), res1=res1, pool=pool, **kw)
        else:                                                 # conv3p_try_launch_img: image input, pooled output
            xd = o.inp(x)
            images = o.scratch(ops.conv_images_floats(Bp, Cin, H, W))
            ops.inorm_silu_images(xd, o.inp(1 + 0.25 * rnd(26, Cin)), o.inp(0.25 * rnd(27, Cin)), 0, out=images)
            ops.conv_img(images, pw, Bp, Cin, H, W, bias=kw["bias"], res1=res1, tile_stats=kw["tile_stats"], out=kw["out"],
                         out_amax=kw["out_amax"], pool=pool)
        assert pool.written, "the default selection no longer routes this launch to the persistent kernel: choose another shape"
    return case


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("form", ["raw", "pool", "img_pool"])
def test_persistent_conv3x3(ops, dev, form, poison):
    run(pc_case(ops, form), dev, poison)


# ==================================================================================================== fp16x3 1x1 (ds_conv1x1_h3)
def conv1_case(ops, N, *, Cin=24, Cout=40, plane=(9, 13), load="plain", split=0, res=()):
    Hi, Wi = plane
    mode = {"plain": N.DS_LOAD_PLAIN, "avgpool": N.DS_LOAD_AVGPOOL2, "up": N.DS_LOAD_UPSAMPLE2}[load]
    H, W = {"plain": (Hi, Wi), "avgpool": (Hi // 2, Wi // 2), "up": (2 * Hi, 2 * Wi)}[load]

    def case(o):
        x = o.inp(rnd(31, B, Cin, Hi, Wi, scale=3.0))
        pw = guard_pack(o, ops.pack_conv(conv_w(32, Cout, Cin, 1, 1).to(o.device), "fp16x3"))
        kw = dict(res1=o.inp(rnd(33, B, Cout, H, W))) if res else {}
        if len(res) > 1:
            kw["res2"] = o.inp(rnd(34, B, Cout, H, W))
        ops.conv(x, pw, bias=o.inp(rnd(35, Cout)), shift=o.inp(rnd(36, B, Cout)), load_mode=mode,
                 in_amax=ops.absmax_rows(x, out=o.zeroed(B)), tile_stats=o.out(B, Cout, ops.conv_tile_count(H, W), 4),
                 out_amax=o.slots(2, B) if split else o.slots(B), amax_split=split, out=o.out(B, Cout, H, W), **kw)
    return case


CONV1 = {
    "plain_9x13": dict(res=(1, 2)),
    "plain_20x36": dict(plane=(20, 36)),
    "plain_20x36_cin40": dict(plane=(20, 36), Cin=40, res=(1,)),
    "up_5x7": dict(load="up", plane=(5, 7)),
    "up_10x18": dict(load="up", plane=(10, 18), res=(1,)),
    "avgpool_18x26": dict(load="avgpool", plane=(18, 26)),
    "avgpool_40x72": dict(load="avgpool", plane=(40, 72), res=(1,)),
    # the attention in-projection: channels >= 64 report to the second row of a [2, B] slot tensor (Cout = 96: q, k | v at E = 32)
    "amax_split_9x13": dict(Cout=96, split=64),
    "amax_split_20x36": dict(Cout=96, split=64, plane=(20, 36), Cin=40),
}


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("name", list(CONV1))
def test_conv1x1_fp16x3(ops, N, dev, name, poison):
    run(conv1_case(ops, N, **CONV1[name]), dev, poison)


# ============================================================================ bf16x6, exact-fp32 MFMA (3x3, 1x1) and conv_direct
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("plane", [(9, 13), (20, 36)])
@pytest.mark.parametrize("load", ["plain", "maxpool", "up"])
@pytest.mark.parametrize("kind,ks", [("bf16x6", 3), ("fp32", 3), ("fp32", 1)])
def test_conv_other_precisions(ops, N, dev, kind, ks, load, plane, poison):
    H, W = plane
    Hi, Wi = {"plain": (H, W), "maxpool": (2 * H, 2 * W), "up": ((H + 1) // 2, (W + 1) // 2)}[load]
    if load == "up":
        H, W = 2 * Hi, 2 * Wi
    mode = {"plain": N.DS_LOAD_PLAIN, "maxpool": N.DS_LOAD_MAXPOOL2, "up": N.DS_LOAD_UPSAMPLE2}[load]

    def case(o):
        x = o.inp(rnd(41, B, 24, Hi, Wi))
        pw = guard_pack(o, ops.pack_conv(conv_w(42, 40, 24, ks, ks).to(o.device), kind))
        assert pw.kind == kind
        ops.conv(x, pw, bias=o.inp(rnd(43, 40)), shift=o.inp(rnd(44, B, 40)), res1=o.inp(rnd(45, B, 40, H, W)),
                 res2=o.inp(rnd(46, B, 40, H, W)), load_mode=mode, out=o.out(B, 40, H, W))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("circular", [False, True, (True, False)])
@pytest.mark.parametrize("Cout", [1, 3])
@pytest.mark.parametrize("plane", [(9, 13), (20, 36)])
def test_conv_direct(ops, dev, plane, Cout, circular, poison):
    def case(o):
        x = o.inp(rnd(51, B, 24, *plane))
        ops.conv_direct(x, o.inp(conv_w(52, Cout, 24, 3, 3)), bias=o.inp(rnd(53, Cout)), circular=circular, out=o.out(B, Cout, *plane))
    run(case, dev, poison)


# ======================================================================================= image producers into image consumers
def images_case(ops, producer, consumer, plane, C=24, Cout=40):
    """producer: inorm | gnorm1 | gnorm1_pool | table; consumer: img | up_img.  The image buffer is poison-filled and holds
    exactly conv_images_floats floats: border, channel pad and all."""
    H, W = plane
    Hc, Wc = (H // 2, W // 2) if producer == "gnorm1_pool" else (H, W)

    def case(o):
        d = o.device
        x = o.inp(rnd(61, B, C, H, W, scale=2.0, shift=0.5))
        wn, bn = o.inp(1 + 0.25 * rnd(62, C)), o.inp(0.25 * rnd(63, C))
        images = o.scratch(ops.conv_images_floats(B, C, Hc, Wc))
        if producer == "inorm":
            ops.inorm_silu_images(x, wn, bn, 1, out=images)
        elif producer in ("gnorm1", "gnorm1_pool"):
            st = ops.gnorm1_stats(x, 0, stats=o.out(B, 2), workspace=o.scratch(ops_workspace_floats(B)))
            ops.gnorm1_apply_images(x, st, wn, bn, 0, pool=producer == "gnorm1_pool", film=o.inp(0.25 * rnd(64, B, 2 * C)), out=images)
        else:
            v = rnd(61, B, C, H, W, scale=2.0, shift=0.5).double()
            tab = torch.zeros(B, ops.table_channels(C), 4)
            tab[:, :C, 0], tab[:, :C, 1], tab[:, :C, 2] = v.mean(dim=(2, 3)).float(), (1 / v.std(dim=(2, 3))).float(), 0.05
            ops.table_apply_images(x, o.inp(tab), out=images)
        up = consumer == "up_img"
        pw = guard_pack(o, ops.pack_conv(conv_w(65, Cout, C, 3, 3).to(d), "fp16x3", upsampled=up))
        Ho, Wo = (2 * Hc, 2 * Wc) if up else (Hc, Wc)
        kw = dict(bias=o.inp(rnd(66, Cout)), shift=o.inp(rnd(67, B, Cout)), res1=o.inp(rnd(68, B, Cout, Ho, Wo)),
                  tile_stats=o.out(B, Cout, ops.conv_tile_count(Ho, Wo), 4), out=o.out(B, Cout, Ho, Wo), out_amax=o.slots(B))
        if up:
            ops.conv_up_img(images, pw, B, C, Hc, Wc, **kw)
        else:
            ops.conv_img(images, pw, B, C, Hc, Wc, res2=o.inp(rnd(69, B, Cout, Ho, Wo)), **kw)
    return case


def ops_workspace_floats(rows):
    from diffsci_amd import _native
    return _native.lib().ds_gnorm1_workspace_bytes(rows) // 4


IMAGES = [(p, c, plane) for p in ("inorm", "gnorm1", "gnorm1_pool", "table") for c, plane in
          # conv_img: k_conv3h<PLAIN, W16 / !W16, .., S16, IMGIN> on ragged planes (H W % 4 == 0 for the image norm kernel);
          # conv_up_img: whole 16 x 16 / 8 x 32 low-resolution tiles
          (("img", (10, 14)), ("img", (20, 36)), ("up_img", (16, 16)), ("up_img", (8, 32)))]


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("producer,consumer,plane", IMAGES)
def test_image_producers_into_image_consumers(ops, dev, producer, consumer, plane, poison):
    if producer == "gnorm1_pool":
        plane = (2 * plane[0], 2 * plane[1])
    run(images_case(ops, producer, consumer, plane), dev, poison)


@pytest.mark.parametrize("poison", POISON)
def test_image_consumer_with_upsampled_residual(ops, dev, poison):
    def case(o):
        x = o.inp(rnd(71, B, 32, 20, 36))
        images = ops.inorm_silu_images(x, None, None, 0, out=o.scratch(ops.conv_images_floats(B, 32, 20, 36)))
        pw = guard_pack(o, ops.pack_conv(conv_w(72, 40, 32, 3, 3).to(o.device), "fp16x3"))
        ops.conv_img(images, pw, B, 32, 20, 36, res1=o.inp(rnd(73, B, 40, 10, 18)), res1_upsampled=True, out=o.out(B, 40, 20, 36))
    run(case, dev, poison)


# ============================================================================================================ stride-2 convolutions
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("kind", ["fp16x3", "direct"])
@pytest.mark.parametrize("plane", [(10, 14), (9, 13), (20, 37)])
def test_conv_s2(ops, dev, plane, kind, poison):
    Cin, Cout = (24, 40) if kind == "fp16x3" else (3, 40)
    H, W = plane[0] // 2, plane[1] // 2

    def case(o):
        x = o.inp(rnd(81, B, Cin, *plane, scale=2.0))
        pw = guard_pack(o, ops.pack_conv_s2(conv_w(82, Cout, Cin, 3, 3).to(o.device), "fp16x3"))
        assert pw.kind == kind
        kw = dict(in_amax=ops.absmax_rows(x, out=o.zeroed(B))) if kind == "fp16x3" else {}
        ops.conv_s2(x, pw, bias=o.inp(rnd(83, Cout)), res1=o.inp(rnd(84, B, Cout, H, W)), out_amax=o.slots(B), out=o.out(B, Cout, H, W), **kw)
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("vol", [(4, 10, 14), (5, 9, 13)])
def test_conv3d_s2(ops, dev, vol, pooled, poison):
    """The D + 2 slice-major copy, its per-slice amax rows and the output slices: from torch.empty (ws=None) or a hostile pool."""
    D, H, W = (v // 2 for v in vol)

    def case(o):
        x = o.inp(rnd(85, B, 24, *vol, scale=2.0))
        packs = guard_pack(o, ops.pack_conv3d_s2(conv_w(86, 40, 24, 3, 3, 3).to(o.device), "fp16x3"))
        pool = Pool(o) if pooled else None
        ops.conv3d_s2(x, packs, bias=o.inp(rnd(87, 40)), res1=o.inp(rnd(88, B, 40, D, H, W)), out=o.out(B, 40, D, H, W), ws=pool)
        assert pool is None or pool.out == 0
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
def test_conv3d_s2_direct(ops, dev, poison):
    def case(o):
        x = o.inp(rnd(89, B, 3, 5, 9, 13))
        pk = ops.pack_conv3d_s2(conv_w(90, 40, 3, 3, 3, 3).to(o.device), "fp16x3")
        pk.data = o.inp(pk.data)
        ops.conv3d_s2(x, pk, bias=o.inp(rnd(91, 40)), out=o.out(B, 40, 2, 4, 6))
    run(case, dev, poison)


# ================================================================================================================== volumes
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("load,circular", [(ld, c) for ld in ("plain", "maxpool", "up") for c in (False, True)]
                         + [("plain", (True, False, False)), ("plain", (False, True, True))])      # mixed axes: on the plain load
@pytest.mark.parametrize("D", [3, 5])
def test_conv3d_mfma(ops, N, dev, D, load, circular, poison):
    """Every scratch tensor and slice copy from a hostile pool: the depth-pad slices are zeros or wrapped copies by the copy
    kernel, never what the pool held."""
    H, W = 9, 13
    Di, Hi, Wi = {"plain": (D, H, W), "maxpool": (2 * D, 2 * H, 2 * W), "up": (D, H, W)}[load]
    Do, Ho, Wo = (2 * D, 2 * H, 2 * W) if load == "up" else (D, H, W)
    mode = {"plain": N.DS_LOAD_PLAIN, "maxpool": N.DS_LOAD_MAXPOOL2, "up": N.DS_LOAD_UPSAMPLE2}[load]

    def case(o):
        x = o.inp(rnd(101, B, 24, Di, Hi, Wi, scale=2.0))
        packs = guard_pack(o, ops.pack_conv3d(conv_w(102, 40, 24, 3, 3, 3).to(o.device), upsampled=load == "up"))
        pool = Pool(o)
        stats = o.out(B, 40, ops.volume_stat_tiles(Do, Ho * Wo), 4)
        ops.conv3d_mfma(x, packs, bias=o.inp(rnd(103, 40)), shift=o.inp(rnd(104, B, 40)), res1=o.inp(rnd(105, B, 40, Do, Ho, Wo)),
                        load_mode=mode, circular=circular, out=o.out(B, 40, Do, Ho, Wo), ws=pool, out_stats=stats)
        assert pool.out == 0
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("circular", [False, True])
def test_conv3d_mfma_k5(ops, N, dev, circular, poison):
    def case(o):
        x = o.inp(rnd(106, B, 24, 5, 9, 13))
        packs = guard_pack(o, ops.pack_conv3d(conv_w(107, 40, 24, 5, 5, 5).to(o.device)))
        ops.conv3d_mfma(x, packs, bias=o.inp(rnd(108, 40)), circular=circular, out=o.out(B, 40, 5, 9, 13), ws=Pool(o))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("load", ["plain", "maxpool", "up"])
@pytest.mark.parametrize("D", [3, 5])
def test_conv3d_direct(ops, N, dev, D, load, circular, poison):
    H, W = 9, 13
    Di, Hi, Wi = (2 * D, 2 * H, 2 * W) if load == "maxpool" else (D, H, W)
    Do, Ho, Wo = (2 * D, 2 * H, 2 * W) if load == "up" else (D, H, W)
    mode = {"plain": N.DS_LOAD_PLAIN, "maxpool": N.DS_LOAD_MAXPOOL2, "up": N.DS_LOAD_UPSAMPLE2}[load]

    def case(o):
        x = o.inp(rnd(111, B, 5, Di, Hi, Wi))
        ops.conv3d(x, o.inp(conv_w(112, 7, 5, 3, 3, 3)), bias=o.inp(rnd(113, 7)), shift=o.inp(rnd(114, B, 7)),
                   res1=o.inp(rnd(115, B, 7, Do, Ho, Wo)), res2=o.inp(rnd(116, B, 7, Do, Ho, Wo)), load_mode=mode, circular=circular,
                   out=o.out(B, 7, Do, Ho, Wo))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("circular", [False, True, (True, False, False)])
@pytest.mark.parametrize("D", [3, 5])
def test_resblock3d_fused(ops, dev, D, circular, poison):
    """S1, S2, the tile statistics, the per-slice tables (ds_slice_tables) and the shift rows all come from the hostile pool; h's
    table from the volume_stat_tiles statistics a conv3d_mfma left."""
    C, H, W = 24, 9, 13

    def case(o):
        d = o.device
        pool = Pool(o)
        x0 = o.inp(rnd(121, B, 24, D, H, W, scale=2.0))
        p0 = guard_pack(o, ops.pack_conv3d(conv_w(122, C, 24, 3, 3, 3).to(d)))
        hs = o.out(B, C, ops.volume_stat_tiles(D, H * W), 4)
        h = ops.conv3d_mfma(x0, p0, bias=o.inp(rnd(123, C)), circular=circular, out=o.out(B, C, D, H, W), ws=pool, out_stats=hs)
        tab1 = ops.inorm_table(hs, o.inp(1 + 0.25 * rnd(124, C)), o.inp(0.25 * rnd(125, C)), 0, D * H * W, out=o.out(B, ops.table_channels(C), 4))
        p1 = guard_pack(o, ops.pack_conv3d(conv_w(126, C, C, 3, 3, 3).to(d)))
        p2 = guard_pack(o, ops.pack_conv3d(conv_w(127, C, C, 3, 3, 3).to(d)))
        ops.resblock3d_fused(h, tab1, p1, o.inp(rnd(128, C)), o.inp(rnd(129, B, C)), p2, o.inp(rnd(130, C)),
                             o.inp(1 + 0.25 * rnd(131, C)), o.inp(0.25 * rnd(132, C)), 1, res2=o.inp(rnd(133, B, C, D, H, W)),
                             out=o.out(B, C, D, H, W), out_stats=o.out(B, C, ops.volume_stat_tiles(D, H * W), 4), ws=pool, circular=circular)
        assert pool.out == 0
    run(case, dev, poison)


# ================================================================================================================ attention
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("amax", ["given", "reduced"])
@pytest.mark.parametrize("L", [32, 96])
@pytest.mark.parametrize("heads", [1, 2])
def test_attention_fp16x3_staged(ops, dev, heads, L, amax, poison):
    """d = 32 per head: ds_attention_h3 (one head) and ds_attention_h3_heads, the staging forms (no workspace below L = 2048);
    L = 96: three 32-key tiles, the last query tile of the 128-wide block ragged."""
    E = 32 * heads

    def case(o):
        qkv = o.inp(rnd(141, B, 3 * E, L))
        kw = {}
        if amax == "given":
            am = o.zeroed(2, B)
            ops.absmax_rows(qkv[:, :2 * E], out=am[0])
            ops.absmax_rows(qkv[:, 2 * E:], out=am[1])
            kw["in_amax"] = am
        ops.attention(qkv, E, out=o.out(B, E, L), precision="fp16x3", out_amax=o.slots(B), heads=heads, **kw)
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("kind,E,L", [("ws", 32, 2048), ("ws", 256, 1024), ("heads2", 128, 2048), ("xkv", 256, 1024), ("xkv", 32, 2048)])
def test_attention_image_forms(ops, dev, kind, E, L, poison):
    """The image forms (ATTN_IMAGES_MIN_L): the K / V images of a workspace of exactly attention_workspace_floats floats."""
    heads = 2 if kind == "heads2" else 1
    Bq = 1 if E == 256 else B

    def case(o):
        need = ops.attention_workspace_floats(Bq, E, L, "fp16x3", heads)
        assert need > 0
        ws = o.scratch(need)
        if kind == "xkv":
            q, x = o.inp(rnd(151, Bq, E, L)), o.inp(rnd(152, Bq, E, L, scale=2.0))
            ops.attention_xkv(q, x, E, out=o.out(Bq, E, L), workspace=ws, q_amax=ops.absmax_rows(q, Bq, out=o.zeroed(Bq)),
                              x_amax=ops.absmax_rows(x, Bq, out=o.zeroed(Bq)), out_amax=o.slots(Bq))
        else:
            qkv = o.inp(rnd(153, Bq, 3 * E, L))
            ops.attention(qkv, E, out=o.out(Bq, E, L), precision="fp16x3", workspace=ws, out_amax=o.slots(Bq), heads=heads)
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("E,heads,L,precision", [(32, 1, 35, "fp16x3"), (48, 1, 32, "fp16x3"), (64, 2, 35, "fp16x3"), (48, 2, 37, "fp32"),
                                                 (32, 1, 32, "fp32"), (32, 1, 96, "fp32")])
def test_attention_generic_and_exact(ops, dev, E, heads, L, precision, poison):
    """ds_attention_generic (L % 32 != 0 or an odd width), ds_attention_heads_generic, ds_attention (exact fp32)."""
    def case(o):
        qkv = o.inp(rnd(161, B, 3 * E, L))
        ops.attention(qkv, E, out=o.out(B, E, L), precision=precision, out_amax=o.slots(B), heads=heads)
    run(case, dev, poison)


# ================================================================================================== statistics and tables
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", [(24, 9, 13), (24, 70, 70)])
def test_gnorm1_stats(ops, dev, shape, kind, poison):
    """A hostile workspace of exactly ds_gnorm1_workspace_bytes; 70 x 70 x 24: more than one workgroup per sample."""
    def case(o):
        x = o.inp(rnd(171, B, *shape, shift=3.0))
        ops.gnorm1_stats(x, kind, stats=o.out(B, 2), workspace=o.scratch(ops_workspace_floats(B)))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("shape,Gn", [((24, 9, 13), 4), ((24, 9, 13), 24), ((32, 70, 70), 2), ((24, 3, 9, 13), 3)])
def test_groupnorm_stats_apply(ops, dev, shape, Gn, poison):
    def case(o):
        C = shape[0]
        x = o.inp(rnd(172, B, *shape, shift=3.0))
        st = ops.groupnorm_stats(x, Gn, stats=o.out(B, Gn, 2), workspace=o.scratch(ops_workspace_floats(B * Gn)))
        ops.groupnorm_apply(x, st, o.inp(1 + 0.25 * rnd(173, C)), o.inp(0.25 * rnd(174, C)), Gn, act=True, out=o.out(B, *shape),
                            out_amax=o.slots(B))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("plane", [(9, 13), (20, 36)])
def test_tables_from_tile_statistics(ops, dev, plane, poison):
    """groupnorm_stats_tiles, groupnorm_table (from tiles and from plain stats), gnorm1_stats_tiles and gnorm1_table of a concat,
    from the tile statistics of ragged producers: every table's pad rows and fourth column are the table kernel's to write."""
    H, W = plane

    def case(o):
        d = o.device
        xa = o.inp(rnd(181, B, 24, H, W))
        nt = ops.conv_tile_count(H, W)
        ta, tb = o.out(B, 24, nt, 4), o.out(B, 40, nt, 4)
        am = ops.absmax_rows(xa, out=o.zeroed(B))
        ya = ops.conv(xa, guard_pack(o, ops.pack_conv(conv_w(182, 24, 24, 3, 3).to(d), "fp16x3")), tile_stats=ta, in_amax=am, out=o.out(B, 24, H, W))
        ops.conv(xa, guard_pack(o, ops.pack_conv(conv_w(183, 40, 24, 1, 1).to(d), "fp16x3")), tile_stats=tb, in_amax=am, out=o.out(B, 40, H, W))
        w24, b24 = o.inp(1 + 0.25 * rnd(184, 24)), o.inp(0.25 * rnd(185, 24))
        w64, b64 = o.inp(1 + 0.25 * rnd(186, 64)), o.inp(0.25 * rnd(187, 64))
        ops.groupnorm_stats_tiles(ta, 4, H * W, stats=o.out(B, 4, 2))
        ops.groupnorm_table(w24, b24, 4, H * W, tile_stats=ta, out=o.out(B, 32, 4))
        st = ops.groupnorm_stats(ya, 3, stats=o.out(B, 3, 2), workspace=o.scratch(ops_workspace_floats(B * 3)))
        ops.groupnorm_table(w24, b24, 3, H * W, stats=st, out=o.out(B, 32, 4))
        for kind in (0, 1):
            ops.gnorm1_stats_tiles(ta, kind, H * W, stats_b=tb, stats=o.out(B, 2))
            ops.gnorm1_table(ta, w64, b64, kind, H * W, stats_b=tb, film=o.inp(0.25 * rnd(188, 1, 128)), out=o.out(B, 64, 4))
            ops.inorm_table(tb, o.inp(1 + 0.25 * rnd(189, 40)), o.inp(0.25 * rnd(190, 40)), kind, H * W, out=o.out(B, 48, 4))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
def test_amax_reductions(ops, dev, poison):
    """absmax_rows (contiguous and a channel slice), absmax_channels with hostile zero-contract scratch, input_amax on a hostile
    arena with a live row in the middle: the launch zeroes the arena itself."""
    def case(o):
        x = o.inp(rnd(191, B, 5, 9, 13, scale=4.0))
        ops.absmax_rows(x, out=o.slots(B))
        ops.absmax_rows(x, B * 5, out=o.slots(B * 5))
        ops.absmax_rows(x[:, 1:4], out=o.slots(B))
        big = o.inp(rnd(192, B, 3, 300, 301))                                 # more than one workgroup per row
        ops.absmax_rows(big, out=o.slots(B))
        wmax = o.inp(rnd(193, 5).abs() + 0.5)
        ops.absmax_channels(x, o.slots(B), o.zeroed(B * 5), flag=o.zeroed(1), wmax=wmax)
        arena = o.out(7, B, dtype=torch.int32)                                # poison-filled: ds_input_amax clears every row
        ops.input_amax(arena, 3, x, flag=o.zeroed(1), wmax=wmax)
        a, b = o.inp(torch.tensor([5, 9], dtype=torch.int32)), o.inp(torch.tensor([7, 2], dtype=torch.int32))
        ops.amax_merge(o.slots(B), a, b)
        ops.amax_zero(o.out(3, B, dtype=torch.int32))
    run(case, dev, poison)


# ================================================================================================================= the rest
def _eval_coef(**kw):
    from diffsci_amd._native import EvalCoef
    base = dict(c_out=0.4, c_skip=0.1, sigma_sq=2.0, neg_mult=-1.4, neg_lang=0.0, guidance=2.0, one_minus_guidance=-1.0, input_kind=0,
                stochastic=0, scale=1.0, scale_mult=1.0, next_scale=1.0)
    base.update(kw)
    return EvalCoef(**base)


@pytest.mark.parametrize("poison", POISON)
def test_streaming_layers(ops, dev, poison):
    def case(o):
        E, H, W = 24, 9, 13
        x = o.inp(rnd(201, B, E, H, W, scale=2.0))
        w = o.inp(1 + 0.25 * rnd(202, E))
        mod = o.inp(rnd(203, 5, E))
        ops.channel_rmsnorm(x, w, mod=mod, row=3, out=o.out(B, E, H, W), out_amax=o.slots(B))
        x2 = o.inp(rnd(204, B, E, 10, 14))
        ops.channel_rmsnorm(x2, w, mod=o.inp(rnd(205, B, E)), pool=2, out=o.out(B, E, 5, 7), out_amax=o.slots(B))
        x3 = o.inp(rnd(206, B, E, 9, 15))
        ops.channel_rmsnorm(x3, w, pool=3, out=o.out(B, E, 3, 5), out_amax=o.slots(B), scratch=o.scratch(B, E, 9, 15))
        # rope2d: in place on a qkv whose v third must stay as it was
        L, heads, Eq = 35, 2, 24
        qkv = o.inp(rnd(207, B, 3 * Eq, L))
        cs = o.inp(rnd(208, L, Eq // heads // 2, 2))
        ops.rope2d(qkv, Eq, heads, cs, out_amax=o.slots(2, B))
        k = 5
        ops.depthwise_conv_silu(x, o.inp(conv_w(209, E, 1, k, k)), o.inp(rnd(210, E)), out=o.out(B, E, H, W), out_amax=o.slots(B))
        ops.swiglu(o.inp(rnd(211, B, 2 * E, H, W)), out=o.out(B, E, H, W), out_amax=o.slots(B))
        ops.upsample_bilinear(x, 3, out=o.out(B, E, 3 * H, 3 * W))
        ops.silu_amax(x, out=o.out(B, E, H, W), out_amax=o.slots(B))
        return [qkv]
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
def test_token_layers(ops, dev, poison):
    def case(o):
        C, p, H, W, E = 3, 4, 12, 20, 40
        L = (H // p) * (W // p)                                                 # 15 tokens
        x = o.inp(rnd(221, B, C, H, W))
        tok = ops.patch_embed(x, o.inp(rnd(222, E, C * p * p) / 7), o.inp(rnd(223, E)), p, out=o.out(B, E, L))
        mod = o.inp(rnd(224, 5, 6 * E))
        ln = ops.token_layernorm(tok, o.inp(1 + 0.25 * rnd(225, E)), o.inp(0.25 * rnd(226, E)), mod, 3, 4, 2, out=o.out(B, E, L),
                                 out_amax=o.slots(B))
        ops.token_gate(tok, ln, mod, chunk=5, row=2, out=o.out(B, E, L))
        ops.patch_unembed(ln, o.inp(rnd(227, C * p * p, E) / 7), o.inp(rnd(228, C * p * p)), p, (B, C, H, W), out=o.out(B, C, H, W))
        t2 = o.inp(rnd(229, B, 3 * E, L))
        ops.token_l2_normalize(t2, E, E, gain=2.0)                              # in place on the middle third only
        return [t2]
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
def test_resampling(ops, dev, poison):
    def case(o):
        C = 5
        x = o.inp(rnd(231, B, C, 9, 15, scale=2.0))
        x1 = o.inp(rnd(232, 1, C, 9, 15))
        te = o.inp(rnd(233, B, C))
        ops.cornerpool_f(x, 3, te=te, out=o.out(B, C, 3, 5), out_amax=o.slots(B))
        ops.cornerpool_f(x1, 3, te=te, out=o.out(B, C, 3, 5), out_amax=o.slots(B))         # x broadcast over the batch
        v = o.inp(rnd(234, B, C, 4, 6, 9))
        ops.cornerpool_f(o.inp(rnd(235, B, C, 4, 6, 10)), 2, te=o.inp(rnd(236, 1, C)), out=o.out(B, C, 2, 3, 5), out_amax=o.slots(B))
        for f in (2, 3):
            ops.maxpool_f(x, f, out=o.out(B, C, 9 // f, 15 // f))
            ops.avgpool_f(x, f, out=o.out(B, C, 9 // f, 15 // f))
            ops.upsample_f(x, f, out=o.out(B, C, 9 * f, 15 * f))
        ops.maxpool_f(v, 2, out=o.out(B, C, 2, 3, 4))
        ops.avgpool_f(v, 2, out=o.out(B, C, 2, 3, 4))
        ops.upsample_f(v, 2, out=o.out(B, C, 8, 12, 18))
        ops.avgpool3d(o.inp(rnd(237, B, C, 4, 6, 10)), out=o.out(B, C, 2, 3, 5))
        ops.upsample3d(v, out=o.out(B, C, 8, 12, 18))
        st = ops.gnorm1_stats(x, 0, stats=o.out(B, 2), workspace=o.scratch(ops_workspace_floats(B)))
        wn, bn = o.inp(1 + 0.25 * rnd(238, C)), o.inp(0.25 * rnd(239, C))
        film = o.inp(0.25 * rnd(240, B, 2 * C))
        ops.gnorm1_apply_poolf(x, st, wn, bn, 0, 3, film=film, out=o.out(B, C, 3, 5))
        ops.gnorm1_apply(x, st, wn, bn, 0, film=film, out=o.out(B, C, 9, 15))
        x4 = o.inp(rnd(241, B, C, 10, 14))
        st4 = ops.gnorm1_stats(x4, 1, stats=o.out(B, 2), workspace=o.scratch(ops_workspace_floats(B)))
        ops.gnorm1_apply(x4, st4, wn, bn, 1, pool=True, out=o.out(B, C, 5, 7))
        ops.inorm_silu(x, wn, bn, 0, out=o.out(B, C, 9, 15))
        ops.concat2(x4, o.inp(rnd(242, B, 2, 10, 14)), out=o.out(B, C + 2, 10, 14))          # per-sample sizes: multiples of four
        ops.crop_blend(o.inp(rnd(243, B, 3, 13, 17)), (2, 3), (2, 2), out=o.out(B, 3, 9, 11))
        ops.crop_blend(o.inp(rnd(244, B, 3, 7, 13, 17)), (1, 2, 3), (1, 2, 2), out=o.out(B, 3, 5, 9, 11))
    run(case, dev, poison)


@pytest.mark.parametrize("poison", POISON)
def test_steppers(ops, dev, poison):
    """n = 2 * 351 = 702: not a multiple of four (a vector body and a two-element tail); xin_copies = 2 writes the network input twice."""
    from diffsci_amd._native import DDPMCoef, SIStep

    def case(o):
        shape = (B, 3, 9, 13)
        n = B * 3 * 9 * 13
        x, f1, f2, u1, u2, eps = (o.inp(rnd(250 + i, *shape, scale=s)) for i, s in enumerate((80.0, 1.0, 1.0, 1.0, 1.0, 1.0)))
        k1, k2 = _eval_coef(xin_copies=2), _eval_coef(sigma_sq=1.5, xin_copies=2)
        ops.euler(x, f1, k1, -3.5, fu=u1, x_out=o.out(*shape), xin_out=o.out(2 * n), c_in_next=0.3)
        ops.euler(x, f1, _eval_coef(stochastic=1, neg_lang=-0.7, xin_copies=2), -3.5, fu=u1, x_out=o.out(*shape), xin_out=o.out(2 * n),
                  c_in_next=0.3, eps=eps, noise_coef=1.3, sqrt_abs_dt=0.9)
        ops.heun(x, f1, k1, f2, k2, -3.5, f1u=u1, f2u=u2, x_out=o.out(*shape), xin_out=o.out(2 * n), c_in_next=0.25)
        ops.churn(x, eps, 3.25, o.out(*shape), xin_out=o.out(2 * n), c_in=0.5, ratio=0.9, scale=2.0, xin_copies=2)
        state = torch.tensor([0x5EED, 4000], dtype=torch.int64, device=o.device)
        ops.churn(x, None, 3.25, o.out(*shape), xin_out=o.out(2 * n), c_in=0.5, philox=(state, 16), xin_copies=2)
        ops.philox_normal(state, 8, (n,), out=o.out(n))
        for form, co in (("classical", (0.014, 1.005, 0.098, 0.0, 0.0)), ("generalized", (0.957, 0.289, 0.290, 0.952, 0.095)),
                         ("forward", (0.995, 0.0098, 0.0, 0.0, 0.0))):
            f = None if form == "forward" else f1
            ops.ddpm_step(x, f, DDPMCoef(*co, None), form, eps=eps, out=o.out(*shape))
            ops.ddpm_step(x, f, DDPMCoef(*co, None), form, philox=(state, 32), out=o.out(*shape))
        s = SIStep(1.0, 1.0, -1.0, -0.5, -0.25, 0.5, 0.75, 0.25, 0.5, 0.5, 0.7)
        ks = _eval_coef(guidance=1.0, one_minus_guidance=0.0, xin_copies=2)
        x_orig, mask = o.inp(rnd(260, 3, 9, 13)), o.inp((rnd(261, 3, 9, 13) > 0).float())
        draws = (eps, o.inp(rnd(262, 3, 9, 13)), o.inp(rnd(263, *shape)), o.inp(rnd(264, 3, 9, 13)))
        for blend, renoise in ((False, False), (True, False), (True, True)):
            ops.si_inpaint_step(x, f1, ks, s, x_orig=x_orig, mask=mask, blend=blend, renoise=renoise, eps=draws, x_out=o.out(*shape),
                                xin_out=o.out(2 * n))
            ops.si_inpaint_step(x, f1, ks, s, x_orig=x_orig, mask=mask, blend=blend, renoise=renoise, philox=(state, 64),
                                x_out=o.out(*shape), xin_out=o.out(2 * n))
        m = o.inp(torch.cat([rnd(265, B, 4, 9, 13), rnd(266, B, 4, 9, 13, scale=0.3)], dim=1))
        ops.posterior_sample(m, eps=o.inp(rnd(267, B, 4, 9, 13)), clamp=(-30.0, 20.0), out=o.out(B, 4, 9, 13))
        ops.scale(x, 0.5, out=o.out(*shape))
        ops.add(x, f1, out=o.out(*shape))
        ops.axpby(x, 0.5, f1, 2.0, out=o.out(*shape))
        ops.mask_blend(x, f1, mask, out=o.out(*shape))
        ops.drift(x, f1, k1, fu=u1, out=o.out(*shape))
        ops.score(x, f1, k1, fu=u1, out=o.out(*shape))
        ops.denoiser(x, f1, o.inp(rnd(269, B)), o.inp(rnd(270, B)), fu=u1, guidance=2.0, out=o.out(*shape))
    run(case, dev, poison)


# ============================================================================ the consumers do read what the inventory says they read
@pytest.mark.parametrize("what", ["table_pad_rows", "table_fourth_column", "image_border", "image_pad_channels"])
def test_consumers_read_their_pads(ops, dev, what):
    """The other direction: with one pad region poisoned by hand after its producer ran, the consuming convolution's output changes
    (the pad rows and the fourth column of a norm table, the border and the channels past C of the pre-split
    images).  So the cases above pass because the producers write those regions, not because nobody looks."""
    C, Cout, H, W = 24, 40, 20, 36
    nan = float("nan")
    x = rnd(301, B, C, H, W).to(dev)
    pw = ops.pack_conv(conv_w(302, Cout, C, 3, 3).to(dev), "fp16x3")
    if what.startswith("table"):
        tab = torch.zeros(B, ops.table_channels(C), 4, device=dev)
        tab[:, :C, 1] = 1.0
        want = ops.conv(x, pw, prenorm=tab)
        if what == "table_pad_rows":
            tab[:, C:] = nan
        else:
            tab[:, :, 3] = nan
        got = ops.conv(x, pw, prenorm=tab)
    else:
        images = ops.inorm_silu_images(x, None, None, 0)
        want = ops.conv_img(images, pw, B, C, H, W)
        v = images.view(B, 2, 2, 2, H + 2, W + 2, 4)              # [B][chunk][piece][half][H + 2][W + 2] x 8 fp16 channels
        if what == "image_border":
            v[:, :, :, :, 0] = nan
        else:
            v[:, 1, :, 1] = nan                                    # channels 24 .. 31: chunk 1, half 1
        got = ops.conv_img(images, pw, B, C, H, W)
    assert bool(torch.isfinite(want).all()) and not torch.equal(got.view(torch.int32), want.view(torch.int32))
