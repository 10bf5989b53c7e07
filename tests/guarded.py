"""Operands on hostile memory.  A kernel under test gets every tensor as a contiguous view inside one larger allocation with a
guard band on both sides: the tensor's own size rounded up to a multiple of 1024 four-byte elements, at least 4096 -- an index
error of up to one whole tensor lands in memory the test owns and shows as a failed assertion, not as a fault; the band is a
multiple of four elements, so the view keeps the allocation's 16-byte alignment (the C ABI's requirement).  Inputs sit in bands
of a poison; outputs and scratch buffers are filled with the poison themselves.  Buffers whose contract is "zeroed by the
caller" (the out_amax slots) are seeded with known values instead, and the merge is checked.

Two poisons, both written through an int32 view:
  NAN_BITS   0x7FC07FC0: NaN as fp32, both 16-bit halves NaN as fp16 (the pre-split images); as an amax slot, above any finite bits.
             A stray read into a sum shows even at weight zero (NaN * 0 = NaN).
  HUGE_BITS  3.0e38f: fmaxf drops a NaN, so maxima (max-pool loaders, amax reductions) need a huge finite value to show a stray
             read -- which a sum would hide (3e38 * 0 = 0).

The oracle is the same call on clean operands (poison=None): every operand in a zero-filled allocation of its own, with the
same layout.  check(case, device, poison) runs `case(operands)` on both and requires every out(), slots() and zeroed() operand,
and whatever the case returns, to agree bit for bit, and every band of the hostile run to be intact.

A case is a function of one Operands that builds its inputs deterministically (seeded CPU generators), takes its tensors from
the Operands in a fixed order, calls the op, and returns None or a list of further tensors to compare.
"""
import struct

import torch

NAN_BITS = 0x7FC07FC0
HUGE_BITS = struct.unpack("<i", struct.pack("<f", 3.0e38))[0]
POISONS = {"nan": NAN_BITS, "huge": HUGE_BITS}
# slot seeds: the merge is max() over float bits; a zero seed shows the produced value, a huge finite one must survive the call
SEED_BITS = struct.unpack("<i", struct.pack("<f", 2.5e38))[0]
MIN_BAND, BAND_UNIT = 4096, 1024


def band_elems(n):
    """Band on each side of an n-element operand."""
    return max(MIN_BAND, (int(n) + BAND_UNIT - 1) // BAND_UNIT * BAND_UNIT)


class _Operand:
    __slots__ = ("kind", "buf", "view", "band", "n", "seed", "name")


class Operands:
    """poison: one of the POISONS' bit patterns, or None for the clean oracle (zero bands, zero-filled outputs)."""

    def __init__(self, device, poison=None):
        self.device, self.poison = torch.device(device), poison
        self.items = []

    # ------------------------------------------------------------------------------------------------------------------------
    def _place(self, kind, shape, dtype, name):
        if dtype not in (torch.float32, torch.int32):
            raise TypeError("guarded operands are four-byte elements (float32 / int32)")
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        band = band_elems(n)
        buf = torch.zeros(n + 2 * band, dtype=torch.int32, device=self.device)
        if self.poison is not None:
            buf.fill_(self.poison)
        o = _Operand()
        o.kind, o.buf, o.band, o.n, o.seed = kind, buf, band, n, None
        o.name = name or f"{kind}{len(self.items)}{list(shape)}"
        o.view = buf[band:band + n].view(dtype).view(shape)
        assert o.view.is_contiguous() and buf.data_ptr() % 16 == 0 and o.view.data_ptr() % 16 == 0 and band % 4 == 0
        self.items.append(o)
        return o

    def inp(self, t, name=None):
        """A copy of t (float32 / int32, any device) between poisoned bands."""
        o = self._place("in", t.shape, t.dtype, name)
        o.view.copy_(t)
        return o.view

    def out(self, *shape, dtype=torch.float32, name=None):
        """An output the op must write completely: poison-filled; compared with the clean run."""
        return self._place("out", shape, dtype, name).view

    def scratch(self, *shape, dtype=torch.float32, name=None):
        """Scratch whose content after the call is nobody's business: poison-filled; only its bands are checked."""
        return self._place("scratch", shape, dtype, name).view

    def zeroed(self, *shape, name=None):
        """int32 slots a consumer in the same case reads back: zero, as the contract asks; compared with the clean run."""
        o = self._place("out", shape, torch.int32, name)
        o.view.zero_()
        return o.view

    def slots(self, *shape, name=None):
        """int32 amax slots nobody in the case reads back.  Clean run: zero, so they end as the produced value.  Hostile run:
        even entries zero, odd entries SEED_BITS; after the call they must hold max(seed, produced value)."""
        o = self._place("slots", shape, torch.int32, name)
        o.view.zero_()
        if self.poison is not None:
            o.view.view(-1)[1::2] = SEED_BITS
        o.seed = o.view.clone()
        return o.view

    # ------------------------------------------------------------------------------------------------------------------------
    def broken_bands(self):
        """Names of the operands with a changed band (hostile run), with the first changed offset relative to the view."""
        bad = []
        for o in self.items:
            fill = 0 if self.poison is None else self.poison
            for side, band, base in (("before", o.buf[:o.band], -o.band), ("after", o.buf[o.band + o.n:], o.n)):
                ne = (band != fill).nonzero()
                if ne.numel():
                    bad.append(f"{o.name}: band {side} changed at element {base + int(ne[0])} ({ne.numel()} in all)")
        return bad


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def _first_diff(a, b):
    ne = (_bits(a) != _bits(b)).view(-1).nonzero()
    i = int(ne[0])
    return f"{ne.numel()} of {a.numel()} elements differ, first at flat index {i}: {a.reshape(-1)[i].item()!r} vs {b.reshape(-1)[i].item()!r}"


def check(case, device, poison):
    """Run `case` on clean and on hostile operands; -> list of complaints (empty: the op passed)."""
    clean, hostile = Operands(device), Operands(device, poison)
    want_extra = case(clean) or []
    got_extra = case(hostile) or []
    bad = hostile.broken_bands() + ["clean run: " + s for s in clean.broken_bands()]
    if len(clean.items) != len(hostile.items) or len(want_extra) != len(got_extra):
        return bad + ["the case took different operands in its two runs"]
    for c, h in zip(clean.items, hostile.items):
        if c.kind != h.kind or c.view.shape != h.view.shape:
            return bad + ["the case took different operands in its two runs"]
        if c.kind == "out" and not torch.equal(_bits(c.view), _bits(h.view)):
            bad.append(f"{h.name}: {_first_diff(h.view, c.view)} (hostile vs clean)")
        if c.kind == "slots":
            want = torch.maximum(h.seed, c.view)               # non-negative float bits order as integers
            if not torch.equal(h.view, want):
                bad.append(f"{h.name}: not merged: {_first_diff(h.view, want)} (got vs max(seed, clean))")
    for i, (w, g) in enumerate(zip(want_extra, got_extra)):
        if w.shape != g.shape or not torch.equal(_bits(w), _bits(g)):
            bad.append(f"returned[{i}]: " + (_first_diff(g, w) if w.shape == g.shape else "shapes differ"))
    return bad


def assert_clean(case, device, poison):
    bad = check(case, device, poison)
    assert not bad, "\n".join(bad)
