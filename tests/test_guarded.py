"""tests/guarded.py rejects what it is there to reject: faulty ops emulated in torch on the CPU -- a store past and before the
output, a band element read into a sum at weight zero, a maximum over a band element, an output element left unwritten, an
amax slot overwritten instead of merged -- and admits the correct op.  Each fault is tried with both poisons; the table says
which poison has to catch it (the other one may miss it: that is why every GPU case runs with both)."""
import pytest
import torch

from tests import guarded as G

CPU = torch.device("cpu")
N = 37                       # not a multiple of four: the view's end is not 16-byte aligned, its start is


def _beyond(t, offset, count=1):
    """`count` elements of t's storage starting `offset` elements from the view's start (negative: before it)."""
    return torch.as_strided(t, (count,), (1,), t.storage_offset() + offset)


def _scaled_sum(o, stray=None):
    """out = 2 x + y; amax slot merged.  `stray`: the fault to commit."""
    g = torch.Generator().manual_seed(7)
    x, y = o.inp(torch.randn(N, generator=g)), o.inp(torch.randn(N, generator=g))
    out, slot = o.out(N), o.slots(2)
    res = 2 * x + y
    amax = res.abs().max().view(1).view(torch.int32).expand(2)
    if stray == "read_sum":
        res = res + 0.0 * _beyond(x, N)                       # one element past x, weight zero
    if stray == "read_max":
        amax = torch.maximum(res.abs().max(), _beyond(y, -1).abs().max()).view(1).view(torch.int32).expand(2)
    if stray == "unwritten":                                  # element N // 2 keeps what the buffer held before the call
        out[:N // 2].copy_(res[:N // 2])
        out[N // 2 + 1:].copy_(res[N // 2 + 1:])
    else:
        out.copy_(res)
    if stray == "store_past":
        _beyond(out, N)[0] = 1.0
    if stray == "store_before":
        _beyond(out, -1)[0] = 1.0
    if stray == "overwrite_slot":
        slot.copy_(amax)
    else:
        slot.copy_(torch.maximum(slot, amax))


def _case(stray):
    return lambda o: _scaled_sum(o, stray)


def test_band_geometry():
    assert G.band_elems(1) == 4096 and G.band_elems(4096) == 4096 and G.band_elems(4097) == 5120 and G.band_elems(10240) == 10240
    o = G.Operands(CPU, G.NAN_BITS)
    v = o.out(3, 5, 7)
    it = o.items[0]
    assert it.band >= v.numel() and it.band % 4 == 0 and v.data_ptr() % 16 == 0 and v.is_contiguous()
    assert it.buf.numel() == v.numel() + 2 * it.band
    assert torch.isnan(v).all() and torch.isnan(it.buf.view(torch.float32)).all()
    assert torch.isnan(it.buf.view(torch.float16)).all()                       # both halves: the packed fp16 images
    h = G.Operands(CPU, G.HUGE_BITS).scratch(4)
    assert torch.equal(h, torch.full((4,), 3.0e38)) and torch.isfinite(h).all()
    z = G.Operands(CPU, G.NAN_BITS).zeroed(2, 3)
    assert z.dtype == torch.int32 and not z.any()
    assert G.NAN_BITS > torch.tensor(3.4e38).view(torch.int32).item()          # as an amax slot: above any finite bits


@pytest.mark.parametrize("poison", list(G.POISONS))
def test_correct_op_is_admitted(poison):
    assert G.check(_case(None), CPU, G.POISONS[poison]) == []


# fault -> the poison that must reject it
FAULTS = {"store_past": ("nan", "huge"), "store_before": ("nan", "huge"), "read_sum": ("nan",), "read_max": ("huge",),
          "unwritten": ("nan", "huge"), "overwrite_slot": ("nan", "huge")}


@pytest.mark.parametrize("fault,poison", [(f, p) for f, ps in FAULTS.items() for p in ps])
def test_faulty_op_is_rejected(fault, poison):
    bad = G.check(_case(fault), CPU, G.POISONS[poison])
    assert bad, f"{fault} passed under the {poison} poison"
    text = "\n".join(bad)
    if fault in ("store_past", "store_before"):
        assert "band " + ("after" if fault == "store_past" else "before") in text
    if fault == "overwrite_slot":
        assert "not merged" in text
    with pytest.raises(AssertionError):
        G.assert_clean(_case(fault), CPU, G.POISONS[poison])


def test_each_poison_is_needed():
    """3e38 * 0 = 0 hides a stray read in a sum; a maximum drops a NaN (fmaxf's rule: torch.fmax on the CPU)."""
    assert G.check(_case("read_sum"), CPU, G.HUGE_BITS) == []
    nan = torch.tensor(G.NAN_BITS, dtype=torch.int32).view(torch.float32)
    assert torch.fmax(torch.tensor(1.0), nan).item() == 1.0
