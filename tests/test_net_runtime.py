"""Host logic the networks share (diffsci_amd/models/nets/runtime.py): the weight-cache signature, the row selection of a
tabulated shift and the amax arena's bookkeeping.  No GPU."""
import pytest
import torch

from diffsci_amd.models.nets import runtime


def test_weights_signature_tracks_updates_and_extras():
    w = torch.nn.Parameter(torch.randn(4, 3))
    b = torch.nn.Parameter(torch.zeros(4))
    sig = runtime.weights_signature([w, b], "fp16x3")
    assert sig == runtime.weights_signature([w, b], "fp16x3")           # nothing changed: equal
    assert sig != runtime.weights_signature([w, b], "bf16x6")           # the switches in front
    assert sig != runtime.weights_signature([w, b], "fp16x3", True)
    assert sig[0] == "fp16x3" and len(sig) == 3
    with torch.no_grad():
        w.mul_(2.0)
    after = runtime.weights_signature([w, b], "fp16x3")
    assert after != sig and after[2] == sig[2]                          # w's entry moved, b's did not


def test_weights_signature_takes_inference_tensors():
    """A module built under torch.inference_mode(): its parameters carry no version counter (reading t._version raises)."""
    with torch.inference_mode():
        lin = torch.nn.Linear(3, 4)
    assert lin.weight.is_inference()
    with pytest.raises(RuntimeError, match="version counter"):
        lin.weight._version
    sig = runtime.weights_signature([lin.weight, lin.bias], "fp16x3")
    assert sig == runtime.weights_signature([lin.weight, lin.bias], "fp16x3")
    assert sig[1] == (lin.weight.data_ptr(), 0, "cpu")


def test_networks_built_under_inference_mode_have_signatures():
    """The networks' own caches go through weights_signature: norms_in_window (every residual block asks it) takes such norms."""
    from diffsci_amd.models.nets import precision
    with torch.inference_mode():
        norms = (torch.nn.GroupNorm(4, 4), torch.nn.GroupNorm(4, 4))
    cache = {}
    assert precision.norms_in_window(cache, 0, norms) is True
    assert precision.norms_in_window(cache, 0, norms) is True and len(cache) == 1


def test_shift_rows_table():
    B, C = 3, 5
    field = torch.randn(B, C, 4, 4)
    assert runtime.shift_rows(field, None, B) is field                  # a field of shifts passes through
    assert runtime.shift_rows(field, 2, B) is field
    per_sample = torch.randn(7, B, C)                                   # [n_evals, B, C] with row
    assert torch.equal(runtime.shift_rows(per_sample, 4, B), per_sample[4])
    table = torch.randn(7, C)                                           # [M, C] with row: one row for the whole batch
    got = runtime.shift_rows(table, 4, B)
    assert got.shape == (1, C) and torch.equal(got, table[4:5])
    for n in (1, B):                                                    # [1 or B, C] without row
        s = torch.randn(n, C)
        assert runtime.shift_rows(s, None, B) is s


def test_shift_rows_refuses_a_wrong_batch():
    B, C = 3, 5
    with pytest.raises(ValueError, match="time embedding batch does not match x"):
        runtime.shift_rows(torch.randn(2, C), None, B)
    with pytest.raises(ValueError, match="time embedding batch does not match x"):
        runtime.shift_rows(torch.randn(7, B + 1, C), 4, B)              # the 3-D form


def test_amax_arena_hands_out_its_rows_then_raises(monkeypatch):
    from diffsci_amd import ops
    monkeypatch.setattr(ops, "amax_zero", lambda t: t.zero_())          # the fill launch, on the host
    ws = runtime.Workspace()
    n, B = 5, 2
    am = runtime.AmaxArena(ws, B, torch.device("cpu"), rows=n)
    assert am.buf.shape == (n, B) and ws.bytes == n * B * 4             # the row count is part of the workspace key
    pair = am.rows(2)
    assert pair.shape == (2 * B,) and pair.dtype == torch.int32
    got = [am.row() for _ in range(n - 2)]
    assert all(r.shape == (B,) for r in got) and len({r.data_ptr() for r in got}) == n - 2
    with pytest.raises(RuntimeError, match="amax arena exhausted"):
        am.row()
    with pytest.raises(RuntimeError, match="amax arena exhausted"):
        am.rows(1)
    am.release()
    assert runtime.AmaxArena(ws, B, torch.device("cpu"), rows=n).buf is am.buf      # the same buffer again: no allocation
    assert runtime.AmaxArena(ws, B, torch.device("cpu"), zero=False).buf.shape == (runtime.AmaxArena.ROWS, B)
