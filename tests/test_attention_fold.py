"""The single-head attention block with its K and V projections folded into the Q and the output projection:
the identity in fp64 against nn.MultiheadAttention, the conditions under which runtime.attention takes the folded route, and the
ABI of the entry point it launches.  Host only.

Bound of the identity: relative 1e-12 in max-abs, 1000 x the 8.9e-16 the fold measures at E = 32 -- room for the E = 256 sums."""
import ctypes
import os
import re

import pytest
import torch

from diffsci_amd import _native, ops
from diffsci_amd.models.nets import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(E, seed):
    torch.manual_seed(seed)
    m = torch.nn.MultiheadAttention(E, 1, batch_first=True).double()
    with torch.no_grad():
        m.in_proj_bias.normal_()
        m.out_proj.bias.normal_()
    return m


def _folded_forward(m, x):
    """x [B, L, E] -> the block through (M, c, W', b'): queries M x + c, keys and values x itself."""
    E = m.embed_dim
    M, c, Wp, bp = runtime.fold_attention_weights(m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias)
    assert all(t.dtype == torch.float64 for t in (M, c, Wp, bp))
    q = x @ M.t() + c
    p = torch.softmax(q @ x.transpose(1, 2) / E ** 0.5, dim=-1)
    return (p @ x) @ Wp.t() + bp


@pytest.mark.parametrize("E", [32, 256])
def test_fold_reproduces_the_module_in_fp64(E):
    L, B = 48, 2
    m = _module(E, 7 + E)
    x = torch.randn(B, L, E, dtype=torch.float64, generator=torch.Generator().manual_seed(E))
    with torch.no_grad():
        want = m(x, x, x, need_weights=False)[0]
        got = _folded_forward(m, x)
        err = float((got - want).abs().max() / want.abs().max())
        print(f"[fold] E={E}: folded vs module, relative max-abs {err:.3e} on values up to {float(want.abs().max()):.2f}")
        assert err <= 1e-12
        # the key bias reaches the logits only through a term without the key index: the softmax removes it
        m.in_proj_bias[E:2 * E] *= 100
        again = _folded_forward(m, x)
        assert torch.equal(again, got)


def test_fold_without_biases():
    """The in-house attention carries no biases: c and b' are None, M and W' the same products."""
    E = 32
    g = torch.Generator().manual_seed(3)
    w_in, w_out = torch.randn(3 * E, E, generator=g), torch.randn(E, E, generator=g)
    M, c, Wp, bp = runtime.fold_attention_weights(w_in, None, w_out, None)
    assert c is None and bp is None
    assert torch.equal(M, w_in[E:2 * E].double().t() @ w_in[:E].double()) and torch.equal(Wp, w_out.double() @ w_in[2 * E:].double())
    assert runtime.fold_attention_weights(w_in, None, w_out, torch.ones(E))[3].tolist() == [1.0] * E


def _bundle(kind="fp16x3", E=256):
    pack = ops.PackedConv(None, E, E, 1, kind)
    return runtime.FoldedAttention(pack, None, pack, None)


def test_route_conditions():
    takes = lambda b, E, L, heads=1, precision="fp16x3", cosine=False: runtime.attention_folds(b, E, L, heads, precision, cosine)
    assert takes(_bundle(), 256, 1024)
    assert not takes(None, 256, 1024)
    assert not takes(_bundle(), 256, 1024, heads=2)
    assert not takes(_bundle(), 256, 1024, cosine=True)
    assert not takes(_bundle("fp32"), 256, 1024, precision="bf16x6")           # what PUNetG packs after an escalation to bf16x6
    assert not takes(_bundle("bf16x6"), 256, 1024) and not takes(_bundle(), 256, 1024, precision="bf16x6")
    assert not takes(_bundle(E=32), 32, 16)
    assert not takes(_bundle(), 256, 512) and not takes(_bundle(E=32), 32, 1024) and takes(_bundle(E=32), 32, 2048)


def test_punetg_switch_and_packed_keys(monkeypatch):
    import diffsci_amd.models as M
    from diffsci_amd.models.karras import engine
    monkeypatch.delenv("DIFFSCI_ATTN_FOLD", raising=False)
    net = M.PUNetG(M.PUNetGConfig(model_channels=8))
    assert net.attn_fold is True and "attn_fold" in engine.MODEL_SWITCHES
    a = engine.model_signature(net)
    net.attn_fold = False
    assert engine.model_signature(net) != a                  # the route is part of a captured plan's key
    monkeypatch.setenv("DIFFSCI_ATTN_FOLD", "0")
    assert M.PUNetG(M.PUNetGConfig(model_channels=8)).attn_fold is False


def test_packed_weights_keeps_its_key_set(monkeypatch):
    """packed_weights() names what it named before the fold existed: per convolution id(m) (+ the input layer's guard), per
    attention block (id, "in") and (id, "out") -- the folded packings live in a cache of their own."""
    import diffsci_amd.models as M
    net = M.PUNetG(M.PUNetGConfig(model_channels=8))
    monkeypatch.setattr(ops, "pack_conv", lambda w, precision="bf16x6", upsampled=False: ("pack", tuple(w.shape), precision))
    keys = set(net.packed_weights())
    convs = list(net._conv_modules())
    want = {id(m) for m in convs} | {(id(net.convin), "wmax")}
    want |= {(id(a), k) for a in net.attn_block for k in ("in", "out")}
    assert len(net.attn_block) > 0 and keys == want
    assert "_attn_folded" not in net.__dict__


def test_entry_point_is_declared_bound_and_not_stream_last():
    src = open(os.path.join(ROOT, "include", "diffsci_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int\s+ds_attention_h3_xkv\s*\((.*?)\)\s*;", src, re.S)
    assert decl, "ds_attention_h3_xkv is not declared in include/diffsci_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["out", "q", "x", "workspace", "B", "E", "L", "q_amax", "k_amax", "v_amax",
                                                           "out_amax", "stream", "flags"]
    res, args = _native._PROTOS["ds_attention_h3_xkv"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[-1] is ctypes.c_int and args[-2] is ctypes.c_void_p               # the flags word closes the list, not the stream
    for p, a in zip(params, args):
        assert (a is ctypes.c_void_p) == ("*" in p) and (a is ctypes.c_int) == p.startswith("int ")
    import build
    lib = ctypes.CDLL(build.build(force=False, verbose=False))
    assert hasattr(lib, "ds_attention_h3_xkv")


def test_wrapper_refuses_what_the_image_form_does_not_take(monkeypatch):
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    q = torch.zeros(2, 32, 64)
    with pytest.raises(ValueError, match="image form"):
        ops.attention_xkv(q, q.clone(), 32)
    with pytest.raises(ValueError, match=r"must be \[B, E"):
        ops.attention_xkv(torch.zeros(2, 256, 1024), torch.zeros(2, 256, 512), 256)
