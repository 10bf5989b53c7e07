"""DiffusionTransformer (diffsci_amd/models/nets/dit.py) on the host: the reference's surface -- constructor, attributes,
state_dict keys and shapes, strict loading of its checkpoints -- from the fixtures tools/make_dit_golden.py recorded, the torch
restatement tests/dit_ref.py pinned against the reference's own outputs, and the refusals raised before any launch."""
import inspect
import json
import os
import re

import pytest
import torch

from tests import dit_ref
from tests.golden_util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("a", "b", "c")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


def test_exported_like_punetg(M):
    import diffsci_amd.models.nets as nets
    from diffsci_amd.models.nets.dit import DiffusionTransformer
    assert M.DiffusionTransformer is nets.DiffusionTransformer is DiffusionTransformer


def test_constructor_signature_and_defaults(M):
    v, _, _ = dit_ref.load_golden("a")
    ref = json.loads(v["signature"])
    got = [[n, p.kind.name, p.default] for n, p in inspect.signature(M.DiffusionTransformer.__init__).parameters.items() if n != "self"]
    assert got == ref
    net = M.DiffusionTransformer()
    for name, _, default in ref:
        assert getattr(net, name) == default
    net = M.DiffusionTransformer(128, 8, 2, 3, 2, 3)
    assert (net.nembed, net.nheads, net.mlp_factor, net.nblocks, net.patch_size, net.nchannels) == (128, 8, 2, 3, 2, 3)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_shapes_and_strict_load(M, tag):
    v, sd, kw = dit_ref.load_golden(tag)
    net = M.DiffusionTransformer(**kw)
    assert [[k, list(t.shape)] for k, t in net.state_dict().items()] == json.loads(v["keys"])
    assert len(sd) == len(json.loads(v["keys"]))
    net.load_state_dict(sd, strict=True)
    assert all(torch.equal(net.state_dict()[k], sd[k]) for k in sd)
    assert net.time_embed.W.numel() == net.nembed // 2 and net.positional_encoding.div_term.numel() == net.nembed // 4
    assert "positional_encoding.div_term" in dict(net.named_buffers()) and "time_embed.W" in dict(net.named_buffers())


def test_two_blocks_have_68_entries(M):
    assert len(M.DiffusionTransformer(nblocks=2).state_dict()) == 68


def test_engine_protocol_attributes(M):
    from diffsci_amd.models.karras.engine import MODEL_SWITCHES, model_signature
    net = M.DiffusionTransformer(nblocks=1)
    assert net.conv_precision == "fp16x3" and net.auto_precision is True and net.capturable is True
    for name in ("embed_time", "time_shifts", "forward_with_shifts", "forward", "forward_unguarded"):
        assert callable(getattr(net, name))
    assert "conv_precision" in MODEL_SWITCHES
    a = model_signature(net)
    net.conv_precision = "fp32"
    assert model_signature(net) != a                      # whatever selects kernels is part of a captured plan's key


@pytest.mark.parametrize("tag", TAGS)
def test_dit_ref_reproduces_the_reference(tag):
    v, sd, kw = dit_ref.load_golden(tag)
    nheads, p = kw.get("nheads", 4), kw.get("patch_size", 4)
    ref_err = rel_l2(v["out_f32"], v["out_f64"])
    with torch.inference_mode():
        o64 = dit_ref.dit_forward({k: t.double() for k, t in sd.items()}, v["x"], v["t"], nheads, p)
        o32 = dit_ref.dit_forward(sd, v["x"], v["t"], nheads, p)
    e64, e32 = rel_l2(o64, v["out_f64"]), rel_l2(o32, v["out_f64"])
    print(f"dit_{tag}: dit_ref fp64 vs reference fp64 {e64:.2e}; dit_ref fp32 vs fp64 {e32:.2e}; reference fp32 vs fp64 {ref_err:.2e}")
    assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o64.shape == v["out_f64"].shape
    assert e64 <= 1e-13
    assert e32 <= ref_err


def test_refusals_before_any_launch(M, monkeypatch):
    from diffsci_amd import _native
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    net = M.DiffusionTransformer(nblocks=1, patch_size=4, nchannels=1)
    t = torch.zeros(2)
    with pytest.raises(ValueError, match=r"30x32.*patch_size=4"):
        net(torch.zeros(2, 1, 30, 32), t)
    with pytest.raises(ValueError, match=r"32x18.*patch_size=4"):
        net(torch.zeros(2, 1, 32, 18), t)
    with pytest.raises(ValueError, match=r"nchannels=1.*got 3"):
        net(torch.zeros(2, 3, 32, 32), t)
    with pytest.raises(ValueError, match="3-D"):
        net(torch.zeros(1, 32, 32), t)
    with pytest.raises(ValueError, match="5-D"):
        net.forward_with_shifts(torch.zeros(2, 1, 1, 32, 32), [None])
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        net(torch.zeros(2, 1, 32, 32), t)
    assert not calls


def test_nembed_must_divide_by_nheads_as_in_torch(M):
    with pytest.raises(AssertionError) as ours:
        M.DiffusionTransformer(nembed=64, nheads=3)
    with pytest.raises(AssertionError) as torchs:
        torch.nn.MultiheadAttention(64, 3)
    assert str(ours.value) == str(torchs.value)


def test_product_imports_nothing_from_oracle_or_tests():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "diffsci_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", text, re.M), os.path.join(dirpath, f)


def test_new_sources_are_in_the_build_list():
    import build
    assert "ds_tokens.hip" in build.SOURCES
    assert set(build.SOURCES) == {f for f in os.listdir(build.CSRC) if f.endswith(".hip")}
