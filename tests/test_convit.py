"""ConVit (diffsci_amd/models/nets/convit.py) on the host: the reference's surface -- constructors, attributes, state_dict keys
and shapes, strict loading of its checkpoints, the config round trips -- from the fixtures tools/make_convit_golden.py recorded,
the torch restatement tests/convit_ref.py pinned against the reference's own outputs, and every refusal of the network and of
the new op wrappers raised before any launch."""
import inspect
import json
import os

import pytest
import torch

from tests import convit_ref
from tests.golden_util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("a", "b", "c")


@pytest.fixture(scope="module")
def nets():
    import diffsci_amd.models.nets as nets
    return nets


def build(nets, kw, **over):
    kw = dict(kw, **over)
    return nets.ConVit(nets.ConVitConfig(**kw), conditional_embedding=torch.nn.Linear(1, kw.get("embed_dim", 64)))


def ref_kwargs(kw):
    return dict(attn_compression_factor=kw.get("attn_compression_factor", 2), relative_positioning=kw.get("relative_positioning", False))


def test_exported_like_the_reference(nets):
    from diffsci_amd.models.nets import convit
    assert nets.ConVit is convit.ConVit and nets.ConVitBlock is convit.ConVitBlock and nets.ConVitConfig is convit.ConVitConfig
    for name in ("ChannelRMSNorm", "MultiheadAttention", "LearnedRoPE", "ConvSwiGLU", "SwiGLU", "Upsample", "Downsample"):
        assert inspect.isclass(getattr(convit, name)), name


def _signature(fn):
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name != "self":
            out.append([name, p.kind.name, "<required>" if p.default is inspect.Parameter.empty else p.default])
    return out


def test_constructor_signatures_and_defaults(nets):
    v, _, _ = convit_ref.load_golden("a")
    ref = json.loads(v["signature"])
    for cname in ("ConVit", "ConVitBlock", "ConVitConfig"):
        assert _signature(getattr(nets, cname).__init__) == ref[cname], cname


def test_the_constructor_quirk_is_kept(nets):
    """convit.py:715: isinstance(conditional_embedding, None) -- the reference cannot be built without a conditional embedding."""
    with pytest.raises(TypeError, match="isinstance"):
        nets.ConVit(nets.ConVitConfig())
    with pytest.raises(TypeError, match="isinstance"):
        nets.ConVit(nets.ConVitConfig(has_time_embedding=True), conditional_embedding=torch.nn.Linear(1, 64))
    with pytest.raises(AssertionError):
        nets.ConVit(nets.ConVitConfig(has_conditional_embedding=True))


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_shapes_and_strict_load(nets, tag):
    v, sd, kw = convit_ref.load_golden(tag)
    net = build(nets, kw)
    ours = net.state_dict()
    assert [[k, list(t.shape)] for k, t in ours.items()] == json.loads(v["keys"])
    assert any(k.endswith("attention.scale") for k in ours) and any(k.endswith("fusion_weight") for k in ours)
    net.load_state_dict(sd, strict=True)
    for k, t in net.state_dict().items():
        assert torch.equal(t, sd[k]), k
    desc = nets.ConVitConfig(**kw).export_description()                  # the reference copies the config onto the network
    for name, value in desc.items():
        if name not in ("has_time_embedding", "out_channels"):
            assert getattr(net, name) == value, name
    assert net.out_channels == desc["in_channels"] and net.has_embedding and net.config.has_time_embedding


def test_two_layers_have_60_entries(nets):
    _, _, kw = convit_ref.load_golden("a")
    assert len(build(nets, kw).state_dict()) == 60


def test_config_round_trips(nets, tmp_path):
    import yaml
    cfg = nets.ConVitConfig(embed_dim=128, num_heads=4, kernel_size_conv=3, relative_positioning=True, has_time_embedding=True)
    d = cfg.export_description()
    assert list(d) == ["in_channels", "embed_dim", "num_pos_dims", "out_channels", "num_layers", "num_heads", "ffn_expansion_factor",
                       "attn_compression_factor", "rope_freq", "with_conv_on_upsample", "with_conv_on_downsample", "kernel_size_conv",
                       "kernel_size_depthwise", "kernel_size_in_out", "has_time_embedding", "has_conditional_embedding",
                       "fourier_projection_scale", "relative_positioning", "linear_attention", "input_batch_norm", "condition_dropout"]
    assert nets.ConVitConfig.from_description(d).export_description() == d
    path = tmp_path / "convit.yaml"
    path.write_text(yaml.safe_dump(d))
    again = nets.ConVitConfig.from_config_file(path)
    assert again.export_description() == d and again.has_embedding and not nets.ConVitConfig().has_embedding
    assert nets.ConVitConfig.from_config_file(str(path)).embed_dim == 128


def test_engine_protocol_attributes(nets):
    from diffsci_amd.models.karras.engine import MODEL_SWITCHES, model_signature
    net = build(nets, dict(num_layers=1, has_time_embedding=True, has_conditional_embedding=True))
    assert net.conv_precision == "fp16x3" and net.auto_precision is True and net.capturable is True
    for name in ("check_input", "embed_condition", "embed_time", "time_shifts", "forward_with_shifts", "forward", "forward_unguarded"):
        assert callable(getattr(net, name))
    assert "conv_precision" in MODEL_SWITCHES
    a = model_signature(net)
    net.conv_precision = "fp32"
    assert model_signature(net) != a


def test_qkv_and_out_weights_put_head_h_on_its_rows(nets):
    """Row h*dh + dv of the q third is q_proj_tensor[:, dv, h]; W_out[d, h*dh + dv] = out_proj_tensor[d, dv, h]."""
    from diffsci_amd.models.nets.convit import MultiheadAttention
    torch.manual_seed(3)
    att = MultiheadAttention(embed_dim=16, num_heads=4, num_pos_dims=2)
    E, dh, H = 16, 4, 4
    wq, wo = att.qkv_weight().reshape(3 * E, E), att.out_weight().reshape(E, E)
    x = torch.randn(5, E)
    for name, third in (("q", 0), ("k", 1), ("v", 2)):
        want = torch.einsum("bd,dvh->bvh", x, getattr(att, name + "_proj_tensor").detach())          # convit.py:473-478
        got = (x @ wq[third * E:(third + 1) * E].T).reshape(5, H, dh).permute(0, 2, 1)
        assert torch.allclose(got, want, atol=1e-6)
    o = torch.randn(5, dh, H)
    want = torch.einsum("bvh,dvh->bd", o, att.out_proj_tensor.detach())                               # convit.py:530-531
    assert torch.allclose(o.permute(0, 2, 1).reshape(5, E) @ wo.T, want, atol=1e-6)


def test_rope_table_is_the_reference_angles(nets):
    from diffsci_amd.models.nets.convit import LearnedRoPE
    torch.manual_seed(4)
    for relative in (False, True):
        layer = LearnedRoPE(embed_dim=8, num_pos_dims=2, relative_positioning=relative)
        cs = layer.cos_sin((3, 5))
        assert cs.shape == (15, 4, 2) and cs.dtype == torch.float32
        x = torch.randn(2, 3, 5, 8, dtype=torch.float64)
        want = convit_ref.rope(x, layer.angles.detach().double(), relative)
        pairs = x.reshape(2, 15, 4, 2)
        c, s = cs[..., 0].double(), cs[..., 1].double()
        got = torch.stack([pairs[..., 0] * c - pairs[..., 1] * s, pairs[..., 0] * s + pairs[..., 1] * c], dim=-1).reshape(2, 3, 5, 8)
        assert float((got - want).abs().max()) < 1e-6


@pytest.mark.parametrize("tag", TAGS)
def test_convit_ref_reproduces_the_reference(tag):
    v, sd, kw = convit_ref.load_golden(tag)
    sd64 = {k: t.double() for k, t in sd.items()}
    for y, suffix in ((v["y"], ""), (None, "_nocond")):
        f32, f64 = v[f"out{suffix}_f32"], v[f"out{suffix}_f64"]
        ref_err = rel_l2(f32, f64)
        with torch.inference_mode():
            o64 = convit_ref.convit_forward(sd64, v["x"], v["t"], y, **ref_kwargs(kw))
            o32 = convit_ref.convit_forward(sd, v["x"], v["t"], y, **ref_kwargs(kw))
        e64, e32 = rel_l2(o64, f64), rel_l2(o32, f64)
        print(f"convit_{tag}{suffix}: convit_ref fp64 vs reference fp64 {e64:.2e}; convit_ref fp32 vs fp64 {e32:.2e}; "
              f"reference fp32 vs fp64 {ref_err:.2e}")
        assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o64.shape == f64.shape
        assert e64 <= 1e-12
        assert e32 <= ref_err


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture
def no_launch(monkeypatch):
    """_native.lib replaced by a recorder: whatever reaches the library is a launch the refusal came too late for."""
    from diffsci_amd import _native
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    yield calls
    assert not calls


def test_constructor_refusals(nets, no_launch):
    base = dict(num_layers=1, has_time_embedding=True, has_conditional_embedding=True)
    for over, exc, match in (
            (dict(linear_attention=True), NotImplementedError, "linear_attention"),
            (dict(with_conv_on_upsample=True), NotImplementedError, "with_conv_on_upsample"),
            (dict(with_conv_on_downsample=True), NotImplementedError, "with_conv_on_downsample"),
            (dict(num_pos_dims=3), NotImplementedError, "num_pos_dims"),
            (dict(num_pos_dims=1), NotImplementedError, "num_pos_dims"),
            (dict(input_batch_norm=True), NotImplementedError, "input_batch_norm"),
            (dict(kernel_size_conv=2), NotImplementedError, "kernel_size_conv"),
            (dict(kernel_size_in_out=4), NotImplementedError, "kernel_size_in_out"),
            (dict(kernel_size_depthwise=2), NotImplementedError, "kernel_size_depthwise"),
            (dict(embed_dim=64, num_heads=3), ValueError, "num_heads"),
            (dict(embed_dim=24, num_heads=8), ValueError, "head width"),
    ):
        with pytest.raises(exc, match=match):
            build(nets, base, **over)
    with pytest.raises(NotImplementedError, match="linear_attention"):
        nets.ConVitBlock(64, 2, linear_attention=True)
    with pytest.raises(NotImplementedError, match="num_pos_dims"):
        nets.ConVitBlock(64, 3)


def test_forward_refusals_before_any_launch(nets, no_launch):
    net = build(nets, dict(num_layers=1, has_time_embedding=True, has_conditional_embedding=True, attn_compression_factor=4)).eval()
    t, y = torch.zeros(2), torch.zeros(2, 1)
    with pytest.raises(ValueError, match=r"30x32.*attn_compression_factor=4"):
        net(torch.zeros(2, 1, 30, 32), t)
    with pytest.raises(ValueError, match=r"32x18.*attn_compression_factor=4"):
        net(torch.zeros(2, 1, 32, 18), t, y)
    with pytest.raises(ValueError, match=r"in_channels=1.*got 3"):
        net(torch.zeros(2, 3, 32, 32), t)
    with pytest.raises(ValueError, match="3-D"):
        net(torch.zeros(1, 32, 32), t)
    with pytest.raises(ValueError, match="5-D"):
        net.forward_with_shifts(torch.zeros(2, 1, 1, 32, 32), [None])
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        net(torch.zeros(2, 1, 32, 32), t)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        net(torch.zeros(2, 1, 32, 32))
    net.train()
    with pytest.raises(NotImplementedError, match="condition_dropout"):
        net(torch.zeros(2, 1, 32, 32), t, y)
    net.eval()


def test_unknown_conv_precision_is_refused(nets, no_launch, monkeypatch):
    from diffsci_amd import ops
    monkeypatch.setattr(ops, "_off_device", lambda t: None)              # the tensors pass for device tensors: no GPU on this host
    net = build(nets, dict(num_layers=1, has_time_embedding=True, has_conditional_embedding=True)).eval()
    net.conv_precision = "fp8"
    with pytest.raises(ValueError, match="conv_precision 'fp8'"):
        net.forward_with_shifts(torch.zeros(2, 1, 32, 32), None)


def test_op_refusals_before_any_launch(no_launch, monkeypatch):
    """Wrong dtype, wrong shape, a non-contiguous tensor, a forbidden alias, a table that is too small -- on tensors that pass for
    device tensors (the device test is replaced: this host has no GPU), with the library replaced by the recorder."""
    from diffsci_amd import ops
    z = torch.zeros
    cpu = z(2, 8, 4, 4)
    for call in (lambda: ops.channel_rmsnorm(cpu, z(8)), lambda: ops.rope2d(z(2, 24, 16), 8, 2, z(16, 2, 2)),
                 lambda: ops.upsample_bilinear(cpu, 2), lambda: ops.depthwise_conv_silu(cpu, z(8, 1, 3, 3), z(8)),
                 lambda: ops.swiglu(cpu), lambda: ops.convit_blend(cpu, cpu.clone(), cpu.clone(), z(1))):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            call()
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    x = z(2, 8, 4, 4)
    nc = z(2, 8, 4, 8)[..., ::2]
    i32 = z(2, dtype=torch.int32)
    # channel_rmsnorm
    for bad, exc in ((lambda: ops.channel_rmsnorm(x.double(), z(8)), TypeError), (lambda: ops.channel_rmsnorm(z(2, 8, 16), z(8)), ValueError),
                     (lambda: ops.channel_rmsnorm(x, z(7)), ValueError), (lambda: ops.channel_rmsnorm(nc, z(8)), ValueError),
                     (lambda: ops.channel_rmsnorm(x, z(8), out=x), ValueError), (lambda: ops.channel_rmsnorm(x, z(8), pool=2, out=z(2, 8, 4, 4)), ValueError),
                     (lambda: ops.channel_rmsnorm(x, z(8), pool=8), ValueError), (lambda: ops.channel_rmsnorm(x, z(8), pool=0), ValueError),
                     (lambda: ops.channel_rmsnorm(x, z(8), mod=z(5, 8), row=5), ValueError),          # a table that is too small
                     (lambda: ops.channel_rmsnorm(x, z(8), mod=z(3, 8)), ValueError), (lambda: ops.channel_rmsnorm(x, z(8), mod=z(2, 16)), ValueError),
                     (lambda: ops.channel_rmsnorm(x, z(8), out_amax=z(3, dtype=torch.int32)), TypeError),
                     (lambda: ops.channel_rmsnorm(x, z(8), out_amax=z(2)), TypeError)):
        with pytest.raises(exc):
            bad()
    # rope2d
    qkv = z(2, 24, 16)
    for bad, exc in ((lambda: ops.rope2d(qkv.double(), 8, 2, z(16, 2, 2)), TypeError), (lambda: ops.rope2d(z(2, 20, 16), 8, 2, z(16, 2, 2)), ValueError),
                     (lambda: ops.rope2d(qkv, 8, 3, z(16, 2, 2)), ValueError), (lambda: ops.rope2d(z(2, 18, 16), 6, 2, z(16, 1, 2)), ValueError),
                     (lambda: ops.rope2d(qkv, 8, 2, z(15, 2, 2)), ValueError),                         # a table that is too small
                     (lambda: ops.rope2d(qkv, 8, 2, z(16, 4, 2)), ValueError), (lambda: ops.rope2d(z(2, 24, 32)[..., ::2], 8, 2, z(16, 2, 2)), ValueError),
                     (lambda: ops.rope2d(qkv, 8, 2, z(16, 2, 2), out_amax=i32), TypeError)):
        with pytest.raises(exc):
            bad()
    # upsample_bilinear
    for bad, exc in ((lambda: ops.upsample_bilinear(x.double(), 2), TypeError), (lambda: ops.upsample_bilinear(z(2, 8, 16), 2), ValueError),
                     (lambda: ops.upsample_bilinear(x, 0), ValueError), (lambda: ops.upsample_bilinear(x, 1.5), ValueError),
                     (lambda: ops.upsample_bilinear(nc, 2), ValueError), (lambda: ops.upsample_bilinear(x, 2, out=z(2, 8, 4, 4)), ValueError),
                     (lambda: ops.upsample_bilinear(x, 1, out=x), ValueError)):
        with pytest.raises(exc):
            bad()
    # depthwise_conv_silu
    w = z(8, 1, 3, 3)
    for bad, exc in ((lambda: ops.depthwise_conv_silu(x.double(), w, z(8)), TypeError), (lambda: ops.depthwise_conv_silu(z(2, 8, 16), w, z(8)), ValueError),
                     (lambda: ops.depthwise_conv_silu(x, z(8, 8, 3, 3), z(8)), ValueError), (lambda: ops.depthwise_conv_silu(x, z(4, 1, 3, 3), z(8)), ValueError),
                     (lambda: ops.depthwise_conv_silu(x, z(8, 1, 2, 2), z(8)), NotImplementedError),
                     (lambda: ops.depthwise_conv_silu(x, z(8, 1, 9, 9), z(8)), NotImplementedError),
                     (lambda: ops.depthwise_conv_silu(x, w, z(7)), ValueError), (lambda: ops.depthwise_conv_silu(nc, w, z(8)), ValueError),
                     (lambda: ops.depthwise_conv_silu(x, w, z(8), out=x), ValueError), (lambda: ops.depthwise_conv_silu(x, w, z(8), out=z(2, 8, 4, 5)), ValueError),
                     (lambda: ops.depthwise_conv_silu(x, w, z(8), out_amax=z(1, dtype=torch.int32)), TypeError)):
        with pytest.raises(exc):
            bad()
    # swiglu
    for bad, exc in ((lambda: ops.swiglu(x.double()), TypeError), (lambda: ops.swiglu(z(2, 7, 4, 4)), ValueError), (lambda: ops.swiglu(z(8)), ValueError),
                     (lambda: ops.swiglu(nc), ValueError), (lambda: ops.swiglu(x, out=x.view(-1)[:64].view(2, 4, 4, 2)), ValueError),
                     (lambda: ops.swiglu(x, out=z(2, 8, 4, 4)), ValueError), (lambda: ops.swiglu(x, out_amax=z(3, dtype=torch.int32)), TypeError)):
        with pytest.raises(exc):
            bad()
    # convit_blend
    u, xc, x0, s = z(2, 8, 4, 4), z(2, 8, 4, 4), z(2, 8, 4, 4), z(1)
    for bad, exc in ((lambda: ops.convit_blend(u.double(), xc, x0, s), TypeError), (lambda: ops.convit_blend(u, z(2, 8, 4, 5), x0, s), ValueError),
                     (lambda: ops.convit_blend(u, xc, z(2, 8, 16), s), ValueError), (lambda: ops.convit_blend(u, xc, x0, z(2)), ValueError),
                     (lambda: ops.convit_blend(u, xc, x0, 0.5), TypeError), (lambda: ops.convit_blend(u, xc, x0, s, out=u), ValueError),
                     (lambda: ops.convit_blend(u, xc, x0, s, out=xc), ValueError), (lambda: ops.convit_blend(nc, xc, x0, s), ValueError),
                     (lambda: ops.convit_blend(u, xc, x0, s, out=x0.view(-1)[16:].view(-1)), ValueError),
                     (lambda: ops.convit_blend(u, xc, x0, s, out=z(2, 8, 4, 5)), ValueError)):
        with pytest.raises(exc):
            bad()


def test_new_source_is_in_the_build_list_and_closes_with_a_flags_word():
    import ctypes

    import build
    from diffsci_amd import _native
    assert "ds_convit.hip" in build.SOURCES
    for name in ("ds_channel_rmsnorm", "ds_rope2d", "ds_upsample_bilinear", "ds_depthwise_conv_silu", "ds_swiglu", "ds_convit_blend"):
        res, args = _native._PROTOS[name]
        assert res is ctypes.c_int and args[-2] is ctypes.c_void_p and args[-1] is ctypes.c_int, name
