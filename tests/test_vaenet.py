"""VAENet (diffsci_amd/models/nets/vaenet.py) on the host: the reference's surface -- constructors, defaults, state_dict keys and
shapes, strict loading of its state_dicts -- from the fixtures tools/make_vaenet_golden.py recorded, the torch restatement
tests/vaenet_ref.py pinned against the reference's own outputs, area x2 = nearest x2, and the refusals raised before any launch."""
import inspect
import json

import pytest
import torch
import torch.nn.functional as F

from tests import vaenet_ref
from tests.golden_util import rel_l2

FULL = ("a", "b", "c")                     # fixtures with weights, moments, a draw and a decode
ENC_ONLY = ("a2", "c2")


def _vn():
    from diffsci_amd.models.nets import vaenet
    return vaenet


def _kw(info):
    c = info["config"]
    kw = dict(G=c.get("num_groups", 32), flash=c.get("use_flash_attention", True))
    return kw, dict(kw, tanh_out=c.get("tanh_out", False))


@pytest.mark.parametrize("tag", FULL + ENC_ONLY)
def test_vaenet_ref_reproduces_the_reference(tag):
    v, sd, info = vaenet_ref.load_golden(tag)
    ekw, dkw = _kw(info)
    enc, dec = vaenet_ref.sub(sd, "encoder."), vaenet_ref.sub(sd, "decoder.")
    d = lambda s: {k: t.double() for k, t in s.items()}  # noqa: E731
    with torch.inference_mode():
        m64, m32 = vaenet_ref.encoder(d(enc), v["x"], **ekw), vaenet_ref.encoder(enc, v["x"], **ekw)
        z64, z32 = vaenet_ref.posterior(m64, v["eps"]), vaenet_ref.posterior(m32, v["eps"])
    ref_err = rel_l2(v["moments_f32"], v["moments_f64"])
    e64, e32 = rel_l2(m64, v["moments_f64"]), rel_l2(m32, v["moments_f64"])
    print(f"vaenet_{tag}: restated moments fp64 {e64:.2e}, fp32 {e32:.2e}; reference fp32 vs fp64 {ref_err:.2e}")
    assert m64.dtype == torch.float64 and m32.dtype == torch.float32 and m64.shape == v["moments_f64"].shape
    assert e64 <= 1e-13 and e32 <= ref_err
    assert rel_l2(z64, v["z_f64"]) <= 1e-13 and rel_l2(z32, v["z_f64"]) <= rel_l2(v["z_f32"], v["z_f64"])
    if tag in FULL:
        with torch.inference_mode():
            o64, o32 = vaenet_ref.decoder(d(dec), v["zin"], **dkw), vaenet_ref.decoder(dec, v["zin"], **dkw)
        ref_err = rel_l2(v["dec_f32"], v["dec_f64"])
        e64, e32 = rel_l2(o64, v["dec_f64"]), rel_l2(o32, v["dec_f64"])
        print(f"vaenet_{tag}: restated decode fp64 {e64:.2e}, fp32 {e32:.2e}; reference fp32 vs fp64 {ref_err:.2e}")
        assert o64.shape == v["dec_f64"].shape and e64 <= 1e-13 and e32 <= ref_err


@pytest.mark.parametrize("tag", FULL)
def test_keys_shapes_and_strict_loading(tag, capsys):
    v, sd, info = vaenet_ref.load_golden(tag)
    net = vaenet_ref.build(info)
    assert capsys.readouterr().out == ""                       # nothing is printed at construction
    assert [[k, list(t.shape)] for k, t in net.state_dict().items()] == json.loads(v["keys"])
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [n for n, _ in net.named_children()] == ["encoder", "decoder"]
    assert "encoder.quant_conv.conv.weight" in sd and "decoder.post_quant_conv.conv.weight" in sd
    assert "encoder.conv_in.conv.weight" in sd
    if info["config"].get("resamp_with_conv", True):
        assert "encoder.down.0.downsample.conv.weight" in sd              # the plain convolution
    assert net.export_description() == json.loads(v["description"])
    cfg = _vn().VAENetConfig.from_description(net.config.export_description())
    assert cfg.export_description() == net.config.export_description()


def test_signatures_and_defaults_equal_the_recorded_ones():
    v, _, _ = vaenet_ref.load_golden("a")
    vn = _vn()
    for name, want in json.loads(v["signatures"]).items():
        got = [[n, p.kind.name, "<required>" if p.default is inspect.Parameter.empty else repr(p.default)]
               for n, p in inspect.signature(getattr(vn, name).__init__).parameters.items() if n != "self"]
        assert got == want, name


def test_config_file_round_trip(tmp_path):
    import yaml
    vn = _vn()
    cfg = vn.VAENetConfig(dimension=2, ch=16, ch_mult=[1, 2], num_groups=8, attn_resolutions=[8])
    path = tmp_path / "vae.yaml"
    path.write_text(yaml.safe_dump(cfg.export_description()))
    assert vn.VAENetConfig.from_config_file(path).export_description() == cfg.export_description()
    assert vn.VAENetConfig.from_config_file(str(path)).num_resolutions == 2


def test_public_names():
    import diffsci_amd.models.nets as nets
    vn = _vn()
    assert nets.VAENet is vn.VAENet and nets.VAENetConfig is vn.VAENetConfig


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 3, 4, 5)])
def test_area_x2_is_nearest_x2(shape):
    torch.manual_seed(3)
    x = torch.randn(*shape)
    assert torch.equal(F.interpolate(x, scale_factor=2.0, mode="area"), F.interpolate(x, scale_factor=2.0, mode="nearest"))


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals_before_any_launch(dim, monkeypatch):
    from diffsci_amd import _native
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    vn = _vn()
    small = dict(dimension=dim, ch=32, ch_mult=[1, 2], num_res_blocks=1, resolution=8)
    sp = (8,) * dim
    with pytest.raises(NotImplementedError, match="dimension=1"):
        vn.VAENet(vn.VAENetConfig(dimension=1))
    with pytest.raises(NotImplementedError, match="with_time_emb"):
        vn.VAENet(vn.VAENetConfig(with_time_emb=True, **small))
    with pytest.raises(NotImplementedError, match="minimal_rf_mode"):
        vn.VAENet(vn.VAENetConfig(minimal_rf_mode=True, **small))
    with pytest.raises(NotImplementedError, match="linear"):
        vn.VAENet(vn.VAENetConfig(attn_type="linear", **small))
    for cls in (vn.VAEEncoder, vn.VAEDecoder):
        with pytest.raises(NotImplementedError, match="with_time_emb"):
            cls(vn.VAENetConfig(with_time_emb=True, **small))
    with pytest.raises(ValueError) as ours:
        vn.ResnetBlock(dimension=dim, in_channels=48, dropout=0.0)
    with pytest.raises(ValueError) as torchs:
        torch.nn.GroupNorm(32, 48)
    assert str(ours.value) == str(torchs.value)
    with pytest.raises(ValueError):
        vn.VAENet(vn.VAENetConfig(dimension=dim, ch=24, ch_mult=[1, 2]))
    vn.VAENet(vn.VAENetConfig(dimension=dim, ch=24, ch_mult=[1, 2], num_groups=8, num_res_blocks=1))      # 8 divides 24 and 48
    net = vn.VAENet(vn.VAENetConfig(**small)).eval()
    with pytest.raises(NotImplementedError, match="time"):
        net.encode(torch.zeros(1, 1, *sp), time=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="time"):
        net.decode(torch.zeros(1, 4, *(4,) * dim), time=torch.zeros(1))
    drop = vn.VAENet(vn.VAENetConfig(dropout=0.1, **small))
    with pytest.raises(NotImplementedError, match=r"dropout.*\.eval\(\)"):
        drop.encode(torch.zeros(1, 1, *sp))
    with pytest.raises(NotImplementedError, match=r"dropout.*\.eval\(\)"):
        drop.decode(torch.zeros(1, 4, *(4,) * dim))
    blk = vn.ResnetBlock(dimension=dim, in_channels=32, dropout=0.1)
    with pytest.raises(NotImplementedError, match=r"dropout.*\.eval\(\)"):
        blk(torch.zeros(1, 32, *sp))
    with pytest.raises(NotImplementedError, match="temb"):
        blk.eval()(torch.zeros(1, 32, *sp), torch.zeros(1, 128))
    with pytest.raises(ValueError, match=f"{dim + 2}-D"):
        net.encode(torch.zeros(1, 1, *sp[1:]))
    with pytest.raises(ValueError, match=f"{dim + 2}-D"):
        net.decode(torch.zeros(1, 4, 2, *sp))
    with pytest.raises(ValueError, match="expects 1 channels; got 3"):
        net.encode(torch.zeros(1, 3, *sp))
    with pytest.raises(ValueError, match="expects 4 channels; got 3"):
        net.decode(torch.zeros(1, 3, *sp))
    with pytest.raises(ValueError, match="sides of at least 2"):
        net.encode(torch.zeros(1, 1, 1, *sp[1:]))
    with pytest.raises(ValueError, match="sides of at least 2"):
        vn.Downsample(dim, 32, True)(torch.zeros(1, 32, *sp[1:], 1))
    with pytest.raises(ValueError, match="sides of at least 2"):
        vn.Downsample(dim, 32, False)(torch.zeros(1, 32, 1, *sp[1:]))
    three = vn.VAENet(vn.VAENetConfig(dimension=dim, ch=32, ch_mult=[1, 1, 1], num_res_blocks=1)).eval()
    with pytest.raises(ValueError, match="sides of at least 2"):
        three.encode(torch.zeros(1, 1, *(3,) * dim))                      # 3 -> 1 -> a Downsample with a side of 1
    for call in (lambda: net.encode(torch.zeros(1, 1, *sp)), lambda: net.decode(torch.zeros(1, 4, *sp)),
                 lambda: net(torch.zeros(1, 1, *sp)), lambda: vn.Downsample(dim, 32, True)(torch.zeros(1, 32, *sp)),
                 lambda: vn.AttnBlock(dim, 32)(torch.zeros(1, 32, *sp)), lambda: vn.Upsample(dim, 32, True)(torch.zeros(1, 32, *sp))):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            call()
    net.conv_precision = "fp8"
    with pytest.raises(ValueError, match="conv_precision"):
        net.decode(torch.zeros(1, 4, *sp))
    assert calls == []


def test_ops_refuse_before_any_launch(monkeypatch):
    from diffsci_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.posterior_sample(torch.zeros(1, 4, 3, 3))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ops.pack_conv_s2(torch.zeros(8, 8, 3, 3))
    assert calls == []
