"""LDM AutoencoderKL decoder (diffsci_amd/models/nets/autoencoderldm{2d,3d}.py) on the host: the reference's surface --
constructors, attributes, state_dict keys and shapes, strict loading of its decoder state_dicts, init_from_ckpt of a full
checkpoint -- from the fixtures tools/make_ldm_golden.py recorded, the torch restatement tests/ldm_ref.py pinned against the
reference's own outputs, and the refusals raised before any launch."""
import inspect
import json
import os

import pytest
import torch

from tests import ldm_ref
from tests.golden_util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("a", "a2", "b", "c")
SURFACE_OF = {"2d": "a", "3d": "c"}                 # the fixture that carries each reference module's recorded surface


@pytest.fixture(scope="module")
def nets():
    import diffsci_amd.models.nets as nets
    return nets


def _mod(which):
    import importlib
    return importlib.import_module("diffsci_amd.models.nets.autoencoderldm" + which)


def _surface(which):
    v, _, _ = ldm_ref.load_golden(SURFACE_OF[which])
    return json.loads(v["surface"])


def _keys(module):
    return [[k, list(t.shape)] for k, t in module.state_dict().items()]


@pytest.mark.parametrize("tag", TAGS)
def test_ldm_ref_reproduces_the_reference(tag):
    v, sd, info = ldm_ref.load_golden(tag)
    kw = info["decoder"]
    ref_err = rel_l2(v["out_f32"], v["out_f64"])
    with torch.inference_mode():
        o64 = ldm_ref.decoder({k: t.double() for k, t in sd.items()}, v["z"], **kw)
        o32 = ldm_ref.decoder(sd, v["z"], **kw)
    e64, e32 = rel_l2(o64, v["out_f64"]), rel_l2(o32, v["out_f64"])
    print(f"ldm_{tag}: ldm_ref fp64 vs reference fp64 {e64:.2e}; ldm_ref fp32 vs fp64 {e32:.2e}; reference fp32 vs fp64 {ref_err:.2e}")
    assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o64.shape == v["out_f64"].shape
    assert e64 <= 1e-13
    assert e32 <= ref_err


def test_ldm_ref_autoencoder_decode_reproduces_the_reference():
    v, sd, _ = ldm_ref.load_golden("ae")
    ref_err = rel_l2(v["out_f32"], v["out_f64"])
    with torch.inference_mode():
        o64 = ldm_ref.autoencoder_decode({k: t.double() for k, t in sd.items()}, v["z"])
        o32 = ldm_ref.autoencoder_decode(sd, v["z"])
    assert rel_l2(o64, v["out_f64"]) <= 1e-13
    assert rel_l2(o32, v["out_f64"]) <= ref_err


def test_exported_as_the_reference_exports_them(nets):
    import diffsci_amd.models as M
    a2, a3 = _mod("2d"), _mod("3d")
    for name in ("ddconfig", "ResnetBlock", "AttnBlock", "Upsample", "Decoder", "AutoencoderKL"):
        assert inspect.isclass(getattr(a2, name)) and inspect.isclass(getattr(a3, name))
        assert getattr(a2, name) is not getattr(a3, name)
        assert getattr(nets, name) is getattr(a3, name)            # the 3-D names win the star export
    assert nets.AutoencoderKL is a3.AutoencoderKL is M.AutoencoderKL
    assert nets.autoencoderldm2d is a2 and nets.autoencoderldm3d is a3
    assert inspect.isclass(nets.LDMAutoencoderKLWrapper)


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_constructor_signatures_and_defaults(which):
    mod, ref = _mod(which), _surface(which)["signatures"]
    for cname, want in ref.items():
        got = [[n, p.kind.name, "<required>" if p.default is inspect.Parameter.empty else repr(p.default)]
               for n, p in inspect.signature(getattr(mod, cname).__init__).parameters.items() if n != "self"]
        if cname == "AutoencoderKL":
            # the one stated difference: lossconfig (training only) may be left out here
            assert got[1] == ["lossconfig", "POSITIONAL_OR_KEYWORD", "None"] and want[1][:2] == got[1][:2]
            got, want = got[:1] + got[2:], want[:1] + want[2:]
        assert got == want, cname
    cfg = mod.ddconfig()
    for name, _, default in ref["ddconfig"]:
        assert repr(getattr(cfg, name)) == default


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_block_keys_attributes_and_z_shape(which):
    mod, ref = _mod(which), _surface(which)
    keys = ref["keys"]
    assert _keys(mod.ResnetBlock(in_channels=32, out_channels=64, dropout=0.0, temb_channels=0)) == keys["ResnetBlock"]
    assert _keys(mod.ResnetBlock(in_channels=32, out_channels=64, conv_shortcut=True, dropout=0.0, temb_channels=0)) == keys["ResnetBlockConvShortcut"]
    assert _keys(mod.ResnetBlock(in_channels=32, dropout=0.0)) == keys["ResnetBlockTemb"]
    assert _keys(mod.AttnBlock(64)) == keys["AttnBlock"]
    assert _keys(mod.Upsample(32, True)) == keys["Upsample"] and _keys(mod.Upsample(32, False)) == []
    v, _, info = ldm_ref.load_golden(SURFACE_OF[which])
    vae = mod.AutoencoderKL(mod.ddconfig(**info["ddconfig"]))
    ours = _keys(vae)
    assert ours == [kv for kv in keys["AutoencoderKL"] if kv[0].startswith(("decoder.", "post_quant_conv."))]
    assert {k.split(".")[0] for k, _ in keys["AutoencoderKL"]} == {"encoder", "quant_conv", "decoder", "post_quant_conv"}
    assert list(vae.decoder.z_shape) == ref["z_shape"] and isinstance(vae.decoder.z_shape, tuple)
    blk = mod.ResnetBlock(in_channels=32, out_channels=64, dropout=0.0, temb_channels=0)
    assert (blk.in_channels, blk.out_channels, blk.use_conv_shortcut) == (32, 64, False)
    assert blk.norm1.eps == 1e-6 and blk.norm1.num_groups == 32
    conv = torch.nn.Conv3d if which == "3d" else torch.nn.Conv2d
    assert type(blk.conv1) is conv and type(blk.nin_shortcut) is conv and type(vae.post_quant_conv) is conv


@pytest.mark.parametrize("tag", ("a", "b", "c"))
def test_decoder_keys_shapes_strict_load_and_attributes(tag, capsys):
    v, sd, info = ldm_ref.load_golden(tag)
    net = ldm_ref.build(info)
    assert capsys.readouterr().out == ""                              # nothing is printed at construction
    assert _keys(net) == json.loads(v["keys"])
    r = net.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert all(torch.equal(net.state_dict()[k], sd[k]) for k in sd)
    cfg = info["ddconfig"]
    for name in ("double_z", "z_channels", "resolution", "in_channels", "out_ch", "ch", "ch_mult", "num_res_blocks",
                 "attn_resolutions", "dropout", "has_mid_attn"):
        assert getattr(net, name) == cfg.get(name, getattr(ldm_ref.module_of(info).ddconfig(), name))
    assert net.temb_ch == 0 and net.num_resolutions == len(cfg["ch_mult"])
    assert net.give_pre_end is False and net.tanh_out is info["decoder"].get("tanh_out", False)
    assert net.conv_precision == "fp16x3" and net.fuse_norm is True
    assert hasattr(net.mid, "attn_1") == cfg.get("has_mid_attn", True)
    assert len(net.up) == len(cfg["ch_mult"]) and not hasattr(net.up[0], "upsample") and hasattr(net.up[1], "upsample")


def test_decoder_options():
    a2 = _mod("2d")
    cfg = a2.ddconfig(ch=32, ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[16, 32], resolution=32)
    net = a2.Decoder(cfg, resamp_with_conv=False, give_pre_end=True, attn_type="none", some_ignored_keyword=1)
    assert net.give_pre_end is True and not any(k.startswith("up.1.upsample") for k in net.state_dict())
    assert isinstance(net.mid.attn_1, torch.nn.Identity) and len(net.up[0].attn) == 2 and len(net.up[1].attn) == 2
    net = a2.Decoder(cfg)
    assert isinstance(net.up[0].attn[1], a2.AttnBlock) and isinstance(net.up[1].upsample, a2.Upsample)
    assert net.up[1].upsample.with_conv is True and "up.1.upsample.conv.weight" in net.state_dict()


def test_init_from_ckpt_loads_a_full_reference_checkpoint(tmp_path):
    a2 = _mod("2d")
    v, sd, info = ldm_ref.load_golden("ae")
    full = {}
    for k, shape in _surface("2d")["keys"]["AutoencoderKL"]:
        if k.startswith("post_quant_conv."):
            shape = list(sd[k].shape)                                   # the fixture's embed_dim is 3
        full[k] = sd[k] if k in sd else torch.full(shape, 0.5)
    full["loss.logvar"] = torch.zeros(())
    assert {k.split(".")[0] for k in full} == {"encoder", "loss", "quant_conv", "decoder", "post_quant_conv"}
    path = tmp_path / "ldm.ckpt"
    torch.save({"state_dict": full}, path)
    cfg = a2.ddconfig(**info["ddconfig"])
    vae = a2.AutoencoderKL(cfg, embed_dim=info["embed_dim"], ckpt_path=str(path))
    assert all(torch.equal(t, sd[k]) for k, t in vae.state_dict().items()) and len(vae.state_dict()) == len(sd)
    assert vae.embed_dim == 3 and tuple(vae.post_quant_conv.weight.shape) == (4, 3, 1, 1)
    vae2 = a2.AutoencoderKL(cfg, None, 3, None, [])
    before = vae2.decoder.conv_in.weight.clone()
    vae2.init_from_ckpt(str(path), ignore_keys=["decoder.conv_in"])
    assert torch.equal(vae2.decoder.conv_in.weight, before) and torch.equal(vae2.decoder.conv_out.weight, sd["decoder.conv_out.weight"])


def test_encoder_is_refused(nets):
    a2 = _mod("2d")
    vae = a2.AutoencoderKL(a2.ddconfig(ch=32, ch_mult=[1, 2], num_res_blocks=1))
    assert [n for n, _ in vae.named_children()] == ["decoder", "post_quant_conv"]
    x = torch.zeros(1, 1, 32, 32)
    for call in (lambda: vae.encode(x), lambda: vae(x), lambda: nets.LDMAutoencoderKLWrapper(vae).encode(x),
                 lambda: nets.LDMAutoencoderKLWrapper(vae).encode(x[0], has_batch_dim=False), lambda: nets.LDMAutoencoderKLWrapper(vae)(x)):
        with pytest.raises(NotImplementedError, match=r"encoder.*outside the HIP sampling path.*is_latent_shape=True"):
            call()


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_refusals_before_any_launch(which, monkeypatch):
    from diffsci_amd import _native
    calls = []
    monkeypatch.setattr(_native, "lib", lambda: calls.append(1))
    mod = _mod(which)
    sp = (8,) * (3 if which == "3d" else 2)
    small = dict(ch=32, ch_mult=[1, 2], num_res_blocks=1)
    with pytest.raises(NotImplementedError, match="linear"):
        mod.Decoder(mod.ddconfig(**small), attn_type="linear")
    with pytest.raises(NotImplementedError, match="linear"):
        mod.Decoder(mod.ddconfig(**small), use_linear_attn=True)
    with pytest.raises(ValueError) as ours:
        mod.ResnetBlock(in_channels=48, dropout=0.0, temb_channels=0)
    with pytest.raises(ValueError) as torchs:
        torch.nn.GroupNorm(32, 48)
    assert str(ours.value) == str(torchs.value)
    with pytest.raises(ValueError):
        mod.Decoder(mod.ddconfig(ch=24, ch_mult=[1, 2], num_res_blocks=1))
    blk = mod.ResnetBlock(in_channels=32, dropout=0.0)
    with pytest.raises(NotImplementedError, match="temb"):
        blk(torch.zeros(1, 32, *sp), torch.zeros(1, 512))
    drop = mod.ResnetBlock(in_channels=32, dropout=0.1, temb_channels=0)
    with pytest.raises(NotImplementedError, match=r"dropout.*\.eval\(\)"):
        drop(torch.zeros(1, 32, *sp), None)
    net = mod.Decoder(mod.ddconfig(dropout=0.1, **small))
    with pytest.raises(NotImplementedError, match=r"dropout.*\.eval\(\)"):
        net(torch.zeros(1, 4, *sp))
    net = mod.Decoder(mod.ddconfig(**small))
    vae = mod.AutoencoderKL(mod.ddconfig(**small), embed_dim=3)
    with pytest.raises(ValueError, match=f"{len(sp) + 2}-D"):
        net(torch.zeros(1, 4, *sp[1:]))
    with pytest.raises(ValueError, match=f"{len(sp) + 2}-D"):
        net(torch.zeros(1, 4, 2, *sp))
    with pytest.raises(ValueError, match="expects 4 channels; got 3"):
        net(torch.zeros(1, 3, *sp))
    with pytest.raises(ValueError, match="expects 3 channels; got 4"):
        vae.decode(torch.zeros(1, 4, *sp))
    with pytest.raises(ValueError, match="expects 64 channels"):
        mod.AttnBlock(64)(torch.zeros(1, 32, *sp))
    for call in (lambda: net(torch.zeros(1, 4, *sp)), lambda: vae.decode(torch.zeros(1, 3, *sp)),
                 lambda: drop.eval()(torch.zeros(1, 32, *sp), None), lambda: mod.AttnBlock(32)(torch.zeros(1, 32, *sp)),
                 lambda: mod.Upsample(32, False)(torch.zeros(1, 32, *sp))):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            call()
    net.conv_precision = "fp8"
    with pytest.raises(ValueError, match="conv_precision"):
        net(torch.zeros(1, 4, *sp))
    assert not calls


def test_new_entry_points_are_declared_bound_and_built():
    from diffsci_amd import _native as N
    import build
    header = open(os.path.join(ROOT, "include", "diffsci_hip.h")).read()
    for name in ("ds_groupnorm_stats", "ds_groupnorm_apply", "ds_groupnorm_stats_tiles", "ds_groupnorm_table"):
        assert name in N.exported_symbols()
        assert f"int {name}(" in header
    assert "ds_groupnorm.hip" in build.SOURCES
    assert N.ABI_VERSION == 4
