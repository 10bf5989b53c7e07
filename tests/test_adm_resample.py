"""ADM resampling by any integer factor (image_sample_factor / downsample_factor / upsample_factor / transition_scale_factor):
construction, state_dict layout, refusals and the binding -- host-side only, no GPU needed."""
import pytest
import torch

import diffsci_amd.models as M
from diffsci_amd import _native as N
from diffsci_amd import ops
from diffsci_amd.models.nets import adm


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("f", [1, 3, 4, 5])
def test_blocks_construct_with_any_factor_and_keep_the_layout(f):
    for dim in (2, 3):
        enc = M.nets.ADMEncoderBlock(16, 32, 24, has_downsample=True, has_residual=True, has_attn=True, attn_heads=2,
                                     dimension=dim, downsample_factor=f)
        assert enc.image_sample_factor == f and enc.image_sample == "downsample"
        assert _shapes(enc) == _shapes(M.nets.ADMEncoderBlock(16, 32, 24, has_downsample=True, has_residual=True,
                                                              has_attn=True, attn_heads=2, dimension=dim))
        dec = M.nets.ADMDecoderBlock(16, 32, 24, channels_skip=8, has_upsample=True, has_residual=True, dimension=dim,
                                     upsample_factor=f)
        assert dec.image_sample_factor == f and dec.image_sample == "upsample"
        assert _shapes(dec) == _shapes(M.nets.ADMDecoderBlock(16, 32, 24, channels_skip=8, has_upsample=True,
                                                              has_residual=True, dimension=dim))
        base = M.nets.ADMBaseBlock(16, 32, 24, image_sample="upsample", image_sample_factor=f, dimension=dim)
        assert base.image_sample_factor == f


def test_containers_take_per_layer_factors():
    layer = adm.ADMEncoderLayer(16, 32, 24, 2, downsample_factor=4)
    assert [b.image_sample_factor for b in layer.input_blocks] == [4, 4]
    assert [b.image_sample for b in layer.input_blocks] == [None, "downsample"]
    enc = adm.ADMEncoder(8, 24, [1, 2, 4], downsample_factor=[2, 4])
    assert [lay.input_blocks[-1].image_sample_factor for lay in enc.layers] == [2, 4]
    assert _shapes(enc) == _shapes(adm.ADMEncoder(8, 24, [1, 2, 4]))
    for dt in (1, 2):
        dec = adm.ADMDecoder(8, 24, [4, 2, 1], upsample_factor=[4, 3], decoder_type=dt)
        assert [lay.input_blocks[-1].image_sample_factor for lay in dec.layers] == [4, 3]
        assert _shapes(dec) == _shapes(adm.ADMDecoder(8, 24, [4, 2, 1], decoder_type=dt))


@pytest.mark.parametrize("f", [1, 3, 4])
def test_adm_network_constructs_with_transition_scale_factor(f):
    cfg = M.ADMConfig(model_channels=8, time_embed_dim=8, output_embed_dim=16, transition_scale_factor=f)
    assert cfg.unsupported_reason() is None
    net = M.ADM(cfg)
    ref = M.ADM(M.ADMConfig(model_channels=8, time_embed_dim=8, output_embed_dim=16))
    assert _shapes(net) == _shapes(ref)                   # the factor adds no parameters
    blocks = list(net._blocks())
    assert {b.factor for b in blocks if b.sample in ("down", "up")} == {f}
    assert sum(b.sample == "down" for b in blocks) == sum(b.sample == "up" for b in blocks) == 2
    assert M.ADMConfig.from_description(cfg.export_description()).transition_scale_factor == f


def test_adm_refuses_fields_that_do_not_divide():
    net = M.ADM(M.ADMConfig(model_channels=8, time_embed_dim=8, output_embed_dim=16, transition_scale_factor=3))
    net.check_field_size((2, 1, 54, 54))                  # 54 -> 18 -> 6
    with pytest.raises(ValueError, match="divide by transition_scale_factor"):
        net.check_field_size((2, 1, 54, 48))
    with pytest.raises(ValueError, match=r"\*\* 2 = 9"):
        net.check_field_size((2, 1, 24, 27))
    net2 = M.ADM(M.ADMConfig(model_channels=8, time_embed_dim=8, output_embed_dim=16))
    net2.check_field_size((1, 1, 12, 20))
    with pytest.raises(ValueError, match="divide"):
        net2.check_field_size((1, 1, 10, 16))


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", None])
def test_factor_refusals(bad):
    with pytest.raises((ValueError, NotImplementedError), match="image_sample_factor"):
        M.nets.ADMBaseBlock(16, 32, 24, image_sample="downsample", image_sample_factor=bad)
    with pytest.raises((ValueError, NotImplementedError), match="image_sample_factor"):
        M.nets.ADMEncoderBlock(16, 32, 24, has_downsample=True, downsample_factor=bad)
    with pytest.raises((ValueError, NotImplementedError), match="image_sample_factor"):
        M.nets.ADMDecoderBlock(16, 32, 24, has_upsample=True, upsample_factor=bad)
    cfg = M.ADMConfig(transition_scale_factor=bad)
    assert "transition_scale_factor" in cfg.unsupported_reason()
    with pytest.raises(NotImplementedError, match="transition_scale_factor"):
        M.ADM(cfg)
    for fn in (ops.upsample_f, ops.avgpool_f):           # checked on the host, before any device work
        with pytest.raises(ValueError, match="factor"):
            fn(torch.zeros(1, 1, 4, 4), bad)


def test_integral_values_are_accepted():
    assert M.nets.ADMEncoderBlock(16, 32, 24, has_downsample=True, downsample_factor=3.0).image_sample_factor == 3
    np = pytest.importorskip("numpy")
    assert M.nets.ADMDecoderBlock(16, 32, 24, has_upsample=True, upsample_factor=np.int64(4)).image_sample_factor == 4


def test_pinned_refusals_are_unchanged():
    with pytest.raises(NotImplementedError, match="num_groups=1"):
        M.nets.ADMEncoderBlock(16, 64, 24, num_groups=2, downsample_factor=3)
    with pytest.raises(NotImplementedError, match="attn_heads=2 with attn_type 'default' only"):
        M.nets.ADMEncoderBlock(16, 64, 24, has_attn=True, attn_type="cosine", attn_heads=2, downsample_factor=4)
    with pytest.raises(NotImplementedError, match="num_groups=1"):
        M.ADM(M.ADMConfig(num_groups=2, transition_scale_factor=3))


def test_binding_exports_the_resampling_kernels():
    names = N.exported_symbols()
    for s in ("ds_gnorm1_apply_poolf", "ds_avgpool3d_f", "ds_upsample_f"):
        assert s in names
