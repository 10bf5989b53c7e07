"""PUNetG with transition_scale_factor other than 2 (MaxPool(f) down, nearest Upsample(f) up): construction, state_dict layout,
the receptive field, refusals and the binding -- host-side only, no GPU needed."""
import pytest
import torch

import diffsci_amd.models as M
from diffsci_amd import _native as N
from diffsci_amd import ops


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def _cfg(f=2, dim=2, **over):
    kw = dict(model_channels=8, dimension=dim, transition_scale_factor=f)
    kw.update(over)
    return M.PUNetGConfig(**kw)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("f", [1, 3, 4])
def test_constructs_with_any_factor_and_keeps_the_layout(f, dim):
    cfg = _cfg(f, dim)
    assert cfg.unsupported_reason() is None
    net = M.PUNetG(cfg)
    assert net.factor == f
    assert _shapes(net) == _shapes(M.PUNetG(_cfg(2, dim)))          # the factor adds no parameters
    ref = M.PUNetG(_cfg(2, dim))
    assert net.load_state_dict(ref.state_dict()) is not None        # a factor-2 checkpoint loads as it is


@pytest.mark.parametrize("f", [1, 3, 4])
def test_conditional_networks_construct(f):
    net = M.nets.PUNetGCond(_cfg(f, input_channels=3), channel_conditional_items=["a"])
    assert net.factor == f
    assert _shapes(net) == _shapes(M.nets.PUNetGCond(_cfg(2, input_channels=3), channel_conditional_items=["a"]))


@pytest.mark.parametrize("f", [1, 3, 4])
def test_description_round_trip(f):
    net = M.PUNetG(_cfg(f, channel_expansion=[2, 4, 4]))
    d = net.export_description()
    assert d["config"]["transition_scale_factor"] == f
    cfg = M.PUNetGConfig.from_description(d["config"])
    assert cfg.transition_scale_factor == f and cfg.export_description() == d["config"]
    assert _shapes(M.PUNetG(cfg)) == _shapes(net)


@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_receptive_field_uses_the_factor(f, levels):
    net = M.PUNetG(_cfg(f, channel_expansion=[2] * levels, number_resnet_attn_block=1))
    rf = net.calculate_receptive_field()
    assert rf["downsampling_factor"] == f ** levels
    assert rf["config_summary"]["transition_scale_factor"] == f
    assert any(f"maxpool: 1 x (k = {f})" in line for line in rf["trace"])


def test_integral_values_are_accepted():
    assert M.PUNetG(_cfg(3.0)).factor == 3
    np = pytest.importorskip("numpy")
    net = M.PUNetG(_cfg(np.int64(4)))
    assert net.factor == 4 and type(net.factor) is int


@pytest.mark.parametrize("bad", [0, -1, -3, 1.5, 2.5, True, False, "2", None])
def test_factor_refusals(bad):
    cfg = _cfg(bad)
    assert "transition_scale_factor" in cfg.unsupported_reason()
    with pytest.raises(NotImplementedError, match="transition_scale_factor"):
        M.PUNetG(cfg)
    with pytest.raises(NotImplementedError, match="transition_scale_factor"):
        M.PUNetG(_cfg(bad, 3))
    with pytest.raises(ValueError, match="factor"):
        ops.maxpool_f(torch.zeros(1, 1, 4, 4), bad)


def test_other_refusals_keep_their_messages():
    with pytest.raises(NotImplementedError, match="convolution_type"):
        M.PUNetG(_cfg(3, convolution_type="spherical"))
    why = _cfg(0, convolution_type="spherical").unsupported_reason()
    assert "convolution_type" in why and "transition_scale_factor" in why


def test_fields_that_do_not_divide_are_refused():
    net = M.PUNetG(_cfg(3))                                           # two transitions by 3
    net.check_field_size((2, 1, 54, 54))                              # 54 -> 18 -> 6
    net.check_field_size((2, 1, 54, 81))
    with pytest.raises(ValueError, match=r"transition_scale_factor \*\* 2 = 9"):
        net.check_field_size((2, 1, 54, 48))
    with pytest.raises(ValueError, match=r"by 3"):
        net.check_field_size((2, 1, 24, 27))
    vol = M.PUNetG(_cfg(4, 3))
    vol.check_field_size((1, 1, 16, 32, 48))
    with pytest.raises(ValueError, match=r"volume does not divide by transition_scale_factor \*\* 2 = 16"):
        vol.check_field_size((1, 1, 16, 16, 8))
    one = M.PUNetG(_cfg(1))
    one.check_field_size((1, 1, 7, 13))
    # factor 2 keeps its own behaviour for every shape: nothing is refused up front
    M.PUNetG(_cfg(2)).check_field_size((1, 1, 10, 14))
    # the network refuses before it looks at the device (the tensors here live on the CPU)
    with pytest.raises(ValueError, match="divide"):
        net.forward_with_shifts(torch.zeros(1, 1, 27, 30), [])


def test_maxpool_wrapper_checks_on_the_host():
    for shape in ((1, 1, 4), (1, 1, 2, 2, 2, 2)):
        with pytest.raises(ValueError, match="fields"):
            ops.maxpool_f(torch.zeros(shape), 2)


def test_binding_exports_the_max_pool():
    assert "ds_maxpool_f" in N.exported_symbols()
    assert "ds_maxpool_f" in N._PROTOS
