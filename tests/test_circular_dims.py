"""Periodic padding per axis, host side: the flag word of ops' circular=, the CircularConv2d / CircularConv3d classes and
extra.convert_conv_to_circular against the fixtures of tools/make_circular_dims_golden.py (the reference's own converter)."""
import copy
import json
import os

import pytest
import torch

from diffsci_amd import _native as N
from diffsci_amd import ops
from diffsci_amd.extra import convert_conv_to_circular, count_conv_layers
from diffsci_amd.models.nets.commonlayers import CircularConv2d, CircularConv3d
from tests.golden_util import GOLDEN_DIR, load

import diffsci_amd.models as M

T, F = True, False


def fixture(tag):
    """(values, converted state_dict) of a case; the weights come from the case named in weights_of."""
    vals, _ = load(tag)
    src, sd, i = vals["weights_of"], {}, 1
    while os.path.exists(os.path.join(GOLDEN_DIR, f"{src}_w{i}.npz")):
        sd.update(load(f"{src}_w{i}")[1])
        i += 1
    return vals, sd


def build(tag):
    """This package's network of a case, from its default (zero-padded) configuration."""
    if tag.startswith("pc3"):
        return M.PUNetG(M.PUNetGConfig(dimension=3, model_channels=16, channel_expansion=[2]))
    if tag == "padm_h":
        return M.ADM(M.ADMConfig(model_channels=16, time_embed_dim=16, output_embed_dim=32, channel_expansion=[1, 2]))
    return M.PUNetG(M.PUNetGConfig(model_channels=16, **(dict(in_out_kernel_size=5) if tag == "pc2_k5" else {})))


def unconverted(sd):
    """The zero-padded network's half of a converted state_dict: the keys without '.conv'."""
    return {k.replace(".conv.", "."): v for k, v in sd.items()}


@pytest.fixture
def no_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(N, "lib", lambda: calls.append(1))
    return calls


# ---------------------------------------------------------------- the flag word
def test_pad_word():
    assert N.DS_PAD_CIRCULAR == 16 and (N.DS_PAD_ZERO_H, N.DS_PAD_ZERO_W, N.DS_PAD_ZERO_D) == (64, 128, 0x10000)
    for nd in (2, 3):
        assert ops.pad_word(True, nd) == ops.pad_word((T,) * nd, nd) == ops.pad_word([T] * nd, nd) == 16
        assert ops.pad_word(False, nd) == ops.pad_word((F,) * nd, nd) == 0
    assert ops.pad_word((T, F), 2) == 16 | 128 and ops.pad_word((F, T), 2) == 16 | 64
    assert ops.pad_word((T, F, F), 3) == 16 | 64 | 128
    assert ops.pad_word((F, T, T), 3) == 16 | 0x10000
    assert ops.pad_word((T, T, F), 3) == 16 | 128
    # free bits only: the load mode (0-3), DS_PAD_CIRCULAR, DS_RES1_UPSAMPLED and the tap offsets stay clear
    assert (64 | 128 | 0x10000) & (15 | 16 | N.DS_RES1_UPSAMPLED | 0xff00) == 0
    for bad, nd in (((T,), 2), ((T, F, T), 2), ((T, F), 3), ((), 3)):
        with pytest.raises(ValueError, match="one flag per spatial axis"):
            ops.pad_word(bad, nd)


def test_wrong_length_raises_before_any_launch(no_launch):
    x, w = torch.zeros(1, 4, 8, 8), torch.zeros(2, 4, 3, 3)
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.conv_direct(x, w, circular=(T, F, F))
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.conv2d(x, w, 2, 3, circular=(T,))
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.conv3d(x[None], w[:, :, None], circular=(T, F))
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.conv3d_mfma(x[None], [None] * 3, circular=(T, F))
    with pytest.raises(ValueError, match="one flag per spatial axis"):
        ops.resblock3d_fused(x[None], None, [None], None, None, [None], None, None, None, 0, circular=(T, F, F, F))
    assert not no_launch


# ---------------------------------------------------------------- the layer classes
@pytest.mark.parametrize("cls,dim", [(CircularConv2d, 2), (CircularConv3d, 3)])
def test_circular_conv_classes(cls, dim, no_launch):
    m = cls(3, 5, 3)
    assert m.circular_dims == set(range(dim)) and m.axes == (T,) * dim                  # None: every axis
    assert (m.in_channels, m.out_channels, m.kernel_size, m.padding) == (3, 5, 3, 1)
    assert list(m.state_dict()) == ["conv.weight", "conv.bias"] and m.weight is m.conv.weight and m.bias is m.conv.bias
    assert tuple(m.conv.weight.shape) == (5, 3) + (3,) * dim and m.conv.padding == (0,) * dim
    assert cls(3, 5, 3, []).axes == (F,) * dim                                          # []: zero padding everywhere
    assert cls(3, 5, 5, [0]).axes == (T,) + (F,) * (dim - 1) and cls(3, 5, 5, (dim - 1,)).axes == (F,) * (dim - 1) + (T,)
    assert cls(3, 5, 1, circular_dims=[0, 0]).circular_dims == {0}
    assert list(cls(3, 5, 7, None, bias=False).state_dict()) == ["conv.weight"]
    assert cls(3, 5, 3, None, 1).conv.stride == (1,) * dim                               # *args go to the torch convolution
    for k in (2, 4):
        with pytest.raises(ValueError, match="odd kernel size"):
            cls(3, 5, k)
    for bad in ([dim], [-1], [0, 7]):
        with pytest.raises(ValueError, match="circular_dims"):
            cls(3, 5, 3, bad)
    for kw in (dict(stride=2), dict(dilation=2), dict(groups=3)):
        with pytest.raises(NotImplementedError, match="stride, dilation and groups"):
            cls(3, 6, 3, **kw)
    with pytest.raises(NotImplementedError, match="kernel sizes up to 7"):
        cls(1, 1, 9)(torch.zeros(1, 1, *([9] * dim)))
    assert not no_launch


# ---------------------------------------------------------------- the converter
@pytest.mark.parametrize("tag", ["pc2_h", "pc2_w", "pc2_k5", "pc3_dh", "pc3_w", "padm_h"])
def test_converter_against_the_reference(tag, no_launch):
    vals, sd = fixture(tag)
    dims = json.loads(vals["circular_dims"])
    net = build(tag)
    net.load_state_dict(unconverted(sd), strict=True)
    keys_before, before = list(net.state_dict()), count_conv_layers(net)
    assert before == json.loads(vals["count_before"])
    conv = convert_conv_to_circular(net, dims)
    assert conv is not net and list(net.state_dict()) == keys_before and count_conv_layers(net) == before   # the original is untouched
    assert not any(net.circular_axes) and not getattr(net, "circular", False)
    assert list(conv.state_dict()) == json.loads(vals["keys"])
    assert count_conv_layers(conv) == json.loads(vals["count_after"])
    nd = len(conv.circular_axes)
    assert conv.circular_axes == tuple(d in dims for d in range(nd)) and conv.circular is True
    for k, v in conv.state_dict().items():
        assert torch.equal(v, sd[k]), k                                                   # the same values under the new keys
    conv.load_state_dict(sd, strict=True)
    layers = [m for m in conv.modules() if isinstance(m, (CircularConv2d, CircularConv3d))]
    assert layers and all(m.circular_dims == set(dims) for m in layers)
    # in place: identity, and a second conversion re-aims the layers instead of nesting them
    again = convert_conv_to_circular(conv, [nd - 1], inplace=True)
    assert again is conv and conv.circular_axes == (F,) * (nd - 1) + (T,)
    assert list(conv.state_dict()) == json.loads(vals["keys"]) and all(m.circular_dims == {nd - 1} for m in layers)
    assert convert_conv_to_circular(conv, [], inplace=True).circular is False and conv.circular_axes == (F,) * nd
    assert not no_launch


def test_converter_drops_packed_weights_and_plans(no_launch):
    net = build("pc2_h")
    mod = M.KarrasModule(net, M.KarrasModuleConfig.from_edm())
    net._packed, net._packed_sig = {"stale": 1}, "sig"
    mod._plans.plans["stale"] = object()
    ws = net._ws
    out = convert_conv_to_circular(mod, [0], inplace=True)
    assert out is mod and net._packed is None and net._packed_sig is None and mod._plans.plans == {} and net._ws is not ws
    assert net.circular_axes == (T, F)
    mod._plans.plans["stale"] = plan = object()
    cp = convert_conv_to_circular(mod, [1])                      # a copy: without the plans, and the original keeps its own
    assert cp is not mod and cp._plans.plans == {} and mod._plans.plans == {"stale": plan}
    assert cp.model.circular_axes == (F, T) and net.circular_axes == (T, F)
    assert not no_launch


def _snapshot(m):
    return [(k, v.clone()) for k, v in m.state_dict().items()], [type(c).__name__ for c in m.modules()]


def _same(m, snap):
    return [type(c).__name__ for c in m.modules()] == snap[1] and all(
        k == k2 and torch.equal(v, v2) for (k, v), (k2, v2) in zip(m.state_dict().items(), snap[0]))


def test_converter_refusals_leave_the_module_alone(no_launch):
    net = build("pc2_h")
    snap = _snapshot(net)
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError, match="circular_dims"):
            convert_conv_to_circular(net, bad, inplace=True)
    vol = build("pc3_w")
    with pytest.raises(ValueError, match="circular_dims"):
        convert_conv_to_circular(vol, [3], inplace=True)
    assert _same(net, snap) and not any(net.circular_axes)
    even = torch.nn.Sequential(torch.nn.Conv2d(2, 2, 3, padding=1), torch.nn.Sequential(torch.nn.Conv2d(2, 2, 4)))
    snap = _snapshot(even)
    with pytest.raises(ValueError, match="CircularConv requires odd kernel size, got 4. This layer cannot be converted."):
        convert_conv_to_circular(even, None, inplace=True)
    assert _same(even, snap)
    assert not no_launch


@pytest.mark.parametrize("name", ["Decoder", "AutoencoderKL", "VAENet", "ConVit", "DiffusionTransformer"])
def test_networks_without_a_periodic_route_are_refused(name, no_launch):
    from diffsci_amd.models.nets import autoencoderldm, convit, dit, vaenet
    cls = dict(Decoder=autoencoderldm.Decoder, AutoencoderKL=autoencoderldm.AutoencoderKL, VAENet=vaenet.VAENet, ConVit=convit.ConVit,
               DiffusionTransformer=dit.DiffusionTransformer)[name]
    m = cls.__new__(cls)                                           # refused by its class, before anything of it is read
    torch.nn.Module.__init__(m)
    holder = torch.nn.Sequential(torch.nn.Conv2d(1, 1, 3), m)
    for target in (m, holder):
        with pytest.raises(NotImplementedError, match=name):
            convert_conv_to_circular(target, [0], inplace=True)
    assert isinstance(holder[0], torch.nn.Conv2d)
    assert not no_launch


def test_magnitude_preserving_network_is_left_alone(no_launch):
    net = M.PUNetG(M.PUNetGConfig(model_channels=16, convolution_type="mp"))
    names = [type(c).__name__ for c in net.modules()]
    out = convert_conv_to_circular(net, [0])
    assert [type(c).__name__ for c in out.modules()] == names and list(out.state_dict()) == list(net.state_dict())
    assert count_conv_layers(out) == dict(Conv2d=0, Conv3d=0, CircularConv2d=0, CircularConv3d=0)
    assert out.circular_axes == (F, F) and out.circular is False
    assert not no_launch


def test_public_adm_block(no_launch):
    from diffsci_amd.models.nets.adm import ADMBaseBlock
    blk = ADMBaseBlock(8, 8, 16)
    before = count_conv_layers(blk)
    out = convert_conv_to_circular(copy.deepcopy(blk), [1], inplace=True)
    assert count_conv_layers(out)["CircularConv2d"] == before["Conv2d"] > 0 and out.circular_axes == (F, T) and out.circular is True
    assert not no_launch
