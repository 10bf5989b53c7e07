"""Multi-head attention in the ADM blocks (attn_heads > 1, attn_type="default"): construction, state_dict layout and the
refusals -- host-side only, no GPU needed."""
import pytest
import torch

import diffsci_amd.models as M
from diffsci_amd import ops
from diffsci_amd import _native as N
from diffsci_amd.models.nets import adm

# state_dict keys and shapes of the reference's blocks (diffsci/models/nets/adm.py) built with the arguments below,
# recorded from the reference: nn.MultiheadAttention(64, num_heads=4) keeps one packed in-projection whatever the head count
_REF_ENC2D = {  # ADMEncoderBlock(16, 64, 24, has_residual=True, has_attn=True, attn_heads=4)
    'norm1.weight': (16,), 'norm1.bias': (16,), 'norm2.weight': (64,), 'norm2.bias': (64,),
    'conv1.weight': (64, 16, 3, 3), 'conv1.bias': (64,), 'conv2.weight': (64, 64, 3, 3), 'conv2.bias': (64,),
    'embed_linear.weight': (128, 24), 'embed_linear.bias': (128,), 'convresidual.weight': (64, 16, 1, 1),
    'convresidual.bias': (64,), 'attn.mhattn.in_proj_weight': (192, 64), 'attn.mhattn.in_proj_bias': (192,),
    'attn.mhattn.out_proj.weight': (64, 64), 'attn.mhattn.out_proj.bias': (64,)}
_REF_DEC3D = {  # ADMDecoderBlock(16, 64, 24, channels_skip=8, has_residual=True, has_attn=True, has_upsample=True, dimension=3,
                #                 attn_heads=4)
    'norm1.weight': (24,), 'norm1.bias': (24,), 'norm2.weight': (64,), 'norm2.bias': (64,),
    'conv1.weight': (64, 24, 3, 3, 3), 'conv1.bias': (64,), 'conv2.weight': (64, 64, 3, 3, 3), 'conv2.bias': (64,),
    'embed_linear.weight': (128, 24), 'embed_linear.bias': (128,), 'convresidual.weight': (64, 24, 1, 1, 1),
    'convresidual.bias': (64,), 'attn.mhattn.in_proj_weight': (192, 64), 'attn.mhattn.in_proj_bias': (192,),
    'attn.mhattn.out_proj.weight': (64, 64), 'attn.mhattn.out_proj.bias': (64,)}


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_blocks_with_heads_match_the_reference_state_dict():
    enc = M.nets.ADMEncoderBlock(16, 64, 24, has_residual=True, has_attn=True, attn_heads=4)
    assert _shapes(enc) == _REF_ENC2D
    assert enc.attn.mhattn.num_heads == 4 and enc.attn_heads == 4
    dec = M.nets.ADMDecoderBlock(16, 64, 24, channels_skip=8, has_residual=True, has_attn=True, has_upsample=True,
                                 dimension=3, attn_heads=4)
    assert _shapes(dec) == _REF_DEC3D
    # a checkpoint of a 4-head block loads by key name, strictly, into a fresh one
    sd = {k: torch.randn(s) for k, s in _REF_ENC2D.items()}
    r = M.nets.ADMEncoderBlock(16, 64, 24, has_residual=True, has_attn=True, attn_heads=4).load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys


def test_heads_pass_through_the_containers():
    layer = adm.ADMEncoderLayer(16, 32, 24, 2, has_attn=True, attn_heads=8)
    assert [b.attn.mhattn.num_heads for b in layer.input_blocks] == [8, 8]
    mid = adm.ADMMiddleBlock(64, 24, 3, has_attn=[True, False, True], attn_heads=2)
    assert [b.attn.mhattn.num_heads for b in mid.middle_blocks if b.has_attn] == [2, 2]


def test_heads_refusals():
    with pytest.raises(ValueError, match="attn_heads=3 must divide channels_out=64"):
        M.nets.ADMEncoderBlock(16, 64, 24, has_attn=True, attn_heads=3)
    with pytest.raises(ValueError, match="must divide"):
        M.nets.ADMDecoderBlock(16, 64, 24, has_attn=True, attn_heads=0)
    with pytest.raises(NotImplementedError, match="attn_heads=2 with attn_type 'default' only"):
        M.nets.ADMEncoderBlock(16, 64, 24, has_attn=True, attn_type="cosine", attn_heads=2)
    with pytest.raises(NotImplementedError, match="num_groups=1"):
        M.nets.ADMEncoderBlock(16, 64, 24, has_attn=True, num_groups=2, attn_heads=4)
    with pytest.raises(ValueError, match="not a multiple of heads=3"):
        ops.attention(torch.zeros(1, 30, 32), 10, heads=3)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.attention_workspace_floats(1, 10, 32, heads=4)


def test_heads_entry_points_in_the_binding():
    for name in ("ds_attention_h3_heads", "ds_attention_h3_heads_workspace_bytes", "ds_attention_heads_generic"):
        assert name in N.exported_symbols()
    L = N.lib()
    # the images of all (sample, head) rows take as many bytes as single-head images of E; no images off the MFMA widths
    assert L.ds_attention_h3_heads_workspace_bytes(3, 256, 4, 1024) == L.ds_attention_h3_workspace_bytes(3, 256, 1024)
    assert L.ds_attention_h3_heads_workspace_bytes(3, 128, 16, 1024) == 0
    assert L.ds_attention_h3_heads_workspace_bytes(3, 128, 3, 1024) == 0
    assert L.ds_attention_h3_heads_workspace_bytes(3, 128, 2, 1000) == 0
