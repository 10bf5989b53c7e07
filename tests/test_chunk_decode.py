"""Host side of the chunked volume decode (diffsci_amd/extra/chunk_decode.py): the receptive-field dicts and the tiling plan
against what the reference produced (tests/golden/chunk_decode_*.npz), integer for integer; the refusals, raised with a
CPU-resident decoder before anything could launch; the decoder's walk as three stage pieces.  No GPU."""
import inspect
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import chunk_decode_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", cases.TAGS + ("default",))
def test_receptive_field_dicts_equal_the_reference(tag):
    from diffsci_amd.models.nets.vaenet import VAENet, VAENetConfig
    info = cases.load("a" if tag == "default" else tag)[2]
    want = info["rf_default"] if tag == "default" else info["rf"]
    net = VAENet(VAENetConfig() if tag == "default" else cases.config(tag))
    got = dict(encoder=net.encoder.calculate_receptive_field(), decoder=net.decoder.calculate_receptive_field(),
               net=net.calculate_receptive_field())
    assert json.loads(json.dumps(got)) == want                   # through JSON: tuples and lists compare as the fixture stores them
    assert got["net"]["encoder"] == got["encoder"] and got["net"]["decoder"] == got["decoder"]
    if tag == "default":
        assert got["decoder"]["rf_latent"] == float("inf") and got["encoder"]["rf_input"] == float("inf")
        assert got["decoder"]["feasible_chunking"] is False and got["encoder"]["feasible_chunking"] is False
    else:
        assert got["decoder"]["feasible_chunking"] is True and isinstance(got["decoder"]["rf_latent"], int)


def test_attn_type_none_counts_as_no_attention(capsys):
    from diffsci_amd.models.nets.vaenet import VAENet, VAENetConfig
    kw = dict(dimension=2, ch=8, num_groups=4, ch_mult=[1, 2], num_res_blocks=1, resolution=16, attn_resolutions=[8])
    with_attn, without = VAENet(VAENetConfig(**kw)), VAENet(VAENetConfig(attn_type="none", **kw))
    assert with_attn.decoder.calculate_receptive_field()["has_attention"] is True
    dec = without.decoder.calculate_receptive_field()
    assert dec["has_attention"] is False and dec["rf_latent"] == 1 + 2 + 2 * 4 + 2 * 2 * 4 + 2 and dec["rf_after_middle"] == 11
    assert without.encoder.calculate_receptive_field()["rf_input"] == 1 + 2 + 2 * 4 + 2 + 2 * 4 + 2
    for net in (with_attn, without):
        net.print_receptive_field_summary()
    assert "decoder" in capsys.readouterr().out


@pytest.mark.parametrize("tag,i", cases.CASES)
def test_plan_equals_the_reference_plan(tag, i):
    from diffsci_amd.extra import decode_plan, stage_radii_and_scales
    vals, _, info = cases.load(tag)
    cfg = cases.config(tag)
    assert [list(v) for v in stage_radii_and_scales(cfg)] == [info["radii"], info["scales"]]
    chunk, cap, periodic = info["tilings"][i]
    plan = decode_plan(cfg, vals["z"].shape, chunk, cap, periodic)
    want = cases.recorded_plan(tag, i)
    assert len(plan) == len(want)
    for s, (tiles, rows) in enumerate(zip(plan, want)):
        assert [t.row() for t in tiles] == rows.tolist(), f"stage {s}"
    # the destination boxes of a stage partition its buffer
    for tiles, scale in zip(plan, info["scales"]):
        cells = sum((t.dst_stop[0] - t.dst_start[0]) * (t.dst_stop[1] - t.dst_start[1]) * (t.dst_stop[2] - t.dst_start[2]) for t in tiles)
        assert cells == scale ** 3 * vals["z"].shape[2] * vals["z"].shape[3] * vals["z"].shape[4]


def test_plan_arguments_are_in_dhw_order():
    from diffsci_amd.extra import decode_plan
    cfg = cases.config("a")
    # D (the tensor's LAST axis) is the only tiled one: chunk 11 with radius 5 leaves one-cell centres
    plan = decode_plan(cfg, (6, 5, 12), (11, 64, 64), None, False)
    assert len(plan[0]) == 12 and all(t.dst_stop[:2] == (6, 5) and t.dst_stop[2] - t.dst_start[2] == 1 for t in plan[0])
    assert decode_plan(cfg, (1, 2, 6, 5, 12), [11, 64, 64], None, [False] * 3) == plan


def _decoder(**kw):
    from diffsci_amd.models.nets.vaenet import VAEDecoder, VAENetConfig
    base = dict(dimension=3, ch=8, num_groups=4, ch_mult=[1, 2], num_res_blocks=1, z_channels=2, z_dim=2, has_mid_attn=False,
                resolution=16)
    base.update(kw)
    return VAEDecoder(VAENetConfig(**base))


def test_refusals_come_before_any_launch():
    from diffsci_amd.extra import chunk_decode_strategy_b_3d as decode
    z = torch.zeros(1, 2, 6, 5, 12)
    for kw in (dict(has_mid_attn=True), dict(attn_resolutions=[8]), dict(has_mid_attn=True, attn_type="none"),
               dict(attn_resolutions=[8], attn_type="none")):
        with pytest.raises(NotImplementedError, match="NO attention"):
            decode(_decoder(**kw), z, 64)
    with pytest.raises(NotImplementedError, match="dimension=2"):
        decode(_decoder(dimension=2), z, 64)
    dec = _decoder()
    with pytest.raises(NotImplementedError, match="time"):
        decode(dec, z, 64, time=torch.zeros(1))
    for bad in (z[0], torch.zeros(1, 3, 6, 5, 12), "z"):
        with pytest.raises(ValueError, match="z_latent"):
            decode(dec, bad, 64)
    with pytest.raises(ValueError, match="chunk_latent must be int or 3-tuple"):
        decode(dec, z, (64, 64))
    with pytest.raises(ValueError, match="chunk_latent"):
        decode(dec, z, 8.0)
    with pytest.raises(ValueError, match="max_stage_out_chunk"):
        decode(dec, z, 64, max_stage_out_chunk=(4, 4, 4, 4))
    for bad in (1, (True, False), "yes"):
        with pytest.raises(ValueError, match="periodicity"):
            decode(dec, z, 64, periodicity=bad)
    # everything well formed: what is left is that the decoder is not on a HIP device
    dec.train()
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode(dec, z, 64)
    assert dec.training


def test_box_copy_refusals_need_no_device():
    from diffsci_amd import ops
    src, dst = torch.zeros(6, 5, 6, 10), torch.zeros(6, 7, 9, 13)
    with pytest.raises(ValueError, match="fp32"):
        ops.box_copy3d(src.double(), (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="planes"):
        ops.box_copy3d(src[:5], (0, 0, 0), dst, (0, 0, 0), (1, 1, 1))
    for start, size in (((5, 6, 8), (2, 3, 6)), ((-1, 0, 0), (1, 1, 1)), ((0, 9, 0), (1, 1, 1)), ((0, 0, 0), (1, -1, 1))):
        with pytest.raises(ValueError, match="leaves dst"):
            ops.box_copy3d(src, (0, 0, 0), dst, start, size)
    with pytest.raises(ValueError, match="share storage"):
        ops.box_copy3d(dst[:3], (0, 0, 0), dst[3:], (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):          # well formed: only the device is missing
        ops.box_copy3d(src, (-3, 0, 40), dst, (5, 6, 8), (2, 3, 5))


def test_decoder_walk_is_three_stage_pieces():
    from diffsci_amd.models.nets import autoencoderldm as L
    from diffsci_amd.models.nets.vaenet import VAEDecoder
    for cls in (L.Decoder, VAEDecoder):
        for name in ("_stage0", "_up_stage", "_final_stage"):
            assert callable(getattr(cls, name))
        assert "self._walk(" in inspect.getsource(cls.forward)
    assert VAEDecoder._walk is L.Decoder._walk and VAEDecoder._up_stage is L.Decoder._up_stage
    assert "post_quant_conv" in inspect.getsource(VAEDecoder._stage0) and "Decoder._stage0(" in inspect.getsource(VAEDecoder._stage0)
    walk = inspect.getsource(L.Decoder._walk)
    order = [walk.index(piece) for piece in ("self._stage0(", "self._up_stage(", "self._final_stage(")]
    assert order == sorted(order)
    # the tiler calls the same pieces
    from diffsci_amd.extra import chunk_decode
    run = inspect.getsource(chunk_decode._run_stage)
    assert all(piece in run for piece in ("._stage0(", "._up_stage(", "._final_stage("))


def test_module_imports_without_the_native_library_and_without_the_oracle(tmp_path):
    code = ("import sys\n"
            "import diffsci_amd.extra.chunk_decode as m\n"
            "from diffsci_amd import _native\n"
            "assert _native._lib is None\n"
            "assert not any(k == 'oracle' or k.startswith('oracle.') for k in sys.modules)\n"
            "from diffsci_amd.models.nets.vaenet import VAENetConfig\n"
            "cfg = VAENetConfig(ch=8, num_groups=4, ch_mult=[1, 2], num_res_blocks=1, has_mid_attn=False)\n"
            "print(len(m.decode_plan(cfg, (6, 5, 12), 64, 4, True)))\n")
    env = dict(os.environ, DIFFSCI_HIP_LIB=str(tmp_path / "absent.so"))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "3"
    text = open(os.path.join(ROOT, "diffsci_amd", "extra", "chunk_decode.py")).read()
    assert "oracle" not in text
