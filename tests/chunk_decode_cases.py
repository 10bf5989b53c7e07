"""The fixtures of the chunked volume decode (tests/golden/chunk_decode_{a,b}.npz, tools/make_chunk_decode_golden.py), shared by
tests/test_chunk_decode.py and tests/test_gpu_chunk_decode.py."""
import functools
import json

from tests import golden_util

TAGS = ("a", "b")
TILINGS = {"a": 5, "b": 3}
CASES = [(tag, i) for tag in TAGS for i in range(TILINGS[tag])]


@functools.lru_cache(maxsize=None)
def load(tag):
    """-> (values, decoder state_dict, info); info["tilings"][i] = [chunk_latent, max_stage_out_chunk, periodicity]."""
    vals, sd = golden_util.load("chunk_decode_" + tag)
    info = json.loads(vals["info"])
    assert len(info["tilings"]) == TILINGS[tag]
    return vals, sd, info


def config(tag):
    from diffsci_amd.models.nets.vaenet import VAENetConfig
    return VAENetConfig(**load(tag)[2]["config"])


def recorded_plan(tag, i):
    """The reference's plan of tiling i: one [tiles, 18] int tensor per stage."""
    vals, _, info = load(tag)
    return [vals[f"t{i}/plan_s{s}"] for s in range(len(info["radii"]))]
