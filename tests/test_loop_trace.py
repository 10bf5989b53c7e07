"""The sampler loops decide what a run launches, with which buffers and scalars, in which order; for the runs of
tests/loop_trace.py -- Karras tables through engine.Loop, interpolant tables through siloop.SILoop, DDPM / DDIM tables through
steploop.DDPMLoop -- they must hand the library exactly what their parent handed it: tests/golden/loop_trace.json, recorded from
the parent commit's diffsci_amd/ by tools/make_loop_trace_golden.py.  Host only: the library is replaced by a recorder and no
kernel runs, so equal launches, arguments and Philox state mean the device sees the same work."""
import json
import os

import pytest
import torch

from . import loop_trace
from .golden_util import cpu_vendor

_traces = {}


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(os.path.dirname(__file__), "golden", "loop_trace.json")) as f:
        return json.load(f)


def trace(case):
    if case not in _traces:
        _traces[case] = json.loads(json.dumps(loop_trace.trace_of(case)))
    return _traces[case]


def test_case_table_and_golden_have_the_same_keys(gold):
    assert set(gold["cases"]) == set(loop_trace.CASES)


def same(got, want, exact):
    """Equal -- on a host whose torch CPU kernels are the golden's (golden_util.same_cpu_arithmetic's test).  Elsewhere exp,
    log, cos and pow differ in the last place between vectorised kernel sets, and the step tables carry that through a few fp32
    operations, some of which cancel against values up to sigma_max = 80 (80 * 2^-23 = 1e-5): there the float scalars are held
    to 1e-5 * max(1, |want|) and everything else -- entry points, labels, offsets, integers, flags, order -- stays exact."""
    if exact or type(got) is not type(want):
        return got == want
    if isinstance(want, list):
        return len(got) == len(want) and all(same(g, w, exact) for g, w in zip(got, want))
    if isinstance(want, float):
        return abs(got - want) <= 1e-5 * max(1.0, abs(want))
    return got == want


@pytest.mark.parametrize("case", sorted(loop_trace.CASES))
def test_record_equals_the_parents(case, gold):
    got, want = trace(case), gold["cases"][case]
    exact = gold["cpu"] == {"cpu_capability": torch.backends.cpu.get_cpu_capability(), "cpu_vendor": cpu_vendor()}
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert same(g, w, exact), f"launch (or give) {i} of {case!r} differs from the parent's: {g} != {w}"
    assert len(got["calls"]) == len(want["calls"])
    assert got["rng"] == want["rng"]                         # what set_noise wrote of (seed, offset)
    assert (got["result"], got["result_shape"]) == (want["result"], want["result_shape"])


def test_cases_reach_every_step_entry_point(gold):
    """gold["entry_points"]: what the parent's loops launched over the whole table, listed by the tool."""
    assert sorted({c[0] for t in gold["cases"].values() for c in t["calls"]} - {"give"}) == gold["entry_points"]
    assert sorted({c[0] for case in loop_trace.CASES for c in trace(case)["calls"]} - {"give"}) == gold["entry_points"]
    assert loop_trace.REQUIRED <= set(gold["entry_points"])
