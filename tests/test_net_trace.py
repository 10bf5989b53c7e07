"""PUNetG's walk decides what is launched, with which buffers, in which order; for the configurations of tests/net_trace.py it
must hand the library exactly what its parent handed it -- tests/golden/net_trace.json.gz, recorded from the parent commit's
diffsci_amd/ by tools/make_net_trace_golden.py.  Host only: the library is replaced by a recorder and no kernel runs, so equal
launches, arguments, pool order and ATen writes mean the device sees the same work."""
import gzip
import json
import os

import pytest

from . import net_trace

GOLD = os.path.join(os.path.dirname(__file__), "golden", "net_trace.json.gz")
_traces = {}


@pytest.fixture(scope="module")
def gold():
    with gzip.open(GOLD, "rt") as f:
        return json.load(f)


def trace(case):
    if case not in _traces:
        _traces[case] = json.loads(json.dumps(net_trace.trace_of(case)))
    return _traces[case]


def test_case_table_and_golden_have_the_same_keys(gold):
    assert set(gold["cases"]) == set(net_trace.CASES)


@pytest.mark.parametrize("case", sorted(net_trace.CASES))
def test_record_equals_the_parents(case, gold):
    got, want = trace(case), gold["cases"][case]
    assert got["pool"] == want["pool"]                       # as many pool buffers taken
    assert got["pool"][1] == 0                               # ... and none kept
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"launch (or give) {i} of {case!r} differs from the parent's"
    assert len(got["calls"]) == len(want["calls"])
    assert got["writes"] == want["writes"]                   # what ATen wrote into pool buffers


def test_cases_reach_every_entry_point_of_the_forward_pass(gold):
    """gold["entry_points"]: what the parent's network launched over the whole table, listed by the tool."""
    assert sorted({c[0] for t in gold["cases"].values() for c in t["calls"]} - {"give"}) == gold["entry_points"]
    assert sorted({c[0] for case in net_trace.CASES for c in trace(case)["calls"]} - {"give"}) == gold["entry_points"]
