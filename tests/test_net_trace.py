"""PUNetG's and ADM's walks (and ADM's stand-alone blocks) decide what is launched, with which buffers, in which order; for the
configurations of tests/net_trace.py they must hand the library exactly what their parent handed it --
tests/golden/net_trace.json.gz and adm_trace.json.gz, recorded from the parent commit's diffsci_amd/ by
tools/make_net_trace_golden.py.  Host only: the library is replaced by a recorder and no kernel runs, so equal
launches, arguments, pool order and ATen writes mean the device sees the same work."""
import gzip
import json
import os

import pytest

from . import net_trace

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TABLES = sorted(net_trace.TABLES)
_traces = {}


@pytest.fixture(scope="module")
def gold():
    def load(table):
        with gzip.open(os.path.join(GOLDEN, table + ".json.gz"), "rt") as f:
            return json.load(f)
    return {table: load(table) for table in TABLES}


def trace(table, case):
    if (table, case) not in _traces:
        _traces[table, case] = json.loads(json.dumps(net_trace.trace_of(case, net_trace.TABLES[table])))
    return _traces[table, case]


def test_case_table_and_golden_have_the_same_keys(gold):
    for table in TABLES:
        assert set(gold[table]["cases"]) == set(net_trace.TABLES[table]), table


# the PUNetG cases keep the test ids they had when theirs was the only table
@pytest.mark.parametrize("table,case", [pytest.param(t, c, id=c if t == "net_trace" else f"{t}-{c}")
                                        for t in TABLES for c in sorted(net_trace.TABLES[t])])
def test_record_equals_the_parents(table, case, gold):
    got, want = trace(table, case), gold[table]["cases"][case]
    assert got["pool"] == want["pool"]                       # as many pool buffers taken
    assert got["pool"][1] == 0                               # ... and none kept
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"launch (or give) {i} of {case!r} differs from the parent's"
    assert len(got["calls"]) == len(want["calls"])
    assert got["writes"] == want["writes"]                   # what ATen wrote into pool buffers


def test_cases_reach_every_entry_point_of_the_forward_pass(gold):
    """gold[table]["entry_points"]: what the parent's network launched over the whole table, listed by the tool."""
    for table in TABLES:
        g = gold[table]
        assert sorted({c[0] for t in g["cases"].values() for c in t["calls"]} - {"give"}) == g["entry_points"], table
        assert sorted({c[0] for case in net_trace.TABLES[table] for c in trace(table, case)["calls"]} - {"give"}) == g["entry_points"], table
