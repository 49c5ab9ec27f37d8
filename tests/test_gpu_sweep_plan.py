"""The launch plan of a sweep is pinned: what each planner of
openr_amd/csrc/engine (derive, batch, lds, wcover, wmulti, wderive) decides
for a small graph -- the launch units in capture order with their kernels,
root counts, next-hop words and compulsory bytes, the sweep's totals, its
device bytes and the order of its roots -- equals the table recorded in
tests/data/sweep_plans.json (scripts/record_sweep_plans.py regenerates it).
A change of the planners' code that is meant to keep behaviour keeps this
table; a change of the plan shows here before it shows in a benchmark.

Every case takes a fresh Engine: device_bytes depends on which pooled blocks
of destroyed sweeps the allocations reuse, and an engine's pool starts empty.
The graphs are the small ones tests/test_gpu_sweep.py reaches each planner with."""
import json
import os

import pytest

from graphs import drained_fabric, random_stream
from openr_amd import topology as T
from openr_amd.engine import Engine, Sweep
from openr_amd.linkstate import LinkState

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "sweep_plans.json")
LAUNCH_KEYS = ("name", "kernel", "n_roots", "nh_words", "compulsory_bytes")
INFO_KEYS = ("mode", "n_rows", "n_launches", "step_compulsory_bytes", "step_traversed_edges",
             "device_bytes")


def _closure_fabric():
    return drained_fabric(40, 4, seed=5, drain=0.0, down=0.0, weighted_seed=11, ssw_per_plane=4)


# name -> (graph, Sweep keywords, environment knobs)
CASES = {
    "derive": (lambda: drained_fabric(6, 4, seed=3), dict(mode="derive"), {}),
    "derive_twins_forced_staged": (
        lambda: drained_fabric(6, 4, seed=3), dict(mode="derive"),
        {"OSPF_SWEEP_TWIN": "1", "OSPF_SWEEP_TWINLV": "1", "OSPF_SWEEP_STAGES": "8"}),
    "derive_no_twin_levels": (lambda: drained_fabric(6, 4, seed=3), dict(mode="derive"),
                              {"OSPF_SWEEP_NOTWINLV": "1"}),
    "derive_part_1_of_2": (lambda: T.fabric(pods=9, planes=4),
                           dict(mode="derive", part=1, n_parts=2), {}),
    "wderive": (lambda: random_stream(10, n=70, unit=False, wmax=50)[0], dict(mode="wderive"), {}),
    "batch": (lambda: random_stream(10, n=70, unit=False, wmax=50)[0], dict(mode="batch"), {}),
    "lds": (lambda: random_stream(0, n=70, unit=True)[0], dict(mode="lds"), {}),
    "wcover_closure": (_closure_fabric, dict(mode="wcover"), {}),
    "wcover_dial": (_closure_fabric, dict(mode="wcover"), {"OSPF_COVER_NOCLOSURE": "1"}),
    "wcover_closure_staged": (_closure_fabric, dict(mode="wcover"), {"OSPF_WCOVER_STAGE": "1"}),
    "wcover_part_0_of_2": (_closure_fabric, dict(mode="wcover", part=0, n_parts=2), {}),
    "wmulti": (lambda: random_stream(40, n=90, unit=False, wmax=30)[0], dict(mode="wmulti"), {}),
}


def record(case):
    """The plan of one case from the library as built (the knobs of the case
    must be in the environment already)."""
    graph, kw, _ = CASES[case]
    ls = LinkState()
    ls.apply(graph())
    eng = Engine()
    try:
        eng.load(ls.csr())
        sw = Sweep(eng, **kw)
        try:
            out = {k: getattr(sw, k) for k in INFO_KEYS}
            out["roots"] = sw.roots.tolist()
            out["launches"] = [{k: p[k] for k in LAUNCH_KEYS} for p in sw.profile(1)]
            return out
        finally:
            sw.close()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def table():
    with open(TABLE, encoding="utf-8") as f:
        return json.load(f)


def test_table_has_exactly_the_cases(table):
    assert sorted(table["plans"]) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_sweep_plan_is_the_recorded_one(case, table, monkeypatch):
    for k, v in CASES[case][2].items():
        monkeypatch.setenv(k, v)
    got, want = record(case), table["plans"][case]
    for k in INFO_KEYS:
        assert got[k] == want[k], (case, k)
    assert [u["name"] for u in got["launches"]] == [u["name"] for u in want["launches"]], case
    for g, w in zip(got["launches"], want["launches"]):
        assert g == w, (case, w["name"])
    assert got["roots"] == want["roots"], case
