"""UCMP weights over a policy select state on the device (ospf_selstate_ucmp /
ospf_selstate_ucmp_copy on a state of ospf_selstate_create_policy): the result
equals ucmp_policy_ref's recursion with the drained-leaf rule, which
test_host_ucmp_policy.py proves against the CPU oracle's walk; the round count
equals the recursion's depth."""
import numpy as np
import pytest

import select_ref as R
import selpolicy_ref as PR
import ucmp_policy_ref as UP
import ucmp_ref as U
from openr_amd.engine import Engine, SelState, Sweep
from test_gpu_select_policy import hub_stream
from test_host_ucmp_policy import PolicyCase, chain_case, random_case

pytestmark = pytest.mark.gpu


def flat(leaf_w):
    return np.array([w for ws in leaf_w for w in ws], np.int64)


def device_case(case, use_link_metric=True, modes=("batch",)):
    """prime a policy state and resolve both algorithms -> {algo: expectation}"""
    _, sel, consts = case.mode(use_link_metric)
    exp = {algo: case.resolve(sel, consts, algo) for algo in U.ALGOS}
    off, nodes = R.csr_table(case.table)
    everyone = list(range(case.V))
    ran = 0
    for mode in modes:
        eng = Engine()
        try:
            eng.load(case.csr)
            sw = Sweep(eng, mode=mode, hop_count=not use_link_metric)
            sw.run()
            eng.sync()
            st = SelState(eng, off, nodes, PR.flat(case.pref), PR.flat(case.mnh))
            st.prime(sw)
            for algo in U.ALGOS:
                rounds = st.ucmp(algo, flat(case.leaf_w), consts.S)
                assert rounds == exp[algo][2], (mode, algo)
                got = st.ucmp_copy(everyone)
                want = UP.copy_expect(sel, consts, exp[algo], everyone, case.table, case.leaf_w,
                                      case.drained)
                for name, g, w in zip(("advertised", "status", "off", "wt"), got, want):
                    assert np.array_equal(g, w), (mode, algo, name)
            st.close()
            sw.close()
            ran += 1
        finally:
            eng.close()
    assert ran
    return sel, consts, exp


@pytest.mark.parametrize("use_link_metric", [True, False])
@pytest.mark.parametrize("kind", ["class", "drain"])
def test_ucmp_policy_chains(kind, use_link_metric):
    """x - k - u with k overloaded: u takes k's LEAF weight in one round; a
    header-width change without the rule gives x's weight in two."""
    case, (k, u, x) = chain_case(kind)
    sel, consts, exp = device_case(case, use_link_metric)
    assert exp["prefix"][0][:, 0].tolist() == [7, 5, 7] and exp["prefix"][2] == 1
    without = case.resolve(sel, consts, "prefix", leaf_rule=False)
    assert without[0][u, 0] == 7 and without[2] == 2


def test_ucmp_policy_zero_leaf_weight_voids():
    case, (k, u, x) = chain_case("drain", zero=True)
    _, _, exp = device_case(case)
    assert exp["prefix"][1][:, 0].tolist() == [U.OK, U.VOID, U.OK]


@pytest.mark.parametrize("use_link_metric", [True, False])
def test_ucmp_policy_random_overloaded_graph(use_link_metric):
    case = random_case(5, (2, 7, 11))
    _, _, exp = device_case(case, use_link_metric, modes=("batch", "wderive"))
    st = exp["prefix"][1]
    assert (st == U.OK).any() and (st == U.VOID).any() and (st == U.NONE).any()
    assert exp["prefix"][2] >= 2


def wide_case():
    """the hub of 5 next-hop words (a lane per word) with drained spokes among
    the announcers"""
    dbs = hub_stream().to_dbs()
    names = sorted(d.name for d in dbs)
    hub, d0, d1 = (names.index(n) for n in ("hub", "s007", "s090"))
    V = len(names)
    rng = np.random.default_rng(8)
    table = [[hub], [d0], sorted([d0, d1, 20, 60]), sorted([d1, 100])] + \
        [sorted(rng.choice(V, size=k, replace=False).tolist()) for k in (3, 9, 70)]
    pref = [rng.integers(0, 2, size=len(a)).tolist() for a in table]
    leaf_w = [[int(w) for w in rng.choice([2, 3, 4, 6], size=len(a))] for a in table]
    case = PolicyCase(dbs, table, pref, leaf_w)
    assert case.names == names and case.W == 5 and case.drained[d0] and case.drained[d1]
    return case


def test_ucmp_policy_wide_root():
    case = wide_case()
    hub, d0 = case.names.index("hub"), case.names.index("s007")
    table, leaf_w = case.table, case.leaf_w
    sel, consts, exp = device_case(case)
    mine = UP.links(sel, consts, exp["prefix"], hub, 1, table, leaf_w, case.drained)
    assert d0 in [k for k, _, _ in mine]  # a drained leaf among the hub's next hops


# ---------------------------------------------------------------- LinkState
@pytest.mark.parametrize("which", ["class", "drain", "random", "wide"])
def test_linkstate_ucmp_over_a_policy_tracked_table(which):
    """LinkState.all_sources_ucmp / ucmp_tracked on a policy-tracked table run
    on the device over the policy state and equal the recursion."""
    from test_host_ucmp_policy import assert_linkstate, tracked
    if which == "random":
        case = random_case(5, (2, 7, 11))
    elif which == "wide":
        case = wide_case()
    else:
        case = chain_case(which)[0]
    ls = tracked(case, True, host=False)
    for algo in U.ALGOS:
        _, _, res = assert_linkstate(ls, case, True, algo)
        info = ls.ucmp_info
        assert info["device"] is True and info["rounds"] == res[2]
    assert ls.counters()["engine_errors"] == 0
