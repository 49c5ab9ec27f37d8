"""The policy selection at its word, key and count limits on the host path,
and the expectation test_gpu_policy_limits.py uses, proved against the
product's own faces without a GPU: LinkState.all_sources_select_policy and
all_sources_select_srmpls with set_host_spf(True), and the per-node route build
route_dbs(best_route_selection=True), i.e. SpfSolver::createRouteForPrefix
(openr/decision/SpfSolver.cpp:197-458). The fixtures and what makes each a
limit case are in policy_limits.py; for the 66-word star only the sampled
roots are judged."""
import numpy as np
import pytest

import policy_limits as L
import selpolicy_ref as PR
import srmpls_ref as SR
from openr_amd.linkstate import LinkState


@pytest.fixture(scope="module")
def cases():
    """every fixture once for the module (policy_limits.case keeps them)"""
    return {name: L.case(name) for name in L.CASES}


def host_ls(version):
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(version.stream)
    assert ls.node_names() == version.names
    return ls


def rows_of(arrs, roots, keys):
    return {k: arrs[k][roots] for k in keys}


@pytest.mark.parametrize("name", list(L.CASES))
def test_preconditions_hold(cases, name):
    """each fixture is the limit case it claims to be, on the expectation alone"""
    L.preconditions(cases[name])


@pytest.mark.parametrize("name", list(L.CASES))
def test_expectation_is_the_host_path(cases, name):
    """selpolicy_ref / srmpls_ref over the oracle == the product's host
    selection, so the restatement is not its own witness. At 65,536 parallel
    links the host path answers 65,536: the count is never capped there."""
    c = cases[name]
    ls, W, roots = host_ls(c.base), c.base.words, c.judged
    got = ls.all_sources_select_policy(L.policy_prefixes(c))
    assert got["nh"].shape[2] == W
    keys = PR.KEYS + ("installed",)
    PR.assert_equal(rows_of(got, roots, keys), rows_of(c.pol(W), roots, keys), keys, ctx=name)
    got = ls.all_sources_select_srmpls(L.srmpls_prefixes(c))
    want, _ = c.sr(W)
    assert got["entry_offsets"].tolist() == np.concatenate(
        [[0], np.cumsum([len(a) for a in c.table])]).tolist()
    keys = SR.KEYS + ("installed",)
    SR.assert_equal(rows_of(got, roots, keys), rows_of(want, roots, keys), keys, ctx=name)
    assert ls.counters()["engine_errors"] == 0


@pytest.mark.parametrize("name", ["L2", "L3"])
def test_expectation_after_the_update_is_the_host_path(cases, name):
    c = cases[name]
    W, roots = c.base.words, c.judged
    keys = PR.KEYS + ("installed",)
    for i in range(1, len(c.versions)):
        got = host_ls(c.versions[i]).all_sources_select_policy(L.policy_prefixes(c))
        PR.assert_equal(rows_of(got, roots, keys), rows_of(c.pol(W, i), roots, keys), keys,
                        ctx=(name, i))


@pytest.mark.parametrize("name", list(L.CASES))
def test_expectation_is_the_route_build(cases, name):
    """route_dbs(best_route_selection=True) for the nodes each case is about:
    a route exists iff `installed`, its igpCost is `metric`, its next hops are
    `links` links towards the decoded `nh` neighbours, its best announcer is
    `best` (as test_host_select_policy.py compares them)."""
    c = cases[name]
    v, W = c.base, c.base.words
    want, names = c.pol(W), c.base.names
    prefixes = {f"p{p}": [(names[a], "ip", "ecmp", 0, None, None, m or None, L.rank_attrs(k))
                          for a, k, m in zip(ann, c.pref[p], c.mnh[p])]
                for p, ann in enumerate(c.table) if ann}
    roots = sorted(c.focus.values())
    dbs = host_ls(v).route_dbs([names[r] for r in roots], prefixes, best_route_selection=True,
                               binary=False)
    seen = 0
    for r in roots:
        db = dbs[names[r]]
        routes = db["routes"] if db else {}
        nbrs = v.nbrs(r)
        for p, ann in enumerate(c.table):
            key = f"p{p}"
            if not ann:
                continue
            assert (key in routes) == bool(want["installed"][r, p]), (names[r], key)
            if key not in routes:
                continue
            seen += 1
            assert routes[key][0] == want["metric"][r, p], (names[r], key)
            hops = db[("U", key)]
            assert len(hops) == want["links"][r, p], (names[r], key)
            assert {names.index(h[1]) for h in hops} == PR.decode(want["nh"][r, p], nbrs)
            assert db["best"][key][0][0] == names[int(want["best"][r, p])]
    assert seen >= 2, seen


def test_l1_cells_by_hand(cases):
    """the cells the fixture was made for, spelled out"""
    c = cases["L1"]
    a, a1 = c.focus["a"], c.focus["a1"]
    e = c.pol(5)
    far = 0x80000005
    assert e["metric"][a, 0] == far and e["best"][a, 0] == c.ids["c"]          # high-words, lane 0
    assert e["metric"][a, 1] == far + 1 and e["best"][a, 1] == c.ids["k000"]   # a middle lane
    assert e["metric"][a, 2] == far + 1 and e["best"][a, 2] == c.ids["k010"]   # the second trip
    assert e["metric"][a, 3] == L.M31 and e["metric"][a1, 3] == L.B31          # b, rank 1 against 2^30
    assert e["best"][a, 5] == c.ids["k040"]
    assert [int(x) for x in e["need"][a, 6:9]] == [L.B31, L.INF, L.INF]
    assert not e["installed"][a, 6:9].any() and (e["links"][a, 6:9] == 1).all()
    assert e["need"][a, 0] == 2 and e["need"][a, 3] == 3  # the losers' 0xFFFFFFFF never counts
