"""LinkState.all_sources_select_policy on the host path (set_host_spf: no
device) against the restatement of selpolicy_ref, and the restatement against
the project's fixture-pinned per-node route build (route_dbs with best-route
selection on): a unicast route exists iff `installed`, its igpCost is
`metric`, its next hops are `links` links towards the decoded `nh`
neighbours, and its best announcer is `best`.

Graphs: a random weighted graph at p = 0.05 (select_ref's sparse-weighted:
some roots do not reach every node, so the best class can be unreachable) and
drained_fabric(6, 4). Every case asserts that its table exercises the corners
of the rule; the unreachable-best-class corner needs unreached nodes, so it is
asserted on the sparse graph (the fabric is connected)."""
import numpy as np
import pytest

import select_ref as R
import selpolicy_ref as PR
from openr_amd.linkstate import LinkState

CASES = [("sparse-weighted", 1), ("fabric", 3)]
# (path preference, source preference, distance) by class rank: 0 wins
CLASS_ATTRS = [(1000, 200, 1), (1000, 200, 4), (1000, 100, 0), (900, 300, 0)]


def host_ls(kind, seed):
    st, _ = R.graph(kind, seed)
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(st)
    return ls


def build_table(names, csr, spf, rng):
    """Random prefixes plus the targeted ones -> (table, pref, mnh)"""
    V = len(names)
    drained = np.nonzero(np.asarray(csr["no_transit"]))[0].tolist()
    live = [v for v in range(V) if v not in set(drained)]
    assert len(drained) >= 2 and len(live) >= 2, "the graph needs drained and undrained nodes"
    table = [[]] + [sorted(rng.choice(V, size=k, replace=False).tolist())
                    for k in (1, 2, 3, 5, 9, 20)]
    pref, mnh = PR.random_policy(table, rng, classes=3, max_need=4)

    def add(ann, pr, mn):
        order = np.argsort(ann)
        table.append([ann[i] for i in order])
        pref.append([pr[i] for i in order])
        mnh.append([mn[i] for i in order])

    d0, d1, u0, u1 = drained[0], drained[1], live[0], live[-1]
    add([d0, u0], [0, 0], [0, 0])        # a drained announcer (and root) beside an undrained one
    add([d0, d1], [1, 1], [2, 0])        # a class of drained announcers only
    add([u0, u1], [0, 0], [0, 9])        # a threshold no root's links meet, on one announcer
    add([d0, d1, u1], [0, 0, 1], [0, 0, 0])  # the better class is all drained
    miss = R.unreached(spf, names)
    if miss:  # the best class announced only by nodes some root does not reach
        root = sorted(miss)[0]
        far = [names.index(x) for x in miss[root]][:3]
        near = [v for v in live if names[v] in spf[root] and v not in far][:2]
        add(far + near, [0] * len(far) + [2] * len(near), [0] * (len(far) + len(near)))
    return table, pref, mnh


def as_prefixes(names, table, pref, mnh):
    """the Python face's input: per entry raw attributes of its class; every
    third threshold of 0 is passed as None, a negative one never withholds"""
    out, n = {}, 0
    for p, ann in enumerate(table):
        ents = []
        for a, c, m in zip(ann, pref[p], mnh[p]):
            pp, sp, d = CLASS_ATTRS[c]
            n += 1
            ents.append((names[a], pp, sp, d, (None if n % 3 else -5) if m == 0 else m))
        out[f"p{p}"] = ents
    return out


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    kind, seed = request.param
    ls = host_ls(kind, seed)
    names, csr = ls.node_names(), ls.csr()
    spf = R.oracle_spf(kind, seed, 70, tuple(names), True)
    table, pref, mnh = build_table(names, csr, spf, np.random.default_rng(40 + seed))
    W = max(1, max((len(R.root_neighbor_ids(csr, r)) + 31) // 32 for r in range(len(names))))
    want, facts = PR.expect(spf, names, csr, table, pref, mnh, W)
    return dict(kind=kind, ls=ls, names=names, csr=csr, spf=spf, table=table, pref=pref, mnh=mnh,
                W=W, want=want, facts=facts)


def test_table_exercises_the_rule(case):
    f = case["facts"]
    for k in ("filtered", "all_drained", "drained_root_skipped", "need_outside_L", "withheld",
              "best_outside", "routes"):
        assert f[k] > 0, (k, f)
    if case["kind"].startswith("sparse"):
        assert f["fallback"] > 0, f


def test_host_face_equals_restatement(case):
    ls, names = case["ls"], case["names"]
    got = ls.all_sources_select_policy(as_prefixes(names, case["table"], case["pref"], case["mnh"]))
    assert got["nh"].shape[2] == case["W"]
    PR.assert_equal(got, case["want"])
    assert np.array_equal(got["installed"], case["want"]["installed"])
    assert ls.counters()["engine_errors"] == 0


def test_host_face_hop_count(case):
    ls, names = case["ls"], case["names"]
    kind, seed = next(c for c in CASES if c[0] == case["kind"])
    spf = R.oracle_spf(kind, seed, 70, tuple(names), False)
    want, _ = PR.expect(spf, names, case["csr"], case["table"], case["pref"], case["mnh"],
                        case["W"], hop=True)
    got = ls.all_sources_select_policy(
        as_prefixes(names, case["table"], case["pref"], case["mnh"]), use_link_metric=False)
    PR.assert_equal(got, want)


def test_restatement_equals_route_build(case):
    """route_dbs(best_route_selection=True), the per-node build the
    Decision.BestRouteSelection / minNexthop fixtures pin."""
    ls, names, csr, want = case["ls"], case["names"], case["csr"], case["want"]
    table, pref, mnh = case["table"], case["pref"], case["mnh"]
    prefixes = {}
    for p, ann in enumerate(table):
        if ann:
            prefixes[f"p{p}"] = [(names[a], "ip", "ecmp", 0, None, None, m or None, CLASS_ATTRS[c])
                                 for a, c, m in zip(ann, pref[p], mnh[p])]
    rng = np.random.default_rng(9)
    roots = sorted(set(rng.choice(len(names), size=24, replace=False).tolist()) |
                   set(np.nonzero(np.asarray(csr["no_transit"]))[0][:2].tolist()))
    dbs = ls.route_dbs([names[r] for r in roots], prefixes, best_route_selection=True,
                       binary=False)
    seen = 0
    for r in roots:
        db = dbs[names[r]]
        routes = db["routes"] if db else {}
        nbrs = R.root_neighbor_ids(csr, r)
        for p, ann in enumerate(table):
            if not ann:
                continue
            key = f"p{p}"
            assert (key in routes) == bool(want["installed"][r, p]), (names[r], key)
            if key not in routes:
                continue
            seen += 1
            assert routes[key][0] == want["metric"][r, p]
            hops = db[("U", key)]
            assert len(hops) == want["links"][r, p]
            assert {names.index(h[1]) for h in hops} == PR.decode(want["nh"][r, p], nbrs)
            assert db["best"][key][0][0] == names[int(want["best"][r, p])]
    assert seen > 50


def test_names_given_twice_and_unknown_names(case):
    """The first occurrence of a name counts; unknown names go with their
    attributes."""
    ls, names, csr = case["ls"], case["names"], case["csr"]
    a, b = names[3], names[11]
    prefixes = {"x": [("no-such-node", 2000, 0, 0, 7), (a, 1000, 0, 0, None), (b, 1000, 0, 0, 3),
                      (a, 5000, 0, 0, 9)]}
    got = ls.all_sources_select_policy(prefixes)
    want, _ = PR.expect(case["spf"], names, csr, [[3, 11]], [[0, 0]], [[0, 3]], case["W"])
    PR.assert_equal(got, want)


def test_bad_arguments(case):
    ls = case["ls"]
    with pytest.raises(ValueError):
        ls.all_sources_select_policy({"x": [("", 0, 0, 0, None)]})
    if case["W"] > 1:  # a width below the widest node's
        from openr_amd.linkstate import LinkStateError
        with pytest.raises(LinkStateError):
            ls.all_sources_select_policy({"x": [(case["names"][0], 0, 0, 0, None)]}, nh_words=1)
