"""The SR_MPLS route selection on the host: the restatement of srmpls_ref
against the project's fixture-pinned per-node route build (route_dbs with
entries forwarded as sr_mpls), and LinkState.all_sources_select_srmpls on the
host path against the restatement.

Graphs: a 4-node ring and a random 40-node weighted graph with parallel links
of independent metrics and a few drained nodes (srmpls_ref.labelled_stream),
both with valid distinct node labels, so that a route's next hops are exactly
its (link, destination) pairs. The random graph's seed is picked so that every
corner the rule has is met (test_table_exercises_the_rule): only the random
case carries the full set of facts. The ring cannot meet two of them -- it has
no parallel links (parallel_dropped) and no neighbour that is a next hop
towards two nodes at one distance (links_gt_or) -- and asserts the others."""
import collections

import numpy as np
import pytest

import select_ref as R
import selpolicy_ref as PR
import srmpls_ref as SR
from openr_amd.linkstate import LinkState
from oracle import Oracle, parse_spf_text

# (path preference, source preference, distance) by class rank: 0 wins
CLASS_ATTRS = [(1000, 200, 1), (1000, 200, 4), (900, 300, 0)]
PREPEND0 = 60000  # entry e's prepend label is PREPEND0 + e: valid, distinct, no node label


def host_ls(st):
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(st)
    return ls


def random_case(seed):
    st, labels = SR.labelled_stream(seed)
    ls = host_ls(st)
    names, csr = ls.node_names(), ls.csr()
    V = len(names)
    rng = np.random.default_rng(100 + seed)
    table = [[]] + [sorted(rng.choice(V, size=k, replace=False).tolist())
                    for k in (1, 1, 2, 2, 3, 3, 5, 9, 20)] + [list(range(V))]
    pref, mnh = PR.random_policy(table, rng, classes=2, max_need=3)
    flags = SR.random_flags(table, rng)
    # one class, no threshold: equidistant destinations are kept
    table.append(sorted(rng.choice(V, size=12, replace=False).tolist()))
    pref.append([0] * 12)
    mnh.append([0] * 12)
    flags.append(SR.random_flags(table[-1:], rng)[0])
    return st, labels, ls, names, csr, table, pref, mnh, flags


def ring_case():
    st, labels = SR.ring_stream()
    ls = host_ls(st)
    names, csr = ls.node_names(), ls.csr()
    a, b, c, d = (names.index(x) for x in "abcd")
    table = [[a], [a, c], [b, d], [a, b, c, d], [a, c], [b], []]
    pref = [[0], [0, 0], [0, 0], [0, 0, 0, 0], [0, 1], [0], []]
    mnh = [[0], [0, 0], [3, 0], [0, 0, 0, 0], [0, 0], [2], []]
    flags = [[1], [1, 0], [0, 1], [1, 1, 0, 0], [1, 0], [0], []]
    return st, labels, ls, names, csr, table, pref, mnh, flags


@pytest.fixture(scope="module", params=["ring", "random"])
def case(request):
    st, labels, ls, names, csr, table, pref, mnh, flags = \
        ring_case() if request.param == "ring" else random_case(3)
    orc = Oracle(st)
    spf = {r: parse_spf_text(orc.spf_text(r, True)) for r in names}
    hops = {r: parse_spf_text(orc.spf_text(r, False)) for r in names}
    W = max(1, max((len(R.root_neighbor_ids(csr, r)) + 31) // 32 for r in range(len(names))))
    want, facts = SR.expect(spf, names, csr, table, pref, mnh, flags, W)
    return dict(kind=request.param, labels=labels, ls=ls, names=names, csr=csr, spf=spf, hops=hops,
                table=table, pref=pref, mnh=mnh, flags=flags, W=W, want=want, facts=facts)


def as_prefixes(c, flags=None):
    flags = c["flags"] if flags is None else flags
    return {f"p{p}": [(c["names"][a],) + CLASS_ATTRS[k] + (m or None, bool(f))
                      for a, k, m, f in zip(ann, c["pref"][p], c["mnh"][p], flags[p])]
            for p, ann in enumerate(c["table"])}


def test_table_exercises_the_rule(case):
    f = case["facts"]
    assert f["rule1208_fired"] == 0, f
    keys = SR.FACTS if case["kind"] == "random" else \
        ("self_prepend_rerouted", "self_prepend_only", "self_no_flag", "multi_dst", "nh_is_dst",
         "withheld")  # the ring has no parallel links, and no next hop towards two nodes at one distance
    for k in keys:
        assert f[k] > 0, (k, f)


def test_restatement_equals_route_build(case):
    """route_dbs over sr_mpls / ecmp entries: per node and prefix the route is
    there iff `installed`, its next hops are the (neighbour, destination) pairs
    of dst_nh, each over c(r, k) links, `links` of them in all."""
    c = case
    ls, names, csr, want, table = c["ls"], c["names"], c["csr"], c["want"], c["table"]
    off = np.concatenate([[0], np.cumsum([len(a) for a in table])]).astype(int)
    by_label = {v: k for k, v in c["labels"].items()}
    prefixes = {}
    for p, ann in enumerate(table):
        if ann:
            prefixes[f"p{p}"] = [
                (names[a], "sr_mpls", "ecmp", 0, PREPEND0 + off[p] + i if f else None, None,
                 m or None, CLASS_ATTRS[k])
                for i, (a, k, m, f) in enumerate(zip(ann, c["pref"][p], c["mnh"][p], c["flags"][p]))]
    dbs = ls.route_dbs(names, prefixes, best_route_selection=True, binary=False)
    seen = rerouted = 0
    for r, rname in enumerate(names):
        db = dbs[rname]
        routes = db["routes"] if db else {}
        nbrs = R.root_neighbor_ids(csr, r)
        cnt = PR.link_counts(csr, r, False)
        for p, ann in enumerate(table):
            key = f"p{p}"
            if not ann:
                continue
            assert (key in routes) == bool(want["installed"][r, p]), (rname, key)
            if key not in routes:
                continue
            seen += 1
            assert routes[key][0] == want["metric"][r, p], (rname, key)
            got = collections.Counter()
            for _, nbr, _, op, labels, _ in db[("U", key)]:
                dst = by_label[labels[-1]] if labels and labels[-1] in by_label else nbr
                i = ann.index(names.index(dst))
                push = ([PREPEND0 + off[p] + i] if c["flags"][p][i] else []) + \
                    ([c["labels"][dst]] if dst != nbr else [])
                assert list(labels) == push and op == ("PUSH" if push else ""), (rname, key, labels)
                got[(nbr, dst)] += 1
            exp = collections.Counter()
            for i, a in enumerate(ann):
                for k in PR.decode(want["dst_nh"][r, off[p] + i], nbrs):
                    exp[(names[k], names[a])] += cnt[k]
            assert got == exp, (rname, key)
            assert sum(got.values()) == want["links"][r, p]
            rerouted += r in ann and bool(c["flags"][p][ann.index(r)])
    assert seen > (5 if c["kind"] == "ring" else 100) and rerouted > 0


def test_host_face_equals_restatement(case):
    ls = case["ls"]
    got = ls.all_sources_select_srmpls(as_prefixes(case))
    assert got["dst_nh"].shape[2] == case["W"]
    assert got["entry_offsets"].tolist() == np.concatenate(
        [[0], np.cumsum([len(a) for a in case["table"]])]).tolist()
    SR.assert_equal(got, case["want"])
    assert np.array_equal(got["installed"], case["want"]["installed"])
    assert ls.counters()["engine_errors"] == 0


def test_host_face_hop_count(case):
    want, _ = SR.expect(case["hops"], case["names"], case["csr"], case["table"], case["pref"],
                        case["mnh"], case["flags"], case["W"], hop=True)
    got = case["ls"].all_sources_select_srmpls(as_prefixes(case), use_link_metric=False)
    SR.assert_equal(got, want)


def test_no_flag_is_the_policy_selection_unmerged(case):
    """All flags 0: metric / count / need / best are selpolicy_ref's, and the
    OR of a prefix's dst_nh is its nh."""
    c = case
    zero = [[0] * len(a) for a in c["table"]]
    want, _ = SR.expect(c["spf"], c["names"], c["csr"], c["table"], c["pref"], c["mnh"], zero,
                        c["W"])
    pol, _ = PR.expect(c["spf"], c["names"], c["csr"], c["table"], c["pref"], c["mnh"], c["W"])
    got = c["ls"].all_sources_select_srmpls(as_prefixes(c, zero))
    SR.assert_equal(got, want)
    for res in (want, got):
        for k in ("metric", "count", "need", "best"):
            assert np.array_equal(res[k], pol[k]), k
        assert np.array_equal(SR.or_of_prefixes(res["dst_nh"], c["table"]), pol["nh"])
        assert (res["links"] >= pol["links"]).all()


def test_names_given_twice_and_unknown_names(case):
    """The kept entries: unknown names go with their attributes and flag, the
    first occurrence of a name counts, ascending by id."""
    ls, names = case["ls"], case["names"]
    a, b = names[1], names[2]
    got = ls.all_sources_select_srmpls(
        {"x": [("no-such-node", 2000, 0, 0, 7, True), (b, 1000, 0, 0, None, True),
               (a, 1000, 0, 0, 3, False), (b, 3000, 0, 0, 9, False)], "y": []})
    want = ls.all_sources_select_srmpls(
        {"x": [(a, 1000, 0, 0, 3, False), (b, 1000, 0, 0, None, True)], "y": []})
    assert got["entry_offsets"].tolist() == [0, 2, 2] and got["dst_links"].shape[1] == 2
    SR.assert_equal(got, want)
    assert got["metric"][2, 0] == want["metric"][2, 0] != 0  # b's own entry is flagged

