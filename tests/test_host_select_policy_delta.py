"""The tracked policy selection on the host path (LinkState.track_select_policy
/ policy_delta / policy_tracked / set_tracked_policy with set_host_spf(True)):
the same walks as on the device, against the numpy diff of
selpolicy_ref.expect; the rules between plain and policy tracking, the
argument checks and the exported symbols."""
import numpy as np
import pytest

import policy_delta_ref as PD
import seldelta_ref as D
import select_ref as R
import selpolicy_ref as PR
from openr_amd import _native as N
from openr_amd import engine as E
from openr_amd.adjdb import AdjDb
from openr_amd.linkstate import LinkState, LinkStateError

NEW_ENGINE = ("ospf_selstate_create_policy", "ospf_selstate_update_policy",
              "ospf_selstate_copy_policy", "ospf_selstate_set_policy")
NEW_DECISION = ("odl_track_select_policy", "odl_policy_delta", "odl_policy_tracked",
                "odl_set_tracked_attrs")


def host_ls(version):
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(version.stream)
    return ls


def test_new_symbols_are_exported():
    eng, dec = N.engine(), N.decision()
    for name in NEW_ENGINE:
        assert name in N.ENGINE_SYMBOLS and getattr(eng, name).argtypes is not None
    for name in NEW_DECISION:
        assert name in N.DECISION_SYMBOLS and getattr(dec, name).argtypes is not None
    assert E.PCHANGE_DTYPE.itemsize == 32
    assert E.PCHANGE_DTYPE.names == ("root", "prefix", "metric", "count", "links", "need", "best",
                                     "installed")


@pytest.mark.parametrize("hop", [False, True])
def test_host_walk_links_down_up_overload_and_attributes(hop):
    """links down and up again, a node overloaded, then an attribute change
    with no topology event (two classes swapped); every step == the numpy diff"""
    base = D.Version(D.base_dbs("weighted", 1))
    down = D.Version(D.link_down(D.link_down(base.dbs, 3), 11))
    ovl = D.Version(D.node_overload(base.dbs, 0))
    rng = np.random.default_rng(41)
    table = R.random_table(base.V, rng)
    pol = PR.random_policy(table, rng, classes=3, max_need=4)
    swapped = ([[{0: 1, 1: 0}.get(c, c) for c in cs] for cs in pol[0]], pol[1])
    ls = host_ls(base)
    ls.track_select_policy(PD.prefixes_by_name(base.names, table, pol), not hop)
    e0, _ = PD.expect(base, table, *pol, base.words, hop)
    got = ls.policy_tracked(base.names)
    for k in PR.KEYS + ("installed",):
        assert np.array_equal(got[k], e0[k]), k
    prev = base
    for v in (down, base, ovl):
        ls.apply(v.stream)
        changed = PD.assert_linkstate_delta(ls, prev, v, table, pol, pol, hop)
        assert 0 < len(changed) < base.V * len(table)
        prev = v
    ls.set_tracked_policy(PD.prefixes_by_name(base.names, table, swapped))
    changed = PD.assert_linkstate_delta(ls, ovl, ovl, table, pol, swapped, hop)
    assert 0 < len(changed) < base.V * len(table)
    d = ls.policy_delta()  # nothing since
    assert len(d["changes"]) == 0 and len(d["rebased"]) == 0 and not d["full"]
    assert ls.counters()["engine_errors"] == 0


def test_host_single_column_changes():
    a, r, t, x = range(4)
    table = [[x], [t, x], [a, t]]
    pol0 = ([[0], [0, 0], [0, 0]], [[2], [0, 0], [0, 0]])
    pol1 = ([[0], [0, 0], [0, 0]], [[2], [1, 0], [0, 0]])
    v0 = D.Version(PD.column_dbs())
    v1 = D.Version(PD.column_dbs(down=[("r", "r-x-2")]))
    v2 = D.Version(PD.column_dbs(down=[("r", "r-x-2"), ("a", "a-x")]))
    ls = host_ls(v0)
    ls.track_select_policy(PD.prefixes_by_name(v0.names, table, pol0))
    for before, after, pb, pa, key in ((v0, v1, pol0, pol0, "links"), (v1, v1, pol0, pol1, "need"),
                                       (v1, v2, pol1, pol1, "best")):
        eb, _ = PD.expect(before, table, *pb, 1)
        ea, _ = PD.expect(after, table, *pa, 1)
        only = PD.only_column(eb, ea, key)
        assert only[r].any(), key
        if after is before:
            ls.set_tracked_policy(PD.prefixes_by_name(v0.names, table, pa))
        else:
            ls.apply(after.stream)
        changed = PD.assert_linkstate_delta(ls, before, after, table, pb, pa)
        assert {(int(i), int(p)) for i, p in np.argwhere(only)} <= changed


def test_host_node_added_reports_full():
    base = D.Version(D.base_dbs("weighted", 1))
    rng = np.random.default_rng(42)
    table = R.random_table(base.V, rng)
    pol = PR.random_policy(table, rng)
    ls = host_ls(base)
    by_name = PD.prefixes_by_name(base.names, table, pol)
    ls.track_select_policy(by_name)
    more = D.Version(D.link_up(base.dbs + [AdjDb("r-new", [], 999)], "r-new", base.names[3], 2))
    assert more.V == base.V + 1
    ls.apply(more.stream)
    d = ls.policy_delta()
    assert d["full"] and len(d["changes"]) == 0 and len(d["rebased"]) == 0
    table2 = [[more.names.index(base.names[v]) for v in ann] for ann in table]
    e, _ = PD.expect(more, table2, *pol, more.words)
    got = ls.policy_tracked(more.names)
    for k in PR.KEYS:
        assert np.array_equal(got[k], e[k]), k


def test_plain_and_policy_tracking_refuse_each_other():
    base = D.Version(D.base_dbs("unit", 0))
    table = [[0], [1, 2]]
    pol = ([[0], [0, 1]], [[0], [2, 0]])
    by_name = PD.prefixes_by_name(base.names, table, pol)
    ls = host_ls(base)
    for call in (ls.policy_delta, lambda: ls.policy_tracked(base.names[:1]),
                 lambda: ls.set_tracked_policy(by_name)):
        with pytest.raises(LinkStateError):  # nothing tracked
            call()
    ls.track_select(D.prefixes_by_name(base.names, table))
    for call in (ls.policy_delta, lambda: ls.policy_tracked(base.names[:1]),
                 lambda: ls.set_tracked_policy(by_name)):
        with pytest.raises(LinkStateError):  # tracked without attributes
            call()
    assert len(ls.select_delta()["changes"]) == 0
    ls.track_select_policy(by_name)
    for call in (ls.select_delta, lambda: ls.select_tracked(base.names[:1])):
        with pytest.raises(LinkStateError):  # tracked with attributes
            call()
    assert len(ls.policy_delta()["changes"]) == 0


def test_argument_checks():
    base = D.Version(D.base_dbs("unit", 0))
    table = [[0], [1, 2]]
    pol = ([[0], [0, 1]], [[0], [2, 0]])
    by_name = PD.prefixes_by_name(base.names, table, pol)
    ls = host_ls(base)
    ls.track_select_policy(by_name)
    with pytest.raises(LinkStateError):  # fewer attribute sets than tracked names
        ls.set_tracked_policy({"p0": by_name["p0"]})
    with pytest.raises(LinkStateError):  # more
        ls.set_tracked_policy(dict(by_name, p2=by_name["p0"]))
    with pytest.raises(LinkStateError):
        ls.policy_tracked(["no-such-node"])
    with pytest.raises(ValueError):
        ls.track_select_policy({"p": [("a\tb", 0, 0, 0, None)]})
    # an unknown announcer name is dropped with its attributes
    odd = {"p0": [("no-such-node", 1, 1, 1, 3)] + list(by_name["p0"]), "p1": by_name["p1"]}
    ls.track_select_policy(odd)
    e, _ = PD.expect(base, table, *pol, base.words)
    got = ls.policy_tracked(base.names)
    for k in PR.KEYS:
        assert np.array_equal(got[k], e[k]), k
