"""LinkState.track_select / select_delta / select_tracked on the host path
(set_host_spf: no device), the Python argument checks and the new exports.

The expected delta is oracle-derived (seldelta_ref): select_ref.expect on the
graph before and after, diffed in numpy, rebased nodes from
select_ref.root_neighbor_ids. Every event asserts 0 < changed < V * P."""
import ctypes

import numpy as np
import pytest

import select_ref as R
import seldelta_ref as D
from openr_amd import _native as N
from openr_amd.adjdb import AdjDb
from openr_amd.linkstate import LinkState, LinkStateError


def host_ls(version, table, use_link_metric=True):
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(version.stream)
    ls.track_select(D.prefixes_by_name(version.names, table), use_link_metric)
    return ls


def step(ls, before, after, table, use_link_metric=True, vacuous_ok=False):
    """apply `after`, then select_delta == the oracle-derived delta"""
    ls.apply(after.stream)
    d = ls.select_delta()
    assert not d["full"]
    W = d["nh"].shape[1]
    assert W == after.words
    changed, rebased, ea, _ = D.delta(before, after, table, max(W, before.words), use_link_metric)
    ea = (ea[0], ea[1], ea[2][:, :, :W])
    if not vacuous_ok:
        assert 0 < len(changed) < before.V * len(table)
    assert sorted(d["rebased"].tolist()) == rebased
    got, want = D.records(d["changes"], d["nh"]), D.wanted(changed, ea)
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    assert got == want
    for g, w in zip(ls.select_tracked(after.names), ea):  # the baseline is the graph after
        assert np.array_equal(g, w)
    return changed, rebased, ea


@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("kind,seed,k_down", [("unit", 0, 0), ("weighted", 1, 1)])
def test_host_delta_random_graphs(kind, seed, k_down, hop):
    base = D.Version(D.base_dbs(kind, seed))
    table = R.random_table(base.V, np.random.default_rng(100 + seed))
    ls = host_ls(base, table, not hop)
    for g, w in zip(ls.select_tracked(base.names), base.expect(table, base.words, not hop)):
        assert np.array_equal(g, w)
    down = D.Version(D.link_down(base.dbs, 0 if hop else k_down))
    ovl = D.Version(D.node_overload(base.dbs, 0))
    step(ls, base, down, table, not hop)
    step(ls, down, base, table, not hop)
    step(ls, base, ovl, table, not hop)
    if kind == "weighted" and not hop:  # only the ECMP set moves
        ecmp = D.Version(D.metric_bump(base.dbs, 75))
        step(ls, ovl, base, table)
        changed, _, ea = step(ls, base, ecmp, table)
        eb = base.expect(table, base.words)
        assert all(ea[0][r, p] == eb[0][r, p] for r, p in changed)
    assert ls.counters()["engine_errors"] == 0


def test_host_delta_announcers_disconnected_and_back():
    base = D.Version(D.base_dbs("sparse-unit", 0))
    table = R.random_table(base.V, np.random.default_rng(7))
    eb = base.expect(table, base.words)
    for k in range(len(D.up_adjs(base.dbs))):
        cut = D.Version(D.link_down(base.dbs, k))
        ea = cut.expect(table, base.words)
        lost = (ea[0] == R.INF) & (eb[0] != R.INF)
        if lost.any():
            break
    assert lost.any(), "this seed must have a bridge"
    ls = host_ls(base, table)
    changed, _, ea = step(ls, base, cut, table)
    assert {(int(r), int(p)) for r, p in np.argwhere(lost)} <= changed
    assert all(ea[1][r, p] == 0 and not ea[2][r, p].any() for r, p in np.argwhere(lost))
    step(ls, cut, base, table)


def test_host_delta_no_event():
    base = D.Version(D.base_dbs("weighted", 1))
    table = R.random_table(base.V, np.random.default_rng(3))
    ls = host_ls(base, table)
    ls.apply(base.stream)
    d = ls.select_delta()
    assert not d["full"] and len(d["changes"]) == 0 and len(d["rebased"]) == 0


def test_host_delta_rebase():
    base = D.Version(D.base_dbs("unit", 2))
    a, b = D.non_neighbours(base, 5)
    up = D.Version(D.link_up(base.dbs, a, b))
    table = R.random_table(base.V, np.random.default_rng(9))
    ls = host_ls(base, table)
    changed, rebased, _ = step(ls, base, up, table)
    ends = sorted([base.names.index(a), base.names.index(b)])
    assert rebased == ends and not any(r in ends for r, _ in changed)


def test_host_delta_rebase_one_word_to_two():
    dbs = D.star_dbs(32, extra=1)
    base = D.Version(dbs)
    up = D.Version(D.link_up(dbs, "hub", "x0", 2))
    assert base.words == 1 and up.words == 2
    table = [[]] + [[v] for v in range(base.V)] + [list(range(base.V))]
    ls = host_ls(base, table)
    _, rebased, _ = step(ls, base, up, table)
    assert rebased == sorted([base.names.index("hub"), base.names.index("x0")])
    step(ls, up, base, table)


def test_host_delta_node_added_is_full():
    base = D.Version(D.base_dbs("weighted", 1))
    table = R.random_table(base.V, np.random.default_rng(101))
    ls = host_ls(base, table)
    grown = D.link_up(base.dbs + [AdjDb("r-new", [], 999)], "r-new", base.names[3], 2)
    more = D.Version(grown)
    ls.apply(more.stream)
    d = ls.select_delta()
    assert d["full"] and len(d["changes"]) == 0 and len(d["rebased"]) == 0
    table2 = [[more.names.index(base.names[x]) for x in ann] for ann in table]
    for g, w in zip(ls.select_tracked(more.names), more.expect(table2, more.words)):
        assert np.array_equal(g, w)
    step(ls, more, D.Version(D.node_overload(grown, 0)), table2)


def test_argument_checks():
    ls = LinkState()
    ls.set_host_spf(True)
    base = D.Version(D.base_dbs("unit", 0))
    ls.apply(base.stream)
    with pytest.raises(LinkStateError):
        ls.select_delta()  # nothing tracked
    with pytest.raises(LinkStateError):
        ls.select_tracked([base.names[0]])
    with pytest.raises(ValueError):
        ls.track_select({"p": ["a\nb"]})
    ls.track_select({"p": [base.names[1]], "q": []})
    with pytest.raises(LinkStateError):
        ls.select_tracked(["no-such-node"])
    m, c, nh = ls.select_tracked([base.names[1], base.names[2]], nh_words=3)
    assert m.shape == (2, 2) and nh.shape == (2, 2, 3) and m[0, 0] == 0 and c[0, 0] == 1
    assert (m[:, 1] == R.INF).all() and not nh[:, :, 1:].any()
    from openr_amd.engine import CHANGE_DTYPE, SelState, SelStateOverflow
    assert CHANGE_DTYPE.itemsize == 16 and CHANGE_DTYPE.names == ("root", "prefix", "metric", "count")
    e = SelStateOverflow("x", 5, 2)
    assert e.code == -4 and e.n_changes == 5 and e.n_rebased == 2
    with pytest.raises(ValueError):
        SelState.update(None, None, cap=-1)
    with pytest.raises(ValueError):
        SelState.copy(object.__new__(SelState), [0], 0)


def test_new_symbols_are_exported():
    eng = ctypes.CDLL(N.ENGINE_SO)
    for name in ("ospf_selstate_create", "ospf_selstate_destroy", "ospf_selstate_last_error",
                 "ospf_selstate_device_bytes", "ospf_selstate_prime", "ospf_selstate_update",
                 "ospf_selstate_copy"):
        assert hasattr(eng, name) and name in N.ENGINE_SYMBOLS, name
    dec = ctypes.CDLL(N.DECISION_SO)
    for name in ("odl_track_select", "odl_select_delta", "odl_select_tracked"):
        assert hasattr(dec, name) and name in N.DECISION_SYMBOLS, name
    assert N.engine().ospf_selstate_destroy(None) == -1
    assert N.engine().ospf_selstate_last_error(None) == b"null select state"
