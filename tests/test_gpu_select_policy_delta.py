"""The policy selection kept resident and its delta on the device
(ospf_selstate_create_policy / update_policy / copy_policy / set_policy):
DecisionRouteDb::calculateUpdate over the routes createRouteForPrefix produces.

Expected values never come from the code under test: policy_delta_ref diffs
selpolicy_ref.expect (the four reference steps over the CPU oracle's SPF)
before and after an event in numpy, over all six columns; the rebased roots
are those whose root_neighbor_ids changed."""
import copy

import numpy as np
import pytest

import policy_delta_ref as PD
import seldelta_ref as D
import select_ref as R
import selpolicy_ref as PR
from openr_amd.engine import EngineError, SelState, SelStateOverflow, Sweep
from test_gpu_select_delta import Rig, modes_for
from policy_delta_ref import column_dbs
from test_gpu_select_policy import hub_stream

pytestmark = pytest.mark.gpu


def policy_state(eng, table, pol):
    off, nodes = R.csr_table(table)
    return SelState(eng, off, nodes, PR.flat(pol[0]), PR.flat(pol[1]))


def assert_update(st, sw, changed, rebased, ea, W, cap=None, what=""):
    rec, nh, reb = st.update_policy(sw, cap=len(changed) + 7 if cap is None else cap,
                                    cap_rebased=len(rebased) + 3, nh_words=W)
    assert sorted(reb.tolist()) == rebased, what
    got, want = PD.records(rec, nh), PD.wanted(changed, ea)
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want))[:8])
    assert got == want, (what, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:4])
    PD.assert_state(st, ea, W, what=what)
    return got


def big_table(V, rng):
    """P = 130 (chunks of 64, 64 and 2); announcer counts 0, 1, 2, 3, 8, 9, 63,
    64, 65 and V (lane, wave, and the 64-stride wrap)."""
    table = R.random_table(V, rng)
    while len(table) < 130:
        table.append(sorted(rng.choice(V, size=int(rng.integers(1, 7)), replace=False).tolist()))
    assert len(table) == 130 and {1, 8, 9, 64, 65, V} <= {len(a) for a in table}
    return table


# ---------------------------------------------------------------- random graphs
@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("kind,seed", [("unit", 0), ("weighted", 1)])
def test_policy_delta_random_graphs_every_mode(kind, seed, hop):
    """two links down, then up again; three classes, thresholds 0-4, drained
    nodes in the graph"""
    base = D.Version(D.base_dbs(kind, seed))
    assert np.asarray(base.csr["no_transit"]).any()
    rng = np.random.default_rng(300 + seed)
    table = big_table(base.V, rng)
    pol = PR.random_policy(table, rng, classes=3, max_need=4)
    down = D.Version(D.link_down(D.link_down(base.dbs, 3), 11))
    W = base.words
    versions = [base, down, base]
    steps = [PD.delta(versions[i - 1], versions[i], table, pol, pol, W, hop) for i in (1, 2)]
    e0, facts = PD.expect(base, table, *pol, W, hop)
    for k in ("filtered", "need_outside_L", "withheld", "best_outside"):
        assert facts[k] > 0, (k, facts)
    for changed, rebased, _, _ in steps:
        assert 0 < len(changed) < base.V * len(table) and not rebased
    ran = []
    for mode in modes_for(kind, hop):
        rig = Rig(mode, hop)
        st = None
        try:
            sw = rig.sweep(base)
            if sw is None:
                continue
            st = policy_state(rig.eng, table, pol)
            st.prime(sw)
            PD.assert_state(st, e0, W, what=(mode, "prime"))
            m, c, nh = st.copy(list(range(base.V)), W)  # the plain copy answers too
            assert np.array_equal(m, e0["metric"]) and np.array_equal(c, e0["count"])
            assert np.array_equal(nh, e0["nh"])
            for i, (changed, rebased, ea, _) in enumerate(steps):
                sw = rig.sweep(versions[i + 1])
                assert sw is not None
                assert_update(st, sw, changed, rebased, ea, W, what=(mode, hop, i))
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    assert "batch" in ran


# ---------------------------------------------------------------- wide roots
def test_policy_delta_wide_root():
    """The hub of 150 spokes (5 words > kSelLaneW, two parallel pairs): the
    lane-per-word store and compare; the hub's link to one spoke gets dearer."""
    dbs = hub_stream().to_dbs()
    after_dbs = copy.deepcopy(dbs)
    for d in after_dbs:
        for a in d.adjs:
            if {d.name, a.other} == {"hub", "s010"}:
                a.metric += 5
    base, after = D.Version(dbs), D.Version(after_dbs)
    hub, V = base.names.index("hub"), base.V
    rng = np.random.default_rng(3)
    table = [[], [hub], [3]] + [[v] for v in range(4, 70)] + \
        [sorted(rng.choice(V, size=k, replace=False).tolist()) for k in (9, 65, 130)] + \
        [list(range(1, V))]
    assert len(table) > 64
    pol = PR.random_policy(table, rng, classes=2, max_need=4)
    W = base.words
    assert W == 5
    changed, rebased, ea, eb = PD.delta(base, after, table, pol, pol, W)
    hubs = [p for r, p in changed if r == hub]
    assert hubs and len(hubs) < len(table) and not rebased
    ran = 0
    for mode in ("batch", "wderive"):
        rig = Rig(mode)
        try:
            sw = rig.sweep(base)
            if sw is None:
                continue
            assert rig.eng.nh_words(hub) == 5
            st = policy_state(rig.eng, table, pol)
            st.prime(sw)
            PD.assert_state(st, eb, W)
            sw = rig.sweep(after)
            assert_update(st, sw, changed, rebased, ea, W, what=mode)
            st.close()
            ran += 1
        finally:
            rig.close()
    assert ran


def test_policy_delta_rebase_grows_a_root_from_one_word_to_two():
    dbs = D.star_dbs(32, extra=1)
    base, up = D.Version(dbs), D.Version(D.link_up(dbs, "hub", "x0", 2))
    hub, x0 = base.names.index("hub"), base.names.index("x0")
    assert base.words == 1 and up.words == 2
    rng = np.random.default_rng(4)
    table = [[]] + [[v] for v in range(base.V)] + [list(range(base.V))] + \
        [sorted({v, (v + 7) % base.V}) for v in range(base.V)]
    pol = PR.random_policy(table, rng, classes=2, max_need=2)
    rig = Rig("batch")
    try:
        sw = rig.sweep(base)
        st = policy_state(rig.eng, table, pol)
        st.prime(sw)
        for before, after in ((base, up), (up, base)):
            changed, rebased, ea, _ = PD.delta(before, after, table, pol, pol, 2)
            assert rebased == sorted([hub, x0]) and changed
            assert_update(st, rig.sweep(after), changed, rebased, ea, 2)
        st.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- single columns
def test_policy_delta_single_column_changes():
    """`links`, `need` and `best` each as the only differing column of a
    record: a half-done compare (metric / count / words only) reports none."""
    a, r, t, x = range(4)
    table = [[x], [t, x], [a, t]]
    pol0 = ([[0], [0, 0], [0, 0]], [[2], [0, 0], [0, 0]])
    pol1 = ([[0], [0, 0], [0, 0]], [[2], [1, 0], [0, 0]])  # t's threshold: in S', outside L for r
    v0 = D.Version(column_dbs())
    v1 = D.Version(column_dbs(down=[("r", "r-x-2")]))
    v2 = D.Version(column_dbs(down=[("r", "r-x-2"), ("a", "a-x")]))
    assert v0.names == ["a", "r", "t", "x"]
    steps = [(v0, v1, pol0, pol0, "links"), (v1, v1, pol0, pol1, "need"), (v1, v2, pol1, pol1, "best")]
    facts = dict(links=0, need=0, best=0, installed_flips=0)
    rig = Rig("batch")
    try:
        sw = rig.sweep(v0)
        st = policy_state(rig.eng, table, pol0)
        st.prime(sw)
        for before, after, pb, pa, key in steps:
            changed, rebased, ea, eb = PD.delta(before, after, table, pb, pa, 1)
            only = PD.only_column(eb, ea, key)
            assert only[r].any(), key
            if after is not before:
                sw = rig.sweep(after)
            else:
                st.set_policy(PR.flat(pa[0]), PR.flat(pa[1]))
            got = assert_update(st, sw, changed, rebased, ea, 1, what=key)
            for rr, p in np.argwhere(only):
                assert (int(rr), int(p)) in got
                facts[key] += 1
            if key == "links":
                assert eb["links"][r, 0] == 2 and ea["links"][r, 0] == 1
                assert eb["installed"][r, 0] and not ea["installed"][r, 0]
                assert got[(r, 0)][5] == 0
                facts["installed_flips"] += 1
            if key == "best":
                assert eb["best"][r, 2] == a and ea["best"][r, 2] == t
        st.close()
    finally:
        rig.close()
    assert all(v > 0 for v in facts.values()), facts


# ---------------------------------------------------------------- in-place overload
def test_policy_delta_in_place_node_overload():
    """ospf_update_nodes + re-sweep: the drain filter flips, and the drained
    root that announces beside an undrained class-mate is no longer selected."""
    base = D.Version(D.base_dbs("weighted", 1))
    ovl_dbs = D.node_overload(base.dbs, 0)
    ovl = D.Version(ovl_dbs)
    node = next(i for i in range(base.V)
                if base.csr["no_transit"][i] != ovl.csr["no_transit"][i])
    mate = next(i for i in range(base.V) if i != node and not ovl.csr["no_transit"][i])
    rng = np.random.default_rng(17)
    table = R.random_table(base.V, rng) + [sorted([node, mate])]
    pol = PR.random_policy(table, rng, classes=2, max_need=3)
    pol[0][-1] = [0, 0]
    W = base.words
    changed, rebased, ea, eb = PD.delta(base, ovl, table, pol, pol, W)
    assert eb["metric"][node, -1] == 0 and ea["metric"][node, -1] > 0 and (node, len(table) - 1) in changed
    assert not rebased
    rig = Rig("batch")
    try:
        sw = rig.sweep(base)
        st = policy_state(rig.eng, table, pol)
        st.prime(sw)
        rig.sw.close()
        rig.ver += 1
        rig.eng.update_nodes([node], [1], version=rig.ver)
        rig.sw = Sweep(rig.eng, mode="batch")
        rig.sw.run()
        rig.eng.sync()
        assert_update(st, rig.sw, changed, rebased, ea, W)
        st.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- set_policy, overflow
def test_policy_delta_set_policy_and_overflow():
    """set_policy with the same sweep: swapping two classes changes exactly
    the numpy-diff set, a second update reports nothing. Then a link up with
    cap = changes - 1 and cap_rebased = 0: OSPF_E_RANGE with complete counts,
    the state unchanged, the retry complete."""
    base = D.Version(D.base_dbs("unit", 2))
    a, b = D.non_neighbours(base, 5)
    up = D.Version(D.link_up(base.dbs, a, b))
    rng = np.random.default_rng(9)
    table = R.random_table(base.V, rng)
    pol = PR.random_policy(table, rng, classes=3, max_need=4)
    swapped = ([[{0: 1, 1: 0}.get(c, c) for c in cs] for cs in pol[0]], pol[1])
    W = max(base.words, up.words)
    rig = Rig("batch")
    try:
        sw = rig.sweep(base)
        st = policy_state(rig.eng, table, pol)
        st.prime(sw)
        changed, rebased, ea, _ = PD.delta(base, base, table, pol, swapped, W)
        assert 0 < len(changed) < base.V * len(table)
        st.set_policy(PR.flat(swapped[0]), PR.flat(swapped[1]))
        assert_update(st, sw, changed, rebased, ea, W, what="swap")
        rec, _, reb = st.update_policy(sw, cap=0, cap_rebased=0, nh_words=W)
        assert len(rec) == 0 and len(reb) == 0
        # overflow
        changed, rebased, ea, eb = PD.delta(base, up, table, swapped, swapped, W)
        assert len(changed) > 1 and len(rebased) == 2
        sw = rig.sweep(up)
        for cap, cap_reb in ((len(changed) - 1, 0), (len(changed), 1), (len(changed) - 1, 2)):
            with pytest.raises(SelStateOverflow) as ei:
                st.update_policy(sw, cap=cap, cap_rebased=cap_reb, nh_words=W)
            assert ei.value.code == -4
            assert ei.value.n_changes == len(changed) and ei.value.n_rebased == 2
            PD.assert_state(st, eb, W, what="after the overflow")
        assert_update(st, sw, changed, rebased, ea, W, cap=len(changed), what="retry")
        st.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- uniform policy
def test_policy_delta_uniform_policy_equals_the_plain_update():
    dbs = copy.deepcopy(D.base_dbs("weighted", 1))
    for d in dbs:
        d.overloaded = False  # a drained announcer would be filtered: none here
    base = D.Version(dbs)
    a, b = D.non_neighbours(base, 3)
    versions = [base, D.Version(D.link_down(base.dbs, 1)), D.Version(D.link_up(base.dbs, a, b))]
    assert not np.asarray(base.csr["no_transit"]).any()
    table = R.random_table(base.V, np.random.default_rng(5))
    off, nodes = R.csr_table(table)
    pol = PR.uniform_policy(table)
    W = max(v.words for v in versions)
    rig = Rig("batch")
    try:
        sw = rig.sweep(base)
        st = policy_state(rig.eng, table, pol)
        plain = SelState(rig.eng, off, nodes)
        st.prime(sw), plain.prime(sw)
        for v in versions[1:]:
            sw = rig.sweep(v)
            rec, nh, reb = st.update_policy(sw, cap=20000, cap_rebased=8, nh_words=W)
            prec, pnh, preb = plain.update(sw, cap=20000, cap_rebased=8, nh_words=W)
            got = {k: (x[0], x[1], x[6]) for k, x in PD.records(rec, nh).items()}
            assert got == D.records(prec, pnh) and len(got)
            assert sorted(reb.tolist()) == sorted(preb.tolist())
            # links = the root's link counts summed over the set bits
            for (r, p), x in PD.records(rec, nh).items():
                nb = v.nbrs(r)
                c = PR.link_counts(v.csr, r, False)
                assert x[2] == sum(c[k] for k in PR.decode(x[6], nb))
        st.close(), plain.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- contract
def test_policy_delta_contract():
    base = D.Version(D.base_dbs("unit", 0))
    down = D.Version(D.link_down(base.dbs, 0))
    rng = np.random.default_rng(1)
    table = R.random_table(base.V, rng)
    off, nodes = R.csr_table(table)
    pol = PR.random_policy(table, rng)
    pref, mnh = PR.flat(pol[0]), PR.flat(pol[1])
    W = base.words
    rig = Rig("batch")
    try:
        sw = rig.sweep(base)
        eng = rig.eng
        bad_pref = pref.copy()
        bad_pref[5] = 2 ** 31
        for kw in (dict(pref=bad_pref), dict(pref=None, min_nexthop=mnh)):
            with pytest.raises(EngineError) as ei:
                SelState(eng, off, nodes, **kw)
            assert ei.value.code == -1
        st = SelState(eng, off, nodes, pref, mnh)
        plain = SelState(eng, off, nodes)
        assert st.policy and not plain.policy

        def refused(call, code=-1):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == code, ei.value

        refused(lambda: st.update_policy(sw, nh_words=W))  # before prime
        refused(lambda: st.copy_policy([0], W))
        st.prime(sw), plain.prime(sw)
        assert st.device_bytes > plain.device_bytes  # five header columns, the policy columns
        e0, _ = PD.expect(base, table, *pol, W)
        # the wrong kind of state, both ways
        refused(lambda: st.update(sw, nh_words=W))
        refused(lambda: plain.update_policy(sw, nh_words=W))
        refused(lambda: plain.copy_policy([0], W))
        refused(lambda: plain.set_policy(pref, mnh))
        assert len(plain.update(sw, nh_words=W)[0]) == 0
        # the columns' checks at set_policy
        refused(lambda: st.set_policy(bad_pref, mnh))
        refused(lambda: st.set_policy(None, mnh))
        with pytest.raises(ValueError):
            st.set_policy(pref[:-1], mnh)
        refused(lambda: st.copy_policy([base.V], W))
        assert len(st.update_policy(sw, nh_words=W)[0]) == 0  # nothing changed
        # a part of the roots
        part = Sweep(eng, mode="batch", part=0, n_parts=2)
        part.run()
        eng.sync()
        refused(lambda: st.update_policy(part, nh_words=W))
        part.close()
        # an injected error on each new entry point
        for call in (lambda: st.update_policy(sw, nh_words=W), lambda: st.copy_policy([0], W),
                     lambda: st.set_policy(pref, mnh)):
            eng._L.ospf_inject_error(eng._h, 1)
            refused(call, -3)
            PD.assert_state(st, e0, W, what="after an injected error")
        # a stale sweep: the graph moved on (the kernel reads the live graph)
        old = sw
        rig.sw = None
        new = rig.sweep(down)
        refused(lambda: st.update_policy(old, nh_words=W))
        old.close()
        PD.assert_state(st, e0, W, what="after the refused calls")
        changed, rebased, ea, _ = PD.delta(base, down, table, pol, pol, W)
        assert changed
        assert_update(st, new, changed, rebased, ea, W)
        st.close(), plain.close()
        # no prefix
        st = SelState(eng, [0], [], [], [])
        assert st.policy
        st.prime(new)
        rec, nh, reb = st.update_policy(new, nh_words=W)
        assert len(rec) == 0 and len(reb) == 0
        assert st.copy_policy([0, 1], W)["metric"].shape == (2, 0)
        st.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- LinkState
def test_linkstate_policy_delta_on_the_device():
    """track_select_policy / policy_delta / policy_tracked / set_tracked_policy:
    a link event, an attribute change with no event, a node added -> full."""
    from openr_amd.adjdb import AdjDb
    from openr_amd.linkstate import LinkState
    base = D.Version(D.base_dbs("weighted", 1))
    down = D.Version(D.link_down(base.dbs, 1))
    rng = np.random.default_rng(101)
    table = R.random_table(base.V, rng)
    pol = PR.random_policy(table, rng, classes=3, max_need=4)
    swapped = ([[{0: 1, 1: 0}.get(c, c) for c in cs] for cs in pol[0]], pol[1])
    ls = LinkState()
    ls.apply(base.stream)
    ls.track_select_policy(PD.prefixes_by_name(base.names, table, pol))
    e0, _ = PD.expect(base, table, *pol, base.words)
    got = ls.policy_tracked(base.names)
    for k in PR.KEYS + ("installed",):
        assert np.array_equal(got[k], e0[k]), k
    ls.apply(down.stream)
    assert PD.assert_linkstate_delta(ls, base, down, table, pol, pol)
    ls.set_tracked_policy(PD.prefixes_by_name(base.names, table, swapped))
    assert PD.assert_linkstate_delta(ls, down, down, table, pol, swapped)
    d = ls.policy_delta()
    assert len(d["changes"]) == 0 and not d["full"]
    grown = D.link_up(down.dbs + [AdjDb("r-new", [], 999)], "r-new", base.names[3], 2)
    more = D.Version(grown)
    ls.apply(more.stream)
    d = ls.policy_delta()
    assert d["full"] and len(d["changes"]) == 0 and len(d["rebased"]) == 0
    table2 = [[more.names.index(base.names[x]) for x in ann] for ann in table]
    e, _ = PD.expect(more, table2, *swapped, more.words)
    got = ls.policy_tracked(more.names)
    for k in PR.KEYS:
        assert np.array_equal(got[k], e[k]), k
    ovl = D.Version(D.node_overload(grown, 0))
    ls.apply(ovl.stream)
    assert PD.assert_linkstate_delta(ls, more, ovl, table2, swapped, swapped)
    assert ls.counters()["engine_errors"] == 0


@pytest.mark.parametrize("after", [1, 2, 3])
def test_linkstate_policy_delta_degrades_to_host_path(after):
    """An injected device error (sweep create, run, or the update itself) with
    degrade on: the baseline comes off the device and the host path still
    answers the delta."""
    from openr_amd.linkstate import LinkState
    base = D.Version(D.base_dbs("weighted", 1))
    down = D.Version(D.link_down(base.dbs, 1))
    rng = np.random.default_rng(101)
    table = R.random_table(base.V, rng)
    pol = PR.random_policy(table, rng, classes=3, max_need=4)
    ls = LinkState()
    ls.set_degrade(True)
    ls.apply(base.stream)
    ls.track_select_policy(PD.prefixes_by_name(base.names, table, pol))
    ls.apply(down.stream)
    before = ls.counters()["engine_errors"]
    ls.inject_engine_error(after)
    assert PD.assert_linkstate_delta(ls, base, down, table, pol, pol)
    c = ls.counters()
    assert c["engine_errors"] == before + 1 and c["engine_degraded"] == 1
    ls.apply(base.stream)
    assert PD.assert_linkstate_delta(ls, down, base, table, pol, pol)


def test_linkstate_attributes_set_while_the_name_set_differs():
    """A node is added, the attributes change, the node goes again: the name
    set is the tracked one at the next policy_delta, which must still report
    the attribute change (the device columns are replaced there)."""
    from openr_amd.adjdb import AdjDb
    from openr_amd.linkstate import LinkState
    base = D.Version(D.base_dbs("weighted", 1))
    rng = np.random.default_rng(7)
    table = R.random_table(base.V, rng)
    pol = PR.random_policy(table, rng, classes=3, max_need=4)
    swapped = ([[{0: 1, 1: 0}.get(c, c) for c in cs] for cs in pol[0]], pol[1])
    ls = LinkState()
    ls.apply(base.stream)
    ls.track_select_policy(PD.prefixes_by_name(base.names, table, pol))
    more = D.Version(D.link_up(base.dbs + [AdjDb("r-new", [], 999)], "r-new", base.names[3], 2))
    ls.apply(more.stream)
    ls.set_tracked_policy(PD.prefixes_by_name(base.names, table, swapped))
    from openr_amd.adjdb import AdjDbStream
    ls.apply(AdjDbStream.from_dbs(base.dbs + [AdjDb("r-new", [], 999, delete=True)]))
    assert ls.node_names() == base.names
    changed = PD.assert_linkstate_delta(ls, base, base, table, pol, swapped)
    assert 0 < len(changed) < base.V * len(table)
    assert ls.counters()["engine_errors"] == 0
