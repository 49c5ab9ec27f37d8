"""The route selections a re-sweep changed, on the device (ospf_selstate_*,
LinkState.track_select / select_delta / select_tracked): the counterpart of
DecisionRouteDb::calculateUpdate (openr/decision/SpfSolver.cpp:24-59) for
ospf_sweep_select's route DB.

Expected values come from the CPU oracle only (seldelta_ref): select_ref.expect
on the graph before and on the graph after, diffed in numpy; rebased roots
from select_ref.root_neighbor_ids. Every case asserts that its expectation has
0 < changed < V * P (the no-event case is 0 by construction). Each event is a
new graph version loaded into the same engine, followed by a new Sweep."""
import numpy as np
import pytest

import select_ref as R
import seldelta_ref as D
from openr_amd.engine import Engine, EngineError, SelState, SelStateOverflow, Sweep
from openr_amd.linkstate import LinkState

pytestmark = pytest.mark.gpu


def modes_for(kind, hop):
    if hop or kind.endswith("unit"):
        return ("lds", "derive", "wderive", "batch")
    return ("wderive", "batch", "wcover")


class Rig:
    """An engine walking through graph versions: load, sweep, run."""

    def __init__(self, mode, hop=False):
        self.eng, self.mode, self.hop, self.ver, self.sw = Engine(), mode, hop, 0, None

    def sweep(self, version):
        """version's graph loaded and swept; None when the mode does not
        take it (EngineError -4, as test_gpu_sweep.py skips it)."""
        if self.sw is not None:
            self.sw.close()
            self.sw = None
        self.ver += 1
        self.eng.load(version.csr, version=self.ver)
        try:
            sw = Sweep(self.eng, mode=self.mode, hop_count=self.hop)
        except EngineError as e:
            assert e.code == -4, (self.mode, e)
            return None
        assert sorted(sw.roots.tolist()) == list(range(version.V))
        sw.run()
        self.eng.sync()
        self.sw = sw
        return sw

    def close(self):
        if self.sw is not None:
            self.sw.close()
        self.eng.close()


def assert_state(st, exp, W, roots=None, what=""):
    roots = list(range(exp[0].shape[0])) if roots is None else list(roots)
    got = st.copy(roots, W)
    for name, g, w in zip(("metric", "count", "nh"), got, exp):
        bad = np.argwhere(g != w[roots])
        assert bad.size == 0, (what, name, bad[:5].tolist())


def assert_update(st, sw, before, after, table, W, hop, *, roots=None, cap=None, what=""):
    """One update against the oracle-derived delta; -> (changed, rebased)."""
    changed, rebased, ea, _ = D.delta(before, after, table, W, not hop, roots)
    rec, nh, reb = st.update(sw, cap=len(changed) + 7 if cap is None else cap,
                             cap_rebased=len(rebased) + 3, nh_words=W)
    got = D.records(rec, nh)
    if roots is not None:  # a sampled expectation: the other roots' records are not judged
        keep = set(roots)
        got = {k: v for k, v in got.items() if k[0] in keep}
        assert sorted(set(reb.tolist()) & keep) == rebased, what
    else:
        assert sorted(reb.tolist()) == rebased, what
    want = D.wanted(changed, ea)
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want))[:8])
    assert got == want, what
    assert_state(st, ea, W, roots, what)
    return changed, rebased


def walk(kind, hop, versions, table, W, vacuous_ok=(), modes=None, checks=None):
    """prime on versions[0], then one update per later version, in every
    mode that takes all of them; -> modes run."""
    off, nodes = R.csr_table(table)
    V, P = versions[0].V, len(table)
    ran = []
    for mode in modes or modes_for(kind, hop):
        rig = Rig(mode, hop)
        st = None
        try:
            sw = rig.sweep(versions[0])
            if sw is None:
                continue
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            assert_state(st, versions[0].expect(table, W, not hop), W, what=(mode, "prime"))
            ok = True
            for i in range(1, len(versions)):
                sw = rig.sweep(versions[i])
                if sw is None:
                    ok = False
                    break
                changed, rebased = assert_update(st, sw, versions[i - 1], versions[i], table, W, hop,
                                                 what=(mode, hop, i))
                if i not in vacuous_ok:
                    assert 0 < len(changed) < V * P, (mode, i, len(changed))
                if checks and i in checks:
                    checks[i](changed, rebased)
            if ok:
                ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    assert ran, "no sweep mode ran"
    return ran


# ---------------------------------------------------------------- 1. random graphs
@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("kind,seed,k_down", [("unit", 0, 0), ("weighted", 1, 1)])
def test_delta_random_graphs_every_mode(kind, seed, k_down, hop):
    """link down, link up again, node overloaded, back; weighted link metrics
    also a metric change that alters only the ECMP set."""
    base = D.Version(D.base_dbs(kind, seed))
    table = R.random_table(base.V, np.random.default_rng(100 + seed))
    assert len(table) > 64 and len(table) % 64
    down = D.Version(D.link_down(base.dbs, 0 if hop else k_down))
    ovl = D.Version(D.node_overload(base.dbs, 0))
    versions, checks = [base, down, base, ovl], {}
    if kind == "weighted" and not hop:
        ecmp = D.Version(D.metric_bump(base.dbs, 75))
        _, _, ea, eb = D.delta(base, ecmp, table, base.words)

        def only_ecmp(changed, rebased):
            assert changed and all(ea[0][r, p] == eb[0][r, p] for r, p in changed)

        versions += [base, ecmp]
        checks[5] = only_ecmp
    ran = walk(kind, hop, versions, table, base.words, checks=checks)
    assert "batch" in ran


# ---------------------------------------------------------------- 2. sparse graph
def test_delta_announcers_disconnected_and_back():
    """sparse-unit: a link down cuts nodes off (entries go to OSPF_DIST_INF /
    0 for the roots that lose their last announcer), the next event brings
    them back."""
    base = D.Version(D.base_dbs("sparse-unit", 0))
    table = R.random_table(base.V, np.random.default_rng(7))
    W = base.words
    eb = base.expect(table, W)
    cut = None
    for k in range(len(D.up_adjs(base.dbs))):  # the first link whose loss unreaches something
        v = D.Version(D.link_down(base.dbs, k))
        ea = v.expect(table, W)
        if ((ea[0] == R.INF) & (eb[0] != R.INF)).any():
            cut = v
            break
    assert cut is not None, "this seed must have a bridge"
    lost = (ea[0] == R.INF) & (eb[0] != R.INF)
    assert (ea[1][lost] == 0).all() and not ea[2][lost].any()

    def went_inf(changed, rebased):
        assert {(int(r), int(p)) for r, p in np.argwhere(lost)} <= changed

    walk("sparse-unit", False, [base, cut, base], table, W, checks={1: went_inf})


# ---------------------------------------------------------------- 3. no event
def test_delta_no_event_reports_nothing():
    base = D.Version(D.base_dbs("weighted", 1))
    table = R.random_table(base.V, np.random.default_rng(3))
    off, nodes = R.csr_table(table)
    rig = Rig("wderive")
    try:
        st = SelState(_loaded(rig, base), off, nodes)
        st.prime(rig.sw)
        order = rig.sw.roots.tolist()
        rig.mode = "batch"  # another plan: the roots' row order may differ
        sw = rig.sweep(base)
        rec, nh, reb = st.update(sw, cap=0, cap_rebased=0, nh_words=base.words)
        assert len(rec) == 0 and len(reb) == 0, (order[:4], sw.roots[:4])
        assert_state(st, base.expect(table, base.words), base.words)
        st.close()
    finally:
        rig.close()


def _loaded(rig, version):
    assert rig.sweep(version) is not None
    return rig.eng


# ---------------------------------------------------------------- 4. rebase
def test_delta_link_up_rebases_both_ends():
    base = D.Version(D.base_dbs("unit", 2))
    a, b = D.non_neighbours(base, 5)
    up = D.Version(D.link_up(base.dbs, a, b))
    table = R.random_table(base.V, np.random.default_rng(9))
    W = max(base.words, up.words)
    ends = sorted([base.names.index(a), base.names.index(b)])

    def both(changed, rebased):
        assert rebased == ends
        assert not any(r in ends for r, _ in changed)

    walk("unit", False, [base, up], table, W, checks={1: both})


def test_delta_rebase_grows_a_root_from_one_word_to_two():
    """A hub with 32 neighbours gains a 33rd: W 1 -> 2 in the shadow buffer's
    own offsets."""
    dbs = D.star_dbs(32, extra=1)
    base = D.Version(dbs)
    up = D.Version(D.link_up(dbs, "hub", "x0", 2))
    hub, x0 = base.names.index("hub"), base.names.index("x0")
    assert len(base.nbrs(hub)) == 32 and len(up.nbrs(hub)) == 33
    assert base.words == 1 and up.words == 2
    table = [[]] + [[v] for v in range(base.V)] + [list(range(base.V))] + \
        [[v, (v + 7) % base.V] if v < (v + 7) % base.V else [(v + 7) % base.V, v]
         for v in range(base.V)]
    assert len(table) > 64

    def both(changed, rebased):
        assert rebased == sorted([hub, x0])

    ran = walk("weighted", False, [base, up, base], table, 2, checks={1: both, 2: both},
               modes=("batch", "wderive"))
    assert "batch" in ran


# ---------------------------------------------------------------- 5. wide roots
def wide_case(dbs, edit, table_of, roots_of=None, modes=("batch", "wderive", "wcover")):
    base = D.Version(dbs)
    after = D.Version(edit(dbs))
    hub = base.names.index("hub")
    table = table_of(base)
    W = base.words
    roots = roots_of(base) if roots_of else None
    off, nodes = R.csr_table(table)
    for mode in modes:
        rig = Rig(mode)
        try:
            sw = rig.sweep(base)
            if sw is None:
                continue
            assert rig.eng.nh_words(hub) == W
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            assert_state(st, base.expect(table, W, True, roots), W, roots)
            sw = rig.sweep(after)
            if sw is None:
                st.close()
                continue
            changed, rebased = assert_update(st, sw, base, after, table, W, False, roots=roots,
                                             cap=4096)
            st.close()
            hubs = [p for r, p in changed if r == hub]
            assert hubs and len(hubs) < len(table) and not rebased
            return W
        finally:
            rig.close()
    raise AssertionError("no sweep mode ran")


def hub_edit(name):
    def edit(dbs):  # the hub's link to one spoke gets dearer: the hub's list stays
        import copy
        out = copy.deepcopy(dbs)
        for d in out:
            for a in d.adjs:
                if {d.name, a.other} == {"hub", name}:
                    a.metric += 5
        return out
    return edit


def test_delta_wide_root():
    """test_gpu_select.py's hub (150 spokes, 5 words): the lane-per-word
    compare, with more than 64 prefixes."""
    from test_gpu_select import hub_stream
    dbs = hub_stream().to_dbs()

    def table_of(v):
        rng = np.random.default_rng(3)
        t = [[]] + [[x] for x in range(v.V)] + [list(range(v.V))]
        for k in (2, 9, 64, 65, 130):
            t.append(sorted(rng.choice(v.V, size=k, replace=False).tolist()))
        return t

    assert wide_case(dbs, hub_edit("s010"), table_of) == 5


def test_delta_star_of_66_words():
    """A star of 2,100 leaves: the hub's 66 words cross the 64-word block in
    the stores and in the compare. The oracle answers for the hub and a
    sample of leaves (2,101 parsed SPF results would take minutes); the other
    roots' records are not judged."""
    dbs = D.star_dbs(2100, ring=False)

    def table_of(v):
        ids = {nm: i for i, nm in enumerate(v.names)}
        t = [[]] + [[ids[f"s{i:04d}"]] for i in range(0, 2100, 30)] + [list(range(v.V))]
        t.append(sorted(ids[f"s{i:04d}"] for i in (10, 40, 2050)))
        return t

    def roots_of(v):
        ids = {nm: i for i, nm in enumerate(v.names)}
        return sorted([ids["hub"]] + [ids[f"s{i:04d}"] for i in (0, 10, 30, 40, 2050, 2099)])

    assert wide_case(dbs, hub_edit("s0030"), table_of, roots_of, modes=("batch", "wderive")) == 66


# ---------------------------------------------------------------- 6. overflow
def test_delta_overflow_leaves_the_state_unchanged():
    base = D.Version(D.base_dbs("unit", 2))
    a, b = D.non_neighbours(base, 5)
    up = D.Version(D.link_up(base.dbs, a, b))
    table = R.random_table(base.V, np.random.default_rng(9))
    W = max(base.words, up.words)
    off, nodes = R.csr_table(table)
    changed, rebased, ea, eb = D.delta(base, up, table, W)
    assert 1 < len(changed) < base.V * len(table) and len(rebased) == 2
    rig = Rig("batch")
    try:
        st = SelState(_loaded(rig, base), off, nodes)
        st.prime(rig.sw)
        sw = rig.sweep(up)
        for cap, cap_reb in ((len(changed) - 1, 2), (len(changed), 1)):
            with pytest.raises(EngineError) as ei:
                st.update(sw, cap=cap, cap_rebased=cap_reb, nh_words=W)
            assert isinstance(ei.value, SelStateOverflow) and ei.value.code == -4
            assert ei.value.n_changes == len(changed) and ei.value.n_rebased == 2
            assert_state(st, eb, W, what="after the overflow")
        rec, nh, reb = st.update(sw, cap=len(changed), cap_rebased=2, nh_words=W)
        assert D.records(rec, nh) == D.wanted(changed, ea) and sorted(reb.tolist()) == rebased
        assert_state(st, ea, W)
        st.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- 7. contract
def test_delta_contract():
    base = D.Version(D.base_dbs("unit", 0))
    down = D.Version(D.link_down(base.dbs, 0))
    other = D.Version(D.base_dbs("unit", 2, 71))
    table = R.random_table(base.V, np.random.default_rng(1))
    off, nodes = R.csr_table(table)
    W = base.words
    rig = Rig("batch")
    try:
        eng = _loaded(rig, base)
        for boff, bnodes in (([0, 2], [7, 7]), ([0, 1], [base.V]), ([0, 2, 1, 3], [1, 2, 3])):
            with pytest.raises(EngineError) as ei:
                SelState(eng, boff, bnodes)
            assert ei.value.code == -1
        st = SelState(eng, off, nodes)
        for call in (lambda: st.update(rig.sw, nh_words=W), lambda: st.copy([0], W)):
            with pytest.raises(EngineError) as ei:  # before prime
                call()
            assert ei.value.code == -1
        st.prime(rig.sw)
        eb = base.expect(table, W)
        # a sweep of another V
        sw = rig.sweep(other)
        with pytest.raises(EngineError) as ei:
            st.update(sw, nh_words=other.words)
        assert ei.value.code == -1
        # a part of the roots
        sw = rig.sweep(down)
        part = Sweep(rig.eng, mode="batch", part=0, n_parts=2)
        part.run()
        rig.eng.sync()
        with pytest.raises(EngineError) as ei:
            st.update(part, nh_words=W)
        assert ei.value.code == -1
        part.close()
        # an injected device error
        rig.eng._L.ospf_inject_error(rig.eng._h, 1)
        with pytest.raises(EngineError) as ei:
            st.update(sw, nh_words=W)
        assert ei.value.code == -3
        assert_state(st, eb, W, what="after the refused calls")
        changed, _ = assert_update(st, sw, base, down, table, W, False)
        assert changed
        st.close()
        # nh_words below the sweep's widest root
        dbs = D.star_dbs(40)
        wide = D.Version(dbs)
        sw = rig.sweep(wide)
        st = SelState(rig.eng, [0, 1], [0])
        st.prime(sw)
        with pytest.raises(EngineError) as ei:
            st.update(sw, nh_words=1)
        assert ei.value.code == -1
        assert len(st.update(sw, nh_words=2)[0]) == 0
        st.close()
        # no prefix: OSPF_OK with zero counts
        st = SelState(rig.eng, [0], [])
        st.prime(sw)
        rec, nh, reb = st.update(sw, nh_words=2)
        assert len(rec) == 0 and len(reb) == 0
        st.close()
    finally:
        rig.close()


# ---------------------------------------------------------------- 8. LinkState
def by_names(ls, before, after, table, use_link_metric=True):
    """select_delta of `ls` == the oracle-derived delta before -> after."""
    d = ls.select_delta()
    assert not d["full"]
    W = d["nh"].shape[1]
    assert W == after.words
    changed, rebased, ea, _ = D.delta(before, after, table, max(W, before.words), use_link_metric)
    ea = (ea[0], ea[1], ea[2][:, :, :W])
    assert sorted(d["rebased"].tolist()) == rebased
    assert D.records(d["changes"], d["nh"]) == D.wanted(changed, ea)
    if rebased:
        got = ls.select_tracked([after.names[r] for r in rebased])
        for g, w in zip(got, ea):
            assert np.array_equal(g, w[rebased])
    return changed


def test_linkstate_select_delta():
    base = D.Version(D.base_dbs("weighted", 1))
    down = D.Version(D.link_down(base.dbs, 1))
    table = R.random_table(base.V, np.random.default_rng(101))
    ls = LinkState()
    ls.apply(base.stream)
    ls.track_select(D.prefixes_by_name(base.names, table))
    got = ls.select_tracked(base.names)
    for g, w in zip(got, base.expect(table, base.words)):
        assert np.array_equal(g, w)
    ls.apply(down.stream)
    assert by_names(ls, base, down, table)
    # a node added: ids renumbered -> full, then deltas again
    from openr_amd.adjdb import AdjDb
    a = base.names[3]
    grown = D.link_up(down.dbs + [AdjDb("r-new", [], 999)], "r-new", a, 2)
    more = D.Version(grown)
    assert more.V == base.V + 1
    ls.apply(more.stream)
    d = ls.select_delta()
    assert d["full"] and len(d["changes"]) == 0 and len(d["rebased"]) == 0
    table2 = [[more.names.index(base.names[x]) for x in ann] for ann in table]
    got = ls.select_tracked(more.names)
    for g, w in zip(got, more.expect(table2, more.words)):
        assert np.array_equal(g, w)
    ovl = D.Version(D.node_overload(grown, 0))
    ls.apply(ovl.stream)
    assert by_names(ls, more, ovl, table2)
    assert ls.counters()["engine_errors"] == 0


@pytest.mark.parametrize("after", [1, 2, 3])
def test_linkstate_select_delta_degrades_to_host_path(after):
    """An injected device error (sweep create, run or the update itself: the
    link event is patched into the device graph in place, so no load comes
    first) with degrade on: the baseline comes off the device and the host
    path answers with the same delta."""
    base = D.Version(D.base_dbs("weighted", 1))
    down = D.Version(D.link_down(base.dbs, 1))
    table = R.random_table(base.V, np.random.default_rng(101))
    ls = LinkState()
    ls.set_degrade(True)
    ls.apply(base.stream)
    ls.track_select(D.prefixes_by_name(base.names, table))
    ls.apply(down.stream)
    before = ls.counters()["engine_errors"]
    ls.inject_engine_error(after)
    assert by_names(ls, base, down, table)
    c = ls.counters()
    assert c["engine_errors"] == before + 1 and c["engine_degraded"] == 1
    ls.apply(base.stream)
    assert by_names(ls, down, base, table)
