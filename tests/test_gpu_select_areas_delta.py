"""The multi-area selection kept resident and its delta (ospf_areastate_*,
engine.AreaSelState): calculateUpdate over createRouteForPrefix's multi-area
routes, on the device.

Expected values come from areas_delta_ref: areas_ref.expect before and after an
event, diffed in numpy over the six columns and every area's words; rebased
roots are the global ids of the nodes whose root_neighbor_ids differ in any
area. test_host_select_areas_delta.py checks the same fixtures for being
non-vacuous without a GPU."""
import numpy as np
import pytest

import areas_delta_ref as DR
import areas_ref as AR
import select_ref as R
import seldelta_ref as SR
import selpolicy_ref as PR
from openr_amd.engine import (AreaSelState, Engine, EngineError, SelState, SelStateOverflow,
                              Sweep)
from openr_amd.linkstate import AreasTracker

pytestmark = pytest.mark.gpu

FF = 0xFFFFFFFF


class Refused(Exception):
    """a sweep mode whose contract does not admit a graph (EngineError -4)"""


class Dev:
    """One Engine per area. load(areas) loads the areas whose dict is not the
    loaded one, sweeps them again in `mode` and keeps the other areas' sweeps."""

    def __init__(self, mode="batch", hop=False):
        self.mode, self.hop = mode, hop
        self.engs, self.sws, self.have, self.ver = [], [], [], 0

    def load(self, areas):
        while len(self.engs) < len(areas):
            self.engs.append(Engine())
            self.sws.append(None)
            self.have.append(None)
        for a, ar in enumerate(areas):
            if self.have[a] is ar:
                continue
            self.ver += 1
            self.engs[a].load(ar["csr"], self.ver)
            self.have[a] = ar
            self.resweep(a)
        return list(self.sws)

    def resweep(self, a, hop=None):
        if self.sws[a] is not None:
            self.sws[a].close()
            self.sws[a] = None
        try:
            sw = Sweep(self.engs[a], mode=self.mode, hop_count=self.hop if hop is None else hop)
            self.sws[a] = sw
            sw.run()
            self.engs[a].sync()
        except EngineError as e:
            assert e.code == -4, (self.mode, e)
            raise Refused(self.mode)
        return sw

    def close(self):
        for sw in self.sws:
            if sw is not None:
                sw.close()
        for e in self.engs:
            e.close()


def state(sws, areas, table):
    gnames, gids = AR.union(areas)
    return AreaSelState(sws, gids, len(gnames), *AR.csr_table(table))


def wmax(before, after):
    return tuple(max(x, y) for x, y in zip(DR.words(before), DR.words(after)))


def step(st, dev, before, after, tb, ta, known=None, what=""):
    """load `after`, update, and compare the records, the rebased roots and the
    whole committed state with the numpy diff. -> (changed, rebased, ea)"""
    sws = dev.load(after)
    W = wmax(before, after)
    key = (id(before), id(after), id(tb), id(ta), W)
    if known is None or key not in known:
        d = DR.delta(before, after, tb, ta, W, dev.hop)
        if known is not None:
            known[key] = d + (before, after)  # the versions are kept alive with their ids
    else:
        d = known[key][:4]
    changed, rebased, ea, eb = d
    G, P = ea["metric"].shape
    assert 0 < len(changed) < G * P, what
    rec, nh, reb = st.update(sws, cap=G * P, cap_rebased=G, nh_words=W)
    assert sorted(reb.tolist()) == rebased, what
    assert DR.records(rec, nh) == DR.wanted(after, changed, ea), what
    DR.assert_state(st, after, ea, W, what=what)
    return changed, rebased, ea


# ---------------------------------------------------------------- random areas
@pytest.mark.parametrize("unit,hop,sizes,nb", DR.RANDOM_CASES)
def test_random_areas_every_sweep_mode(unit, hop, sizes, nb):
    vs = DR.random_versions(11 + len(sizes), sizes, nb, unit, hop)
    table = DR.random_table(vs[0])
    modes = ("lds", "derive", "wderive", "batch") if unit or hop else ("wderive", "batch", "wcover")
    known, ran = {}, []
    e0 = AR.expect(vs[0], table, DR.words(vs[0]), hop)[0]
    for mode in modes:
        dev = Dev(mode, hop)
        st = None
        try:
            sws = dev.load(vs[0])
            st = state(sws, vs[0], table)
            st.prime(sws)
            DR.assert_state(st, vs[0], e0, DR.words(vs[0]), what=(mode, "prime"))
            for i, (b, a) in enumerate(zip(vs, vs[1:])):
                step(st, dev, b, a, table, table, known, what=(mode, i))
            assert st.device_bytes() > 0
            ran.append(mode)
        except Refused:
            pass
        finally:
            if st is not None:
                st.close()
            dev.close()
    assert "batch" in ran, ran


# ---------------------------------------------------------------- the 4-node fixtures
def test_four_node_fixtures():
    B_, A_ = 0, 1
    t = [[(3, B_, 0, 0), (3, A_, 0, 0)], [(1, A_, 0, 0)], [(2, B_, 0, 0)]]
    v = [DR.four_nodes(m) for m in (10, 5, 20)]
    dev = Dev()
    try:
        sws = dev.load(v[0])
        st = state(sws, v[0], t)
        st.prime(sws)
        got = st.copy([0], (1, 1))
        # tie: "1" reaches "4" through both areas at 20
        assert got["metric"][0, 0] == 20 and got["areas"][0, 0] == 3 and got["count"][0, 0] == 2
        assert got["nh"][B_][0, 0, 0] == 1 and got["nh"][A_][0, 0, 0] == 1
        # B's links at 5: B wins, A's words become zero
        sws = dev.load(v[1])
        rec, nh, reb = st.update(sws, cap=16, cap_rebased=4, nh_words=(1, 1))
        recs = DR.records(rec, nh)
        #                 metric count links need best areas installed (B words, A words)
        assert recs[0, 0] == (10, 1, 1, 0, 0, 1, 1, (1, 0))
        assert recs[0, 2] == (5, 1, 1, 0, 0, 1, 1, (1, 0))
        # "3" is in B only and "2" in A only: "3" and "4" see B's metric, "2" sees nothing
        assert recs[2, 0] == (5, 1, 1, 0, 0, 1, 1, (2, 0))
        assert {r for r, _ in recs} == {0, 2, 3} and reb.size == 0
        changed, rebased, ea, _ = DR.delta(v[0], v[1], t, t, (1, 1))
        assert recs == DR.wanted(v[1], changed, ea) and not rebased
        DR.assert_state(st, v[1], ea, (1, 1))
        # B's links at 20: A wins, B's words become zero
        sws = dev.load(v[2])
        rec, nh, reb = st.update(sws, cap=16, cap_rebased=4, nh_words=(1, 1))
        recs = DR.records(rec, nh)
        assert recs[0, 0] == (20, 1, 1, 0, 0, 2, 1, (0, 1))
        assert recs[2, 0] == (20, 1, 1, 0, 0, 1, 1, (2, 0))
        assert 1 not in {r for r, _ in recs}
        changed, rebased, ea, _ = DR.delta(v[1], v[2], t, t, (1, 1))
        assert recs == DR.wanted(v[2], changed, ea) and not rebased
        DR.assert_state(st, v[2], ea, (1, 1))
        st.close()
    finally:
        dev.close()


def test_words_of_one_area_only():
    """the six columns stay, one area's next hop moves: the comparison reads
    the words"""
    before, after, table = DR.swap_versions()
    dev = Dev()
    try:
        sws = dev.load(before)
        st = state(sws, before, table)
        st.prime(sws)
        changed, _, ea = step(st, dev, before, after, table, table)
        eb = AR.expect(before, table, DR.words(before))[0]
        assert any(DR.only_one_areas_words(before, eb, ea)[c] for c in changed)
        st.close()
    finally:
        dev.close()


# ---------------------------------------------------------------- strategy edges
def test_wide_root_in_one_area_only():
    """a hub of 5 words in area 0 and a handful of neighbours in area 1: the
    lane-per-word store and compare, the verdict by ballot"""
    before = [DR.area_links(*x) for x in DR.hub_links()]
    after = [DR.area_links(*DR.hub_links(DR.DEAR)[0]), before[1]]
    table = DR.random_table_hub(before)
    assert len(table) > 64
    dev = Dev()
    try:
        sws = dev.load(before)
        assert sws[0].max_nh_words == 5 and sws[1].max_nh_words <= 2
        st = state(sws, before, table)
        st.prime(sws)
        DR.assert_state(st, before, AR.expect(before, table, DR.words(before))[0], DR.words(before))
        changed, rebased, _ = step(st, dev, before, after, table, table)
        g = AR.union(before)[0].index("hub")
        mine = {p for r, p in changed if r == g}
        assert not rebased and 0 < len(mine) < len(table)
        step(st, dev, after, before, table, table)
        st.close()
    finally:
        dev.close()


def test_rebase_in_one_area():
    """a link up to a new neighbour takes the hub from 1 to 2 words in area 0:
    both endpoints are rebased, their cells read back by copy; then the reverse"""
    v0, v1 = DR.rebase_versions()
    table = DR.rebase_table(v0)
    gnames, _ = AR.union(v0)
    ends = sorted(gnames.index(n) for n in ("hub", "x0"))
    dev = Dev()
    try:
        sws = dev.load(v0)
        st = state(sws, v0, table)
        st.prime(sws)
        for b, a in ((v0, v1), (v1, v0)):
            changed, rebased, ea = step(st, dev, b, a, table, table)
            assert rebased == ends and not {r for r, _ in changed} & set(ends)
            DR.assert_state(st, a, ea, wmax(b, a), roots=ends)
        st.close()
    finally:
        dev.close()


def test_node_overload_in_place_in_one_area():
    """Engine.update_nodes on one area's engine and a re-sweep of that area
    only: the drained bit is read from the loaded graph"""
    spec = AR.random_area_links(13, (60, 70), 5, False)
    before = [DR.area_links(*x) for x in spec]
    l1, o1 = spec[1]
    after = [before[0], DR.area_links(l1, DR.toggled(o1, "b03"))]
    table = DR.random_table(before)
    dev = Dev()
    try:
        sws = dev.load(before)
        st = state(sws, before, table)
        st.prime(sws)
        node = before[1]["names"].index("b03")
        assert not np.asarray(before[1]["csr"]["no_transit"])[node]
        dev.ver += 1
        dev.engs[1].update_nodes([node], [1], dev.ver)
        kept = dev.sws[0]
        dev.resweep(1)
        dev.have[1] = after[1]  # what the engine holds now
        step(st, dev, before, after, table, table)
        assert dev.sws[0] is kept
        st.close()
    finally:
        dev.close()


# ---------------------------------------------------------------- attributes, overflow
def test_set_policy_and_overflow():
    vs = DR.random_versions(13, (60, 70), 5, False)
    v, table = vs[0], DR.random_table(vs[0])
    other = DR.other_attrs(table)
    W = DR.words(v)
    dev = Dev()
    try:
        sws = dev.load(v)
        st = state(sws, v, table)
        st.prime(sws)
        changed, rebased, ea, eb = DR.delta(v, v, table, other, W)
        G, P = ea["metric"].shape
        assert 3 < len(changed) < G * P and not rebased
        _, _, _, pref, mnh = AR.csr_table(other)
        st.set_policy(pref, mnh)
        DR.assert_state(st, v, eb, W, what="set_policy commits nothing")
        with pytest.raises(SelStateOverflow) as e:
            st.update(sws, cap=3, cap_rebased=4, nh_words=W)
        assert e.value.code == -4
        assert (e.value.n_changes, e.value.n_rebased) == (len(changed), 0)
        DR.assert_state(st, v, eb, W, what="after an overflow")
        rec, nh, reb = st.update(sws, cap=e.value.n_changes, cap_rebased=0, nh_words=W)
        assert DR.records(rec, nh) == DR.wanted(v, changed, ea) and reb.size == 0
        DR.assert_state(st, v, ea, W)
        rec, nh, reb = st.update(sws, cap=4, cap_rebased=4, nh_words=W)
        assert len(rec) == 0 and reb.size == 0
        st.close()
    finally:
        dev.close()


# ---------------------------------------------------------------- one area
def test_one_area_is_the_policy_state():
    """A = 1: records and copy equal SelState(pref=...).update_policy /
    copy_policy on the same events, best mapped from the entry's position to
    its node id and areas == (metric != INF)."""
    dbs = SR.base_dbs("weighted", 1, 70)
    v = [SR.Version(dbs), SR.Version(SR.metric_bump(SR.link_down(dbs, 5), 9, 3))]
    assert v[0].names == v[1].names
    V = v[0].V
    rng = np.random.default_rng(3)
    table = R.random_table(V, rng)
    pref, mnh = PR.random_policy(table, rng)
    ents = [[(n, 0, pref[p][i], mnh[p][i]) for i, n in enumerate(ann)]
            for p, ann in enumerate(table)]
    off, nodes = R.csr_table(table)
    eng = Engine()
    try:
        def sweep(i):
            eng.load(v[i].csr, i + 1)
            sw = Sweep(eng, mode="batch")
            sw.run()
            eng.sync()
            return sw

        def node_of(best):
            out = np.full(best.shape, FF, np.uint32)
            for p, ann in enumerate(table):
                ok = best[:, p] != FF
                out[ok, p] = np.asarray(ann, np.uint32)[best[ok, p]] if len(ann) else FF
            return out

        sw = sweep(0)
        pol = SelState(eng, off, nodes, PR.flat(pref), PR.flat(mnh))
        ars = AreaSelState([sw], [np.arange(V)], V, *AR.csr_table(ents))
        pol.prime(sw)
        ars.prime([sw])
        sw.close()
        sw = sweep(1)
        W = max(v[0].words, v[1].words)
        prec, pnh, preb = pol.update_policy(sw, cap=V * len(table), cap_rebased=V, nh_words=W)
        arec, anh, areb = ars.update([sw], cap=V * len(table), cap_rebased=V, nh_words=(W,))
        assert 0 < len(prec) < V * len(table)
        assert sorted(preb.tolist()) == sorted(areb.tolist())
        want = {(int(r["root"]), int(r["prefix"])):
                tuple(int(r[k]) for k in ("metric", "count", "links", "need", "best", "installed")) +
                (tuple(pnh[i].tolist()),) for i, r in enumerate(prec)}
        got = {}
        for i, r in enumerate(arec):
            b = int(r["best"])
            b = FF if b == FF else int(table[int(r["prefix"])][b])
            assert int(r["areas"]) == int(r["metric"] != FF)
            got[int(r["root"]), int(r["prefix"])] = \
                (int(r["metric"]), int(r["count"]), int(r["links"]), int(r["need"]), b,
                 int(r["installed"]), tuple(anh[i].tolist()))
        assert got == want
        roots = list(range(V))
        pc, ac = pol.copy_policy(roots, W), ars.copy(roots, (W,))
        for k in ("metric", "count", "links", "need"):
            assert np.array_equal(pc[k], ac[k]), k
        assert np.array_equal(pc["nh"], ac["nh"][0])
        assert np.array_equal(pc["best"], node_of(ac["best"]))
        assert np.array_equal(ac["areas"], (ac["metric"] != FF).astype(np.uint32))
        sw.close()
        pol.close()
        ars.close()
    finally:
        eng.close()


# ---------------------------------------------------------------- the contract
def test_contract_errors_leave_the_state():
    t = [[(3, 0, 0, 0), (3, 1, 0, 0)], [(1, 1, 0, 0)], [(2, 0, 0, 0)]]
    v = DR.four_nodes()
    W = (1, 1)
    e0 = AR.expect(v, t, W)[0]
    dev = Dev()
    extra = []
    try:
        sws = dev.load(v)
        st = state(sws, v, t)

        def refused(code, what, **kw):
            with pytest.raises(EngineError) as e:
                st.update(kw.get("sweeps", sws), cap=16, cap_rebased=4,
                          nh_words=kw.get("nh_words", W))
            assert e.value.code == code, (what, e.value)
            if primed:
                DR.assert_state(st, v, e0, W, what=what)

        primed = False
        refused(-1, "update before prime")
        with pytest.raises(EngineError) as e:
            st.copy([0], W)
        assert e.value.code == -1
        st.prime(sws)
        primed = True
        DR.assert_state(st, v, e0, W)
        refused(-1, "a sweep of another context", sweeps=[sws[1], sws[0]])
        refused(-1, "a short nh_words", nh_words=(1, 0))
        hop = Sweep(dev.engs[1], mode="batch", hop_count=True)
        extra.append(hop)
        hop.run()
        dev.engs[1].sync()
        refused(-1, "mixed metric modes", sweeps=[sws[0], hop])
        dev.engs[1]._L.ospf_inject_error(dev.engs[1]._h, 1)
        refused(-3, "an injected error on the second area's context")
        dev.engs[1]._L.ospf_inject_error(dev.engs[1]._h, 1)
        with pytest.raises(EngineError) as e:
            st.set_policy([1, 1, 1, 1], None)
        assert e.value.code == -3
        DR.assert_state(st, v, e0, W, what="after an injected set_policy")
        # the state works after all of them
        rec, nh, reb = st.update(sws, cap=16, cap_rebased=4, nh_words=W)
        assert len(rec) == 0 and reb.size == 0
        # a sweep made stale by an in-place patch of its area
        dev.engs[0].update_nodes([0], [1], 9)
        refused(-1, "a stale sweep")
        # another V_a: area 1 reloaded with a node more
        five = DR.area_links([("1", "2", 10, 10), ("2", "4", 10, 10), ("4", "5", 1, 1)])
        dev.engs[1].load(five["csr"], 10)
        s1 = Sweep(dev.engs[1], mode="batch")
        s0 = Sweep(dev.engs[0], mode="batch")
        extra += [s0, s1]
        s0.run()
        s1.run()
        dev.engs[0].sync()
        dev.engs[1].sync()
        refused(-1, "another node count", sweeps=[s0, s1])
        # one area's engine closed under the live state
        for sw in extra + dev.sws[1:]:
            sw.close()
        extra.clear()
        dev.sws[1] = None
        dev.engs[1].close()
        with pytest.raises(EngineError) as e:
            st.copy([0], W)
        assert e.value.code == -1
        with pytest.raises(EngineError) as e:
            st.prime([s0, s1])
        assert e.value.code == -1
        assert st.device_bytes() == 0
        st.close()
    finally:
        for sw in extra:
            sw.close()
        dev.close()


# ---------------------------------------------------------------- linkstate.AreasTracker
def test_tracker_on_the_device():
    vs = DR.random_versions(13, (60, 70), 5, False)
    table = DR.random_table(vs[0])
    lss = DR.ls_areas(vs[0], host=False)
    tr = AreasTracker(lss, DR.ls_prefixes(vs[0], table))
    try:
        DR.assert_tracked(tr, vs[0], table)
        for b, a in zip(vs, vs[1:]):
            DR.ls_load(lss, b, a)
            DR.assert_tracker_delta(tr, b, a, table, table, on_device=True)
        other = DR.other_attrs(table)
        tr.set_policy(DR.ls_prefixes(vs[0], other))
        DR.assert_tracker_delta(tr, vs[0], vs[0], table, other, on_device=True)
        d = tr.delta()
        assert d["on_device"] and not d["full"] and len(d["changes"]) == 0
        assert all(ls.counters()["engine_errors"] == 0 for ls in lss)
    finally:
        tr.close()


def test_tracker_rebase_and_full_on_the_device():
    v0, v1 = DR.rebase_versions()
    table = DR.rebase_table(v0)
    lss = DR.ls_areas(v0, host=False)
    tr = AreasTracker(lss, DR.ls_prefixes(v0, table))
    try:
        for b, a in ((v0, v1), (v1, v0)):
            DR.ls_load(lss, b, a)
            DR.assert_tracker_delta(tr, b, a, table, table, on_device=True)
        # a node more in area 1 and new attributes while the name set differs
        _, grown = DR.grown_versions()
        DR.ls_load(lss, [None, None], grown)
        back = DR.other_attrs(table, seed=6)
        tr.set_policy(DR.ls_prefixes(v0, back))
        d = tr.delta()
        assert d["full"] and d["on_device"] and len(d["changes"]) == 0 and d["rebased"].size == 0
        DR.assert_tracked(tr, grown, DR.renamed(v0, grown, back))
        # and the new state answers deltas
        again = DR.other_attrs(table, seed=8)
        tr.set_policy(DR.ls_prefixes(v0, again))
        DR.assert_tracker_delta(tr, grown, grown, DR.renamed(v0, grown, back),
                                DR.renamed(v0, grown, again), on_device=True)
    finally:
        tr.close()


@pytest.mark.parametrize("after", [1, 2, 3])
def test_tracker_degraded_call_still_answers_the_delta(after):
    """an injected device error (sweep create, run, or the update itself): the
    previous result is copied off the device and the host answers the same delta"""
    vs = DR.random_versions(13, (60, 70), 5, False)
    table = DR.random_table(vs[0])
    lss = DR.ls_areas(vs[0], host=False)
    tr = AreasTracker(lss, DR.ls_prefixes(vs[0], table))
    try:
        DR.ls_load(lss, vs[0], vs[1])
        DR.assert_tracker_delta(tr, vs[0], vs[1], table, table, on_device=True)
        lss[-1].inject_engine_error(after)
        DR.ls_load(lss, vs[1], vs[2])
        DR.assert_tracker_delta(tr, vs[1], vs[2], table, table, on_device=False)
        assert sum(ls.counters()["engine_errors"] for ls in lss) >= 1
        DR.ls_load(lss, vs[2], vs[3])  # and stays on the host path
        DR.assert_tracker_delta(tr, vs[2], vs[3], table, table, on_device=False)
    finally:
        tr.close()
