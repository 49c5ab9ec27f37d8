"""UCMP weights of every root and prefix on the device (ospf_selstate_ucmp /
ospf_selstate_ucmp_copy): the device against ucmp_ref's recursion over
select_ref's expectation (both from the CPU oracle's SPF results; the
recursion itself is proved against the oracle's walk in
test_host_ucmp_all.py), and on the small graphs directly against the oracle's
resolveUcmpWeights per root."""
import copy

import numpy as np
import pytest

import seldelta_ref as D
import select_ref as R
import ucmp_ref as U
from openr_amd.adjdb import AdjDb, create_adjacency
from openr_amd.engine import EngineError, SelState, UcmpOverflow
from openr_amd.linkstate import LinkState
from test_gpu_select_delta import Rig, modes_for
from test_host_ucmp_all import CASES, Case, assert_linkstate, build_graph, oracle_view, tracked

pytestmark = pytest.mark.gpu


def link_keys(version):
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(version.stream)
    return ls.link_keys()


def weights_for(table, seed=0, pool=(2, 3, 4, 6, 9, 10)):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.choice(pool, size=len(a))] for a in table]


def flat(leaf_w):
    return np.array([w for ws in leaf_w for w in ws], np.int64)


def expectation(version, table, leaf_w, hop=False, roots=None):
    consts = U.Consts(version.csr, version.names, version.dbs, link_keys(version), not hop)
    sel = version.expect(table, version.words, not hop, roots)
    return consts, sel, {algo: U.resolve(sel, consts, table, leaf_w, algo) for algo in U.ALGOS}


def assert_view(st, sel, consts, res, roots, what=""):
    adv, status, off, wt = st.ucmp_copy(roots)
    e_adv, e_st, e_off, e_wt = U.copy_expect(sel, consts, res, roots)
    assert np.array_equal(status, e_st), (what, np.argwhere(status != e_st)[:5].tolist())
    assert np.array_equal(adv, e_adv), (what, np.argwhere(adv != e_adv)[:5].tolist())
    assert np.array_equal(off, e_off), what
    assert np.array_equal(wt, e_wt), what


def device_case(version, table, leaf_w, hop=False, modes=("batch",), roots=None, want=None):
    """prime + both algorithms in every mode that takes the graph; -> the
    expectation. want(res of 'prefix') asserts the case is not vacuous."""
    consts, sel, exp = expectation(version, table, leaf_w, hop, roots)
    off, nodes = R.csr_table(table)
    look = list(range(version.V)) if roots is None else list(roots)
    ran = []
    for mode in modes:
        rig = Rig(mode, hop)
        st = None
        try:
            sw = rig.sweep(version)
            if sw is None:
                continue
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            assert st.ucmp_slots == len(consts.dn)
            for algo in U.ALGOS:
                rounds = st.ucmp(algo, flat(leaf_w), consts.S)
                if roots is None:
                    assert rounds == exp[algo][2], (mode, algo)
                assert_view(st, sel, consts, exp[algo], look, (mode, algo))
            st.ucmp("prefix", flat(leaf_w))  # S may be left out
            assert_view(st, sel, consts, exp["prefix"], look, (mode, "prefix, no S"))
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    assert ran, "no sweep mode ran"
    if want:
        want(exp["prefix"])
    return consts, sel, exp


# ---------------------------------------------------------------- 1. table widths
@pytest.mark.parametrize("P", [1, 64, 65])
def test_ucmp_prefix_counts_around_a_wave(P):
    v = D.Version(build_graph(seed=3, parallel=0.6, equal=True, overload=(5,)))
    rng = np.random.default_rng(P)
    main = [i for i, nm in enumerate(v.names) if not nm.startswith("z")]
    table = [sorted(rng.choice(main, size=1 + k % 4, replace=False).tolist()) for k in range(P)]
    if P > 1:
        table[2] = [main[0], main[-1]]  # two announcers far apart, the first of weight zero
    leaf_w = weights_for(table, P)
    if P > 1:
        table[1], leaf_w[1] = [v.names.index("z0")], [5]  # unreachable from the rest
        leaf_w[2][0] = 0  # a zero-weight leaf: VOID for the roots nearest to it only
        table[3], leaf_w[3] = [], []

    def want(res):
        st = res[1]
        if P > 1:
            assert (st[:, 1] == U.NONE).sum() == v.V - 2 and (st[:, 3] == U.NONE).all()
            assert 0 < (st[:, 2] == U.VOID).sum() < v.V - 2
        assert (st == U.OK).any()

    device_case(v, table, leaf_w, want=want)


# ---------------------------------------------------------------- 2. shapes
def named_dbs(links, over=()):
    """links: (a, b, metric a->b, metric b->a, weight a, weight b)"""
    names = sorted({x for l in links for x in l[:2]})
    adjs = {nm: [] for nm in names}
    for i, (a, b, ma, mb, wa, wb) in enumerate(links):
        adjs[a].append(create_adjacency(b, f"{a}-{b}-{i}", f"{b}-{a}-{i}", ma, weight=wa))
        adjs[b].append(create_adjacency(a, f"{b}-{a}-{i}", f"{a}-{b}-{i}", mb, weight=wb))
    return [AdjDb(nm, adjs[nm], i + 1, overloaded=nm in over) for i, nm in enumerate(names)]


def oracle_check(version, table, leaf_w, consts, sel, exp, hop=False):
    """the expectation itself against the oracle's walk, root by root"""
    from oracle import Oracle
    orc = Oracle(version.stream)
    spf = version.spf(not hop)
    for algo in U.ALGOS:
        Wv, st, _ = exp[algo]
        for r in range(version.V):
            for p, ann in enumerate(table):
                best = U.min_cost(spf[version.names[r]], version.names, ann)
                lw = dict(zip(ann, leaf_w[p]))
                if not best or any(lw[a] == 0 for a in best):
                    assert st[r, p] == (U.VOID if best else U.NONE)
                    continue
                got = orc.ucmp(version.names[r], {version.names[a]: lw[a] for a in best}, algo, not hop)
                w, hops = got[version.names[r]]
                mine = U.links(sel, consts, exp[algo], r, p)
                assert st[r, p] == U.OK and int(Wv[r, p]) == w
                assert sorted((version.names[k], wt) for k, c, wt in mine for _ in range(c)) == \
                    sorted((nh, hw) for nh, hw in hops.values())


def test_ucmp_chain_of_12_takes_11_rounds():
    links = [(f"c{i:02d}", f"c{i + 1:02d}", 1, 1, 1 + i % 3, 2) for i in range(11)]
    v = D.Version(named_dbs(links))
    table, leaf_w = [[11], [0], [0, 11]], [[6], [4], [3, 9]]
    consts, sel, exp = device_case(v, table, leaf_w)
    assert exp["prefix"][2] == 11 and exp["adj"][2] == 11
    oracle_check(v, table, leaf_w, consts, sel, exp)


def test_ucmp_parallel_links_and_overloaded_neighbours():
    """r - a by two links of metric 1 and one of metric 2 (c = 2 under link
    metrics, 3 under hop count); o1 overloaded and a leaf, o2 overloaded and on
    no path; t announces beyond a and b; an island announcer."""
    links = [("r", "a", 1, 1, 2, 1), ("r", "a", 1, 1, 3, 1), ("r", "a", 2, 2, 5, 1),
             ("r", "b", 1, 1, 4, 1), ("a", "t", 1, 1, 1, 1), ("b", "t", 1, 1, 2, 1),
             ("b", "t", 1, 1, 3, 1), ("r", "o1", 2, 2, 7, 1), ("o1", "t", 1, 1, 1, 1),
             ("r", "o2", 1, 1, 1, 1), ("o2", "t", 1, 1, 1, 1), ("t", "u", 1, 1, 2, 2),
             ("y0", "y1", 1, 1, 1, 1)]
    v = D.Version(named_dbs(links, over=("o1", "o2")))
    ids = {nm: i for i, nm in enumerate(v.names)}
    table = [[ids["t"]], [ids["o1"], ids["t"]], [ids["r"]], [ids["y0"]], [ids["a"], ids["u"]],
             [ids["o1"]]]
    table = [sorted(a) for a in table]
    leaf_w = [[4], [6, 9], [5], [3], [0, 8], [2]]
    for hop in (False, True):
        consts, sel, exp = device_case(v, table, leaf_w, hop=hop)
        r, a = ids["r"], ids["a"]
        slot = int(consts.dn_off[r]) + R.root_neighbor_ids(v.csr, r).tolist().index(a)
        assert consts.c[slot] == (3 if hop else 2)
        Wv, st, _ = exp["prefix"]
        assert st[r, 2] == U.OK and Wv[r, 2] == 5  # the root announces the prefix itself
        assert st[r, 3] == U.NONE and st[ids["y1"], 3] == U.OK
        assert st[r, 5] == U.OK  # an overloaded neighbour that is the leaf
        assert st[a, 4] == U.VOID and st[ids["u"], 4] == U.OK  # zero-weight leaf: some roots only
        assert len({w for _, _, w in U.links(sel, consts, exp["prefix"], r, 0)}) > 1
        oracle_check(v, table, leaf_w, consts, sel, exp, hop)


@pytest.mark.parametrize("spokes,words", [(33, 2), (129, 5)])
def test_ucmp_wide_roots(spokes, words):
    """A hub of 33 neighbours (two words, the lane path) and one of 129 (five
    words: a prefix per wave, a lane per word), spokes in a ring, extra nodes
    behind the first spokes so that the hub is a transit too."""
    v = D.Version(D.star_dbs(spokes, extra=3))
    assert v.words == words
    ids = {nm: i for i, nm in enumerate(v.names)}
    rng = np.random.default_rng(spokes)
    table = [[ids["x0"]], [ids["hub"]], sorted(ids[f"s{i:04d}"] for i in range(0, spokes, 3)),
             sorted(rng.choice(v.V, size=9, replace=False).tolist()), list(range(v.V))]
    table += [sorted(rng.choice(v.V, size=3, replace=False).tolist()) for _ in range(62)]
    leaf_w = weights_for(table, spokes)
    roots = None if spokes == 33 else sorted({ids["hub"], ids["x0"], ids["x2"], ids["s0000"],
                                              ids["s0064"], ids["s0128"]})
    hub = ids["hub"]
    # the expectation of every root is needed for the recursion; the device is
    # compared on all roots (33) or on a sample (129: the view of 133 x 67)
    consts, sel, exp = expectation(v, table, leaf_w)
    off, nodes = R.csr_table(table)
    for mode in ("batch", "wderive"):
        rig = Rig(mode)
        st = None
        try:
            sw = rig.sweep(v)
            if sw is None:
                continue
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            for algo in U.ALGOS:
                assert st.ucmp(algo, flat(leaf_w), consts.S) == exp[algo][2]
                assert_view(st, sel, consts, exp[algo], roots or list(range(v.V)), (mode, algo))
            break
        finally:
            if st is not None:
                st.close()
            rig.close()
    else:
        raise AssertionError("no sweep mode ran")
    many = [len(U.links(sel, consts, exp["prefix"], hub, p)) for p in range(len(table))]
    assert max(many) > 4  # the hub spreads over several next hops somewhere


def test_ucmp_overflow_status_on_a_diamond():
    """Leaf weights of 2^61 behind a diamond whose arms are two parallel
    links: each arm advertises 2^62, their sum 2^63 leaves i63. Only the
    status is asserted (the reference overflows a signed integer there)."""
    links = [("s", "a", 1, 1, 1, 1), ("s", "b", 1, 1, 1, 1), ("q", "s", 1, 1, 1, 1)]
    links += [("a", "t", 1, 1, 1, 1)] * 2 + [("b", "t", 1, 1, 1, 1)] * 2
    v = D.Version(named_dbs(links))
    ids = {nm: i for i, nm in enumerate(v.names)}
    table, leaf_w = [[ids["t"]], [ids["t"]]], [[1 << 61], [5]]
    consts, sel, exp = expectation(v, table, leaf_w)
    off, nodes = R.csr_table(table)
    rig = Rig("batch")
    st = None
    try:
        assert rig.sweep(v) is not None, "the batch mode takes every graph"
        st = SelState(rig.eng, off, nodes)
        st.prime(rig.sw)
        st.ucmp("prefix", flat(leaf_w))
        _, status, _, _ = st.ucmp_copy(list(range(v.V)))
        want = {"t": U.OK, "a": U.OK, "b": U.OK, "s": U.OVERFLOW, "q": U.OVERFLOW}
        assert {nm: int(status[ids[nm], 0]) for nm in want} == want
        assert (status[:, 1] == U.OK).all()
        assert np.array_equal(status, exp["prefix"][1])
    finally:
        if st is not None:
            st.close()
        rig.close()


# ---------------------------------------------------------------- 3. sweep modes
@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("kind,seed", [("unit", 0), ("weighted", 1)])
def test_ucmp_random_graphs_every_mode(kind, seed, hop):
    base = D.Version(D.base_dbs(kind, seed, 40))
    rng = np.random.default_rng(50 + seed)
    table = [[]] + [[x] for x in range(0, base.V, 5)]
    table += [sorted(rng.choice(base.V, size=k, replace=False).tolist()) for k in (2, 3, 5, 9, 17)]
    leaf_w = weights_for(table, seed)
    leaf_w[-2][1] = 0

    def want(res):
        st = res[1]
        assert (st == U.OK).any() and (st == U.VOID).any() and (st == U.NONE).any()

    device_case(base, table, leaf_w, hop=hop, modes=modes_for(kind, hop), want=want)


# ---------------------------------------------------------------- 4. in-place patch
def test_ucmp_after_link_down_in_place_and_update():
    """One of two equal parallel links taken down in place (ospf_update_links):
    before ospf_selstate_update the state is another graph version's
    (OSPF_E_INVAL); after it the re-run equals the new graph's reference --
    the tight-link counts are derived again from the patched CSR."""
    dbs = build_graph(seed=3, parallel=0.6, equal=True)
    base = D.Version(dbs)
    csr = base.csr
    pick = None
    for u in range(base.V):
        lo, hi = int(csr["row_ptr"][u]), int(csr["row_ptr"][u + 1])
        for e in range(lo, hi - 1):
            if csr["col"][e] == csr["col"][e + 1] and csr["edge_up"][e] and csr["edge_up"][e + 1] \
                    and csr["metric"][e] == csr["metric"][e + 1] and u < csr["col"][e]:
                pick = (u, e)
                break
        if pick:
            break
    assert pick, "this seed must have equal parallel links"
    u, e = pick
    lid, twin = int(csr["link_id"][e]), int(csr["twin"][e])
    key = link_keys(base)[lid]
    after = copy.deepcopy(dbs)
    for end in key.split("|"):
        node, iface = end.split("%")
        for d in after:
            for a in d.adjs:
                if d.name == node and a.if_name == iface:
                    a.overloaded = True
    down = D.Version(after)
    assert down.names == base.names and down.words == base.words
    rng = np.random.default_rng(4)
    table = [[x] for x in range(0, base.V, 3)] + \
        [sorted(rng.choice(base.V, size=4, replace=False).tolist()) for _ in range(6)]
    leaf_w = weights_for(table, 4)
    cb, sb, eb = expectation(base, table, leaf_w)
    ca, sa, ea = expectation(down, table, leaf_w)
    assert (ca.c != cb.c).any() and not np.array_equal(eb["prefix"][0], ea["prefix"][0])
    off, nodes = R.csr_table(table)
    rig = Rig("batch")
    st = None
    try:
        sw = rig.sweep(base)
        st = SelState(rig.eng, off, nodes)
        st.prime(sw)
        st.ucmp("prefix", flat(leaf_w))
        everyone = list(range(base.V))
        assert_view(st, sb, cb, eb["prefix"], everyone, "before")
        rig.ver += 1
        rig.eng.update_links([(lid, 0, int(csr["metric"][e]), int(csr["metric"][twin]))], rig.ver)
        with pytest.raises(EngineError) as ei:  # the state's selection is the old graph's
            st.ucmp("prefix", flat(leaf_w))
        assert ei.value.code == -1
        sw.close()
        from openr_amd.engine import Sweep
        rig.sw = sw = Sweep(rig.eng, mode="batch")
        sw.run()
        rig.eng.sync()
        st.update(sw, cap=base.V * len(table), cap_rebased=base.V, nh_words=base.words)
        with pytest.raises(EngineError) as ei:  # the weights are the old selection's
            st.ucmp_copy([0])
        assert ei.value.code == -1
        for algo in U.ALGOS:
            assert st.ucmp(algo, flat(leaf_w), ca.S) == ea[algo][2]
            assert_view(st, sa, ca, ea[algo], everyone, ("after", algo))
    finally:
        if st is not None:
            st.close()
        rig.close()


# ---------------------------------------------------------------- 5. contract
def test_ucmp_contract():
    v = D.Version(build_graph(seed=2, mmax=6))
    rng = np.random.default_rng(8)
    table = [[x] for x in range(0, v.V, 4)] + \
        [sorted(rng.choice(v.V, size=3, replace=False).tolist()) for _ in range(5)]
    leaf_w = weights_for(table, 8)
    consts, sel, exp = expectation(v, table, leaf_w)
    off, nodes = R.csr_table(table)
    everyone = list(range(v.V))
    rig = Rig("batch")
    st = None
    try:
        sw = rig.sweep(v)
        st = SelState(rig.eng, off, nodes)

        def refused(call, code=-1):
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == code, ei.value

        refused(lambda: st.ucmp("prefix", flat(leaf_w)))  # before prime
        st.prime(sw)
        refused(lambda: st.ucmp_copy([0]))  # before a run
        st.ucmp("adj", flat(leaf_w), consts.S)
        assert_view(st, sel, consts, exp["adj"], everyone)
        neg = flat(leaf_w)
        neg[3] = -1
        refused(lambda: st.ucmp("prefix", neg))
        bad_s = consts.S.copy()
        bad_s[0] = -2
        refused(lambda: st.ucmp("adj", flat(leaf_w), bad_s))
        refused(lambda: st.ucmp("adj", flat(leaf_w)))  # adjacency propagation without S
        refused(lambda: st.ucmp("adj", flat(leaf_w), consts.S[:-1]))
        refused(lambda: st.ucmp_copy([v.V]))
        rig.eng._L.ospf_inject_error(rig.eng._h, 1)
        refused(lambda: st.ucmp("prefix", flat(leaf_w)), -3)
        rig.eng._L.ospf_inject_error(rig.eng._h, 1)
        refused(lambda: st.ucmp_copy(everyone), -3)
        assert_view(st, sel, consts, exp["adj"], everyone, "after the refused calls")
        # the OSPF_E_RANGE retry of the copy
        total = len(U.copy_expect(sel, consts, exp["adj"], everyone)[3])
        assert total > 1
        with pytest.raises(EngineError) as ei:
            st.ucmp_copy(everyone, cap=total - 1)
        assert isinstance(ei.value, UcmpOverflow) and ei.value.code == -4 and ei.value.n_wt == total
        adv, status, o, wt = st.ucmp_copy(everyone, cap=total)
        assert len(wt) == total and int(o[-1]) == total
        # another graph version loaded: the state is the old one's
        rig.sw.close()
        rig.sw = None
        rig.ver += 1
        rig.eng.load(v.csr, version=rig.ver)
        refused(lambda: st.ucmp("prefix", flat(leaf_w)))
        refused(lambda: st.ucmp_copy([0]))
    finally:
        if st is not None:
            st.close()
        rig.close()


# ---------------------------------------------------------------- 6. LinkState
@pytest.mark.parametrize("name", ["parallel-unequal", "overloaded-announcers", "hop-count"])
def test_linkstate_all_sources_ucmp_by_names_equals_the_oracle(name):
    """LinkState.all_sources_ucmp / ucmp_tracked on the device, by node names,
    against the oracle's walk of every root (and against ucmp_ref)."""
    kw, ulm = CASES[name]
    case = Case(build_graph(**kw), kw["seed"])
    ls = tracked(case, ulm, host=False)
    spf, sel, _ = case.mode(ulm)
    for algo in U.ALGOS:
        res = assert_linkstate(ls, case, ulm, algo)
        assert ls.ucmp_info["device"] and ls.ucmp_info["rounds"] == res[2]
        weight, status, off, wt = ls.ucmp_tracked(case.names)
        masks = ls.select_tracked(case.names)[2]
        checked = 0
        for r in range(case.V):
            for p, ann in enumerate(case.table):
                best = U.min_cost(spf[case.names[r]], case.names, ann)
                lw = dict(zip(ann, case.leaf_w[p]))
                if not best or any(lw[a] == 0 for a in best):
                    assert status[r, p] == (U.VOID if best else U.NONE)
                    continue
                want_w, want_hops = oracle_view(case, r, {a: lw[a] for a in best}, algo, ulm)
                e = r * len(case.table) + p
                hops = ls.next_hop_names(case.names[r], masks[r, p], case.csr, case.names)
                mine = dict(zip(hops, wt[int(off[e]):int(off[e + 1])].tolist()))
                assert status[r, p] == U.OK and int(weight[r, p]) == want_w
                assert mine == {case.names[k]: w for k, (_, w) in want_hops.items()}
                checked += 1
        assert checked > case.V
    assert ls.counters()["engine_errors"] == 0


def test_linkstate_all_sources_ucmp_follows_a_link_event():
    """a link down applied to the LinkState (patched into the device graph in
    place), select_delta, then the weights of the new graph"""
    kw, ulm = CASES["parallel-equal"]
    dbs = build_graph(**kw)
    case = Case(dbs, kw["seed"])
    ls = tracked(case, ulm, host=False)
    assert_linkstate(ls, case, ulm, "prefix")
    after = D.link_down(dbs, 3)
    ls.apply(D.Version(after).stream)
    ls.select_delta()
    moved = Case(after, kw["seed"])
    for algo in U.ALGOS:
        assert_linkstate(ls, moved, ulm, algo)
        assert ls.ucmp_info["device"]


def test_linkstate_all_sources_ucmp_degrades_to_the_host_loop(monkeypatch):
    """ODL_STRICT_ENGINE unset, degrading on, an injected device error in the
    engine call: the host loop answers with the same arrays."""
    monkeypatch.delenv("ODL_STRICT_ENGINE", raising=False)
    kw, ulm = CASES["overloaded-interior"]
    case = Case(build_graph(**kw), kw["seed"])
    ls = tracked(case, ulm, host=False)
    ls.set_degrade(True)
    assert_linkstate(ls, case, ulm, "adj")
    assert ls.ucmp_info["device"]
    before = ls.counters()["engine_errors"]
    ls.inject_engine_error(1)
    assert_linkstate(ls, case, ulm, "prefix")
    c = ls.counters()
    assert c["engine_errors"] == before + 1 and c["engine_degraded"] == 1
    assert not ls.ucmp_info["device"]
    assert_linkstate(ls, case, ulm, "adj")  # and stays on the host path
