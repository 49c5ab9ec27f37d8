"""Device-side route selection across several areas
(ospf_areas_select_policy*): createRouteForPrefix's multi-area rule
(openr/decision/SpfSolver.cpp:197-458) for every node of the union of the
areas and every prefix, one sweep per area.

Expected values come from areas_ref.expect: the rule restated in Python over
the CPU oracle's SPF results of every area and the CSR columns, never the
engine's rows or its packed key."""
import functools

import numpy as np
import pytest
import torch

import areas_ref as AR
import select_ref as R
import selpolicy_ref as PR
from graphs import metric_graph
from openr_amd.adjdb import AdjDbStream
from openr_amd.engine import (Engine, EngineError, Sweep, select_policy_areas,
                              select_policy_areas_dev)
from openr_amd.linkstate import LinkState, all_areas_select_policy
from oracle import Oracle, parse_spf_text

pytestmark = pytest.mark.gpu

FF = 0xFFFFFFFF
GUARD = 16  # poisoned words kept before and after every device output
HDR = AR.KEYS


def area_of(links, overloaded=(), hop=False):
    """{names, csr, spf, eng} of one area's explicit graph"""
    st = AdjDbStream.from_dbs(metric_graph(links, overloaded))
    ls = LinkState()
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    orc = Oracle(st)
    spf = {r: parse_spf_text(orc.spf_text(r, not hop)) for r in names}
    eng = Engine()
    eng.load(csr)
    return dict(names=names, csr=csr, spf=spf, eng=eng)


def close(areas):
    for a in areas:
        a["eng"].close()


def run_sweeps(areas, mode, hop=False):
    """one run sweep per area in `mode`, or None when an area's contract does
    not admit it (EngineError -4, as test_gpu_sweep.py skips it)"""
    sws = []
    try:
        for a in areas:
            sw = Sweep(a["eng"], mode=mode, hop_count=hop)
            sws.append(sw)
            sw.run()
            a["eng"].sync()
    except EngineError as e:
        for sw in sws:
            sw.close()
        assert e.code == -4, (mode, e)
        return None
    return sws


def select(areas, sws, table, **kw):
    _, gids = AR.union(areas)
    G = len(AR.union(areas)[0])
    return select_policy_areas(sws, gids, G, *AR.csr_table(table), **kw)


def check(areas, table, modes, hop=False, facts_wanted=()):
    ran = []
    want = {}
    for mode in modes:
        sws = run_sweeps(areas, mode, hop)
        if sws is None:
            continue
        try:
            W = tuple(max(1, s.max_nh_words) for s in sws)
            if W not in want:
                want[W] = AR.expect(areas, table, W, hop)
            exp, facts = want[W]
            for k in facts_wanted:
                assert facts[k] > 0, (k, facts)
            AR.assert_equal(select(areas, sws, table), exp, ctx=(mode, hop))
            ran.append(mode)
        finally:
            for sw in sws:
                sw.close()
    assert ran, "no sweep mode ran"
    return want


# ---------------------------------------------------------------- random areas
def random_areas(seed, sizes, n_border, unit, hop=False, p=0.1):
    """AR.random_area_links as loaded areas"""
    return [area_of(links, over, hop)
            for links, over in AR.random_area_links(seed, sizes, n_border, unit, p)]


random_entries = AR.random_entries


CORNERS = ("tie", "shorter_area", "cross_area", "skipped_area", "single_area_root", "filtered",
           "all_drained", "drained_in_one_area", "need_from_loser", "withheld", "best_outside",
           "unreached_best")


@pytest.mark.parametrize("unit,hop,sizes,nb", [(True, False, (60, 70), 5), (False, False, (60, 70), 4),
                                               (False, True, (45, 50, 40), 6),
                                               (False, False, (45, 50, 40), 3)])
def test_random_areas_every_sweep_mode(unit, hop, sizes, nb):
    areas = random_areas(11 + len(sizes), sizes, nb, unit, hop)
    try:
        for a in areas:
            assert 40 <= len(a["names"]) <= 70 and np.asarray(a["csr"]["no_transit"]).any()
        table = random_entries(areas, np.random.default_rng(5))
        modes = ("lds", "derive", "wderive", "batch") if unit or hop else ("wderive", "batch", "wcover")
        check(areas, table, modes, hop, CORNERS)
    finally:
        close(areas)


# ---------------------------------------------------------------- one area
@pytest.mark.parametrize("hop", [False, True])
def test_one_area_is_the_policy_selection(hop):
    """A = 1: every output equals Sweep.select_policy word for word, rows by
    node id and best mapped from the entry's position to its node id."""
    st = R.graph("weighted", 1, 70)[0]
    ls = LinkState()
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    assert np.asarray(csr["no_transit"]).any()
    eng = Engine()
    eng.load(csr)
    try:
        rng = np.random.default_rng(3)
        table = R.random_table(70, rng)
        pref, mnh = PR.random_policy(table, rng)
        ents = [[(n, 0, pref[p][i], mnh[p][i]) for i, n in enumerate(ann)]
                for p, ann in enumerate(table)]
        sw = Sweep(eng, mode="batch", hop_count=hop)
        try:
            sw.run()
            eng.sync()
            off, nodes = R.csr_table(table)
            old = sw.select_policy(off, nodes, PR.flat(pref), PR.flat(mnh))
            got = select_policy_areas([sw], [np.arange(70)], 70, *AR.csr_table(ents))
            for k in ("metric", "count", "links", "need"):
                b = np.zeros_like(old[k])
                b[sw.roots] = old[k]
                assert np.array_equal(got[k], b), k
            b = np.zeros_like(old["nh"])
            b[sw.roots] = old["nh"]
            assert np.array_equal(got["nh"][0], b)
            best = np.full((70, len(table)), FF, np.uint32)
            for p, ann in enumerate(table):
                col = got["best"][:, p]
                ok = col != FF
                best[ok, p] = np.asarray(ann, np.uint32)[col[ok]] if len(ann) else FF
            b = np.zeros_like(old["best"])
            b[sw.roots] = old["best"]
            assert np.array_equal(best, b)
            assert np.array_equal(got["areas"], (got["metric"] != FF).astype(np.uint32))
        finally:
            sw.close()
    finally:
        eng.close()


# ---------------------------------------------------------------- the 4-node fixtures
def four_nodes(b_metric=10):
    """MultiAreaBestPathCalculation's graphs (DecisionTest.cpp): area "A" is
    1 - 2 - 4, area "B" 1 - 3 - 4; in name order B is area 0"""
    b = area_of([("1", "3", b_metric, b_metric), ("3", "4", b_metric, b_metric)])
    a = area_of([("1", "2", 10, 10), ("2", "4", 10, 10)])
    return [b, a]


B_, A_ = 0, 1


def test_four_node_fixtures():
    n1, n2, n3, n4 = range(4)
    areas = four_nodes()
    try:
        sws = run_sweeps(areas, "batch")
        try:
            # ADDR[1] .. ADDR[4], one area each
            t = [[(n1, A_, 0, 0)], [(n2, A_, 0, 0)], [(n3, B_, 0, 0)], [(n4, B_, 0, 0)]]
            got = select(areas, sws, t)
            assert got["metric"].tolist() == [[0, 10, 10, 20], [10, 0, FF, FF], [FF, FF, 0, 10],
                                              [20, 10, 10, 0]]
            assert got["areas"].tolist() == [[2, 2, 1, 1], [2, 2, 0, 0], [0, 0, 1, 1], [2, 2, 1, 1]]
            assert got["nh"][B_][:, :, 0].tolist() == [[0, 0, 1, 1], [0, 0, 0, 2], [0, 0, 1, 0]]
            assert got["nh"][A_][:, :, 0].tolist() == [[0, 1, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0]]
            AR.assert_equal(got, AR.expect(areas, t, (1, 1))[0])
            # "1" originates ADDR[1] into B too: 3 reaches it in B, 4 through
            # both areas at metric 20
            t[0] = [(n1, B_, 0, 0), (n1, A_, 0, 0)]
            got = select(areas, sws, t)
            assert got["metric"][:, 0].tolist() == [0, 10, 10, 20]
            assert got["areas"][:, 0].tolist() == [3, 2, 1, 3]
            assert got["count"][:, 0].tolist() == [2, 1, 1, 2]
            assert got["links"][:, 0].tolist() == [0, 1, 1, 2]
            assert got["nh"][B_][2, 0, 0] == 1 and got["nh"][A_][2, 0, 0] == 1
            exp, facts = AR.expect(areas, t, (1, 1))
            assert facts["tie"] > 0
            AR.assert_equal(got, exp)
        finally:
            for sw in sws:
                sw.close()
    finally:
        close(areas)
    # the shorter area: B's links cost 3, "4" announces in both areas
    areas = four_nodes(3)
    try:
        sws = run_sweeps(areas, "batch")
        try:
            t = [[(n4, B_, 0, 0), (n4, A_, 0, 0)]]
            got = select(areas, sws, t)
            assert got["metric"][:, 0].tolist() == [6, 10, 3, 0]
            assert got["areas"][:, 0].tolist() == [1, 2, 1, 3]
            assert got["nh"][A_][0, 0, 0] == 0 and got["nh"][B_][0, 0, 0] == 1
            exp, facts = AR.expect(areas, t, (1, 1))
            assert facts["shorter_area"] > 0
            AR.assert_equal(got, exp)
        finally:
            for sw in sws:
                sw.close()
    finally:
        close(areas)


# ---------------------------------------------------------------- strategy edges
@functools.lru_cache(maxsize=None)
def hub_areas():
    """area 0: a hub with 140 spokes (5 next-hop words: the lane-per-word
    path), two of them drained; area 1: the hub is a leaf behind one spoke of
    a small ring that shares three spokes with area 0"""
    sp = [f"s{i:03d}" for i in range(140)]
    l0 = [("hub", s, 1 + i % 3, 1 + i % 2) for i, s in enumerate(sp)]
    l0 += [(sp[i], sp[i + 1], 2, 2) for i in range(0, 60, 2)]
    l1 = [("hub", "s005", 2, 2), ("s005", "s007", 1, 1), ("s007", "s009", 1, 3), ("s009", "t0", 1, 1),
          ("t0", "s005", 4, 1), ("t0", "t1", 1, 1)]
    # 60 more spokes shared with area 0, on a ladder behind t0 / t1
    l1 += [("t0" if i % 2 else "t1", sp[i], 1 + i % 4, 1 + i % 3) for i in range(10, 72)]
    l1 += [(sp[i], sp[i + 1], 1, 2) for i in range(10, 71, 3)]
    return [area_of(l0, ("s003", "s009")), area_of(l1, ("s007", "s020"))]


def spread_prefix(areas, k, rng):
    """k entries alternating between the two areas over their shared nodes
    (every shared node in both areas first), ascending in (node, area)"""
    gnames, gids = AR.union(areas)
    shared = sorted(set(gids[0].tolist()) & set(gids[1].tolist()))
    ents = [(g, a) for g in shared for a in (0, 1)][:k]
    assert len(ents) == k and sum(a for _, a in ents) >= k // 2 - 1
    return [(n, a, int(rng.integers(2)), int(rng.integers(5))) for n, a in ents]


def test_wide_root_in_one_area_leaf_in_the_other():
    areas = hub_areas()
    gnames, gids = AR.union(areas)
    hub0, hub1 = areas[0]["names"].index("hub"), areas[1]["names"].index("hub")
    rng = np.random.default_rng(9)
    table = random_entries(areas, rng, sizes=(0, 1, 2, 8, 9, 64, 65, 130), singles=12)
    # long prefixes with half their entries in each area: the wave walks of a
    # wide root across a 64-entry step, in both areas
    table += [spread_prefix(areas, k, rng) for k in (8, 9, 64, 65, 130)]
    sws = run_sweeps(areas, "batch")
    try:
        assert sws[0].max_nh_words == 5 and sws[1].max_nh_words <= 2
        W1 = max(1, sws[1].max_nh_words)
        exp, facts = AR.expect(areas, table, (5, W1))
        for k in ("tie", "shorter_area", "cross_area", "filtered"):
            assert facts[k] > 0, (k, facts)
        g = gnames.index("hub")
        assert (exp["areas"][g] == 3).any() and exp["nh"][0][hub0].any() and exp["nh"][1][hub1].any()
        AR.assert_equal(select(areas, sws, table), exp)
        # wider outputs than the roots need: the padding is written too
        got = select(areas, sws, table, nh_words=(8, 3))
        wide, _ = AR.expect(areas, table, (8, 3))
        AR.assert_equal(got, wide)
    finally:
        for sw in sws:
            sw.close()


@pytest.mark.parametrize("P", [63, 64, 65])
def test_chunk_tail_and_pref_edges(P):
    """P on both sides of a wave's 64 prefixes; pref 0 beside 2^31 - 1 in one
    prefix; an unreached entry (the island) holding the best pref."""
    areas = random_areas(4, (40, 45), 3, False)
    try:
        gnames, gids = AR.union(areas)
        rng = np.random.default_rng(P)
        table = random_entries(areas, rng, sizes=(8, 9, 64, 65), singles=P - 4)
        z = gnames.index("mz0")
        top = 2 ** 31 - 1
        some = sorted((int(g), a) for a, gs in enumerate(gids) for g in gs[:6])
        table[4] = [(n, a, top if i % 2 else 0, i % 3) for i, (n, a) in enumerate(some)]
        table[5] = sorted([(z, 0, 0, 2)] + [(n, a, top, 1) for n, a in some if n != z])
        table = table[:P]
        assert len(table) == P
        want = check(areas, table, ("batch",), False, ("unreached_best",))
        exp = next(iter(want.values()))[0]
        assert (exp["best"][:, 5] != FF).any()
    finally:
        close(areas)


# ---------------------------------------------------------------- stores
def dev_buffer(words):
    buf = torch.full((words + 2 * GUARD,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
    return buf


def test_dev_call_writes_every_wanted_word_and_no_other():
    areas = hub_areas()
    gnames, gids = AR.union(areas)
    G = len(gnames)
    table = random_entries(areas, np.random.default_rng(2), sizes=(0, 3, 9, 65), singles=4)
    P = len(table)
    cols = AR.csr_table(table)
    sws = run_sweeps(areas, "batch")
    try:
        W = (6, 2)
        exp, _ = AR.expect(areas, table, W)
        sizes = {k: G * P for k in HDR}
        sizes.update({("nh", a): len(areas[a]["names"]) * P * W[a] for a in range(2)})
        poison = np.uint32(0xA5A5A5A5)
        for skip in [None] + list(sizes):
            bufs = {k: dev_buffer(n) for k, n in sizes.items() if k != skip}
            ptr = lambda k: bufs[k].data_ptr() + 4 * GUARD if k in bufs else 0  # noqa: E731
            select_policy_areas_dev(sws, gids, G, *cols, W,
                                    **{f"d_{k}": ptr(k) for k in HDR},
                                    d_nh=[ptr(("nh", 0)), ptr(("nh", 1))])
            torch.cuda.synchronize()
            for k, b in bufs.items():
                h = b.cpu().numpy().view(np.uint32)
                assert (h[:GUARD] == poison).all() and (h[-GUARD:] == poison).all(), (skip, k)
                body = h[GUARD:-GUARD]
                w = exp["nh"][k[1]] if isinstance(k, tuple) else exp[k]
                assert np.array_equal(body, w.reshape(-1)), (skip, k)
    finally:
        for sw in sws:
            sw.close()


# ---------------------------------------------------------------- contract errors
def test_contract_errors_write_nothing():
    areas = four_nodes()
    try:
        _, gids = AR.union(areas)
        sws = run_sweeps(areas, "batch")
        hop = Sweep(areas[1]["eng"], mode="batch", hop_count=True)
        hop.run()
        fresh = Sweep(areas[1]["eng"], mode="batch", defer=True, hip_graph=False)
        part = Sweep(areas[1]["eng"], mode="batch", part=0, n_parts=2)
        part.run()
        areas[1]["eng"].sync()
        try:
            good = [[(0, 0, 0, 0), (0, 1, 0, 0), (3, 1, 1, 2)]]
            c = AR.csr_table(good)
            tab = lambda t: AR.csr_table(t)  # noqa: E731
            bad_gid = [gids[0], np.array([0, 3, 1], np.uint32)]
            cases = {
                "no areas": dict(sweeps=[], gids=[]),
                "null sweep": dict(sweeps=[sws[0], None]),
                "not run": dict(sweeps=[sws[0], fresh]),
                "part": dict(sweeps=[sws[0], part]),
                "mixed modes": dict(sweeps=[sws[0], hop]),
                "gid order": dict(gids=bad_gid),
                "gid range": dict(gids=[gids[0], np.array([0, 1, 4], np.uint32)]),
                "unheld id": dict(G=5),
                "absent node": dict(table=tab([[(1, 0, 0, 0)]])),
                "entry order": dict(table=tab([[(0, 1, 0, 0), (0, 0, 0, 0)]])),
                "entry twice": dict(table=tab([[(0, 1, 0, 0), (0, 1, 0, 0)]])),
                "area range": dict(table=tab([[(0, 2, 0, 0)]])),
                "pref range": dict(table=tab([[(0, 0, 2 ** 31, 0)]])),
                "null pref": dict(table=c[:3] + (None, None)),
                "nh_words": dict(nh_words=(1, 0)),
            }
            for what, kw in cases.items():
                buf = dev_buffer(64)
                p = buf.data_ptr() + 4 * GUARD
                s = kw.get("sweeps", sws)
                with pytest.raises(EngineError) as e:
                    select_policy_areas_dev(s, kw.get("gids", gids), kw.get("G", 4),
                                            *kw.get("table", c), kw.get("nh_words", (1, 1)),
                                            d_metric=p, d_areas=p, d_nh=[p, p])
                assert e.value.code == -1, (what, e.value)
                torch.cuda.synchronize()
                assert (buf.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all(), what
            with pytest.raises(EngineError) as e:
                select_policy_areas(sws * 17, gids * 17, 4, *c)
            assert e.value.code == -1
            buf = dev_buffer(64)
            p = buf.data_ptr() + 4 * GUARD
            with pytest.raises(EngineError) as e:
                select_policy_areas_dev(sws * 17, gids * 17, 4, *c, (1,) * 34, d_metric=p, d_best=p,
                                        d_nh=[p] * 34)
            assert e.value.code == -1
            torch.cuda.synchronize()
            assert (buf.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
            # no prefix: OSPF_OK, nothing written
            buf = dev_buffer(64)
            select_policy_areas_dev(sws, gids, 4, [0], [], [], [], None, (1, 1),
                                    d_metric=buf.data_ptr() + 4 * GUARD)
            torch.cuda.synchronize()
            assert (buf.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
            # a sweep made stale by an in-place patch
            assert select(areas, sws, good)["metric"][3, 0] == 20
            areas[0]["eng"].update_nodes([0], [1], 2)
            with pytest.raises(EngineError) as e:
                select(areas, sws, good)
            assert e.value.code == -1 and "changed" in str(e.value)
            buf = dev_buffer(64)
            p = buf.data_ptr() + 4 * GUARD
            with pytest.raises(EngineError) as e:
                select_policy_areas_dev(sws, gids, 4, *c, (1, 1), d_metric=p, d_links=p, d_nh=[p, p])
            assert e.value.code == -1 and "changed" in str(e.value)
            torch.cuda.synchronize()
            assert (buf.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
        finally:
            for sw in sws + [hop, fresh, part]:
                sw.close()
    finally:
        close(areas)


# ---------------------------------------------------------------- the LinkState call
def ls_area(name, links, overloaded=()):
    """an area as a LinkState on the device, with what areas_ref reads of it"""
    st = AdjDbStream.from_dbs(metric_graph(links, overloaded))
    ls = LinkState(area=name)
    ls.set_degrade(True)
    ls.apply(st)
    orc = Oracle(st)
    names = ls.node_names()
    return dict(name=name, ls=ls, names=names, csr=ls.csr(),
                spf={r: parse_spf_text(orc.spf_text(r, True)) for r in names})


def ls_policy(areas, table):
    gnames, _ = AR.union(areas)
    return {f"p{p}": [(gnames[n], areas[a]["name"], 1000 - r, 0, 0, mn or None)
                      for n, a, r, mn in ents] for p, ents in enumerate(table)}


def ls_check(areas, table, on_device):
    got = all_areas_select_policy([a["ls"] for a in areas], ls_policy(areas, table))
    W = [x.shape[2] for x in got["nh"]]
    exp, facts = AR.expect(areas, table, W)
    assert got["on_device"] == on_device and got["names"] == AR.union(areas)[0]
    AR.assert_equal(got, exp)
    assert np.array_equal(got["installed"], exp["installed"])
    return exp, facts


def ls_areas(seed=20):
    spec = AR.random_area_links(seed, (30, 34), 3, False, p=0.15)
    areas = [ls_area(f"a{i}", links, over) for i, (links, over) in enumerate(spec)]
    table = AR.random_entries(areas, np.random.default_rng(8), sizes=(0, 1, 2, 3, 9, 20, 65),
                              singles=24)
    return spec, areas, table


def test_linkstate_call_on_the_device_and_after_a_link_down():
    spec, areas, table = ls_areas()
    exp, facts = ls_check(areas, table, True)
    for k in ("tie", "shorter_area", "cross_area", "skipped_area"):
        assert facts[k] > 0, (k, facts)
    sweeps = [a["ls"].sweep_stats()["sweeps"] for a in areas]
    assert sweeps == [1, 1]
    ls_check(areas, table, True)  # nothing moved: no new sweep
    assert [a["ls"].sweep_stats()["sweeps"] for a in areas] == [1, 1]
    # LINK DOWN in area 1: a border node's first link there goes away
    links, over = spec[1]
    gone = next(ln for ln in links if ln[0] == "b00")
    st = AdjDbStream.from_dbs(metric_graph([ln for ln in links if ln is not gone], over))
    areas[1]["ls"].apply(st)
    orc = Oracle(st)
    areas[1]["csr"] = areas[1]["ls"].csr()
    assert areas[1]["ls"].node_names() == areas[1]["names"]
    areas[1]["spf"] = {r: parse_spf_text(orc.spf_text(r, True)) for r in areas[1]["names"]}
    after, _ = ls_check(areas, table, True)
    assert [a["ls"].sweep_stats()["sweeps"] for a in areas] == [1, 2]
    assert any(not np.array_equal(after[k], exp[k]) for k in ("metric", "links", "count"))
    assert all(a["ls"].counters()["engine_errors"] == 0 for a in areas)


def test_linkstate_call_degrades_after_an_injected_error():
    spec, areas, table = ls_areas()
    ls_check(areas, table, True)
    areas[1]["ls"].inject_engine_error(1)
    ls_check(areas, table, False)
    assert areas[1]["ls"].counters()["engine_errors"] == 1
    assert all(a["ls"].counters()["engine_degraded"] == 1 for a in areas)
    ls_check(areas, table, False)  # and stays on the host path
