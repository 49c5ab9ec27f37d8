"""Oracle-derived expectation for the delta of the multi-area selection (shared
by the tests of ospf_areastate_*).

A version is a list of areas (area-name order), each a dict {names, csr, spf}
as areas_ref takes it, built here from an AdjDb list by LinkState's ingest and
the CPU oracle. Its expectation is areas_ref.expect under one table (the
entries and their attributes). The expected delta between two (version, table)
pairs is the numpy diff of their expectations over the six columns and every
area's words; the rebased roots are the global ids of the nodes whose
root_neighbor_ids differ in any area. Nothing here reads the code under test
beyond LinkState's ingest."""
import numpy as np

import areas_ref as AR
from graphs import metric_graph
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState, root_neighbor_ids
from oracle import Oracle, parse_spf_text

INF = 0xFFFFFFFF
COLS = AR.KEYS


def area(dbs, hop=False):
    """{names, csr, spf, dbs} of one area's AdjDb list"""
    st = AdjDbStream.from_dbs(dbs)
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    orc = Oracle(st)
    spf = {r: parse_spf_text(orc.spf_text(r, not hop)) for r in names}
    return dict(names=names, csr=csr, spf=spf, dbs=dbs)


def area_links(links, overloaded=(), hop=False):
    """area() of an explicit graph (graphs.metric_graph)"""
    return area(metric_graph(links, overloaded), hop)


def words(areas):
    """per area the widest root's next-hop words"""
    return tuple(max(1, max((root_neighbor_ids(a["csr"], r).size + 31) // 32
                            for r in range(len(a["names"])))) for a in areas)


def by_global(areas, exp):
    """the expectation's words by global id: [G, P, sum of the areas' words],
    area a's words one after the other, zero where a does not hold the node"""
    _, gids = AR.union(areas)
    G, P = exp["metric"].shape
    out = np.zeros((G, P, sum(x.shape[2] for x in exp["nh"])), np.uint32)
    o = 0
    for a, x in enumerate(exp["nh"]):
        out[gids[a], :, o:o + x.shape[2]] = x
        o += x.shape[2]
    return out


def rebased_roots(before, after):
    gnames, gids = AR.union(before)
    out = set()
    for a, (b, c) in enumerate(zip(before, after)):
        assert b["names"] == c["names"]
        for i in range(len(b["names"])):
            if root_neighbor_ids(b["csr"], i).tolist() != root_neighbor_ids(c["csr"], i).tolist():
                out.add(int(gids[a][i]))
    return sorted(out)


def diff(areas, eb, ea, rebased=()):
    """{(global root, prefix)} where any column or any area's word differs;
    rebased roots left out"""
    mask = (by_global(areas, eb) != by_global(areas, ea)).any(axis=2)
    for k in COLS:
        mask |= eb[k] != ea[k]
    mask[list(rebased)] = False
    return {(int(r), int(p)) for r, p in np.argwhere(mask)}


def delta(before, after, table_before, table_after, W, hop=False):
    """before / after: lists of areas; table_*: areas_ref tables with the same
    entries (the attributes may differ). -> (changed, rebased, expectation
    after, expectation before)"""
    eb, _ = AR.expect(before, table_before, W, hop)
    ea, _ = AR.expect(after, table_after, W, hop)
    rebased = rebased_roots(before, after)
    return diff(before, eb, ea, rebased), rebased, ea, eb


def records(rec, nh):
    """AreaSelState.update()'s arrays -> {(root, prefix): (metric, count, links,
    need, best, areas, installed, words tuple)}; asserts that no cell is listed
    twice"""
    out = {}
    for i in range(len(rec)):
        key = (int(rec["root"][i]), int(rec["prefix"][i]))
        assert key not in out, ("listed twice", key)
        out[key] = tuple(int(rec[k][i]) for k in COLS + ("installed",)) + \
            (tuple(int(x) for x in nh[i]),)
    return out


def wanted(areas, changed, ea):
    nh = by_global(areas, ea)
    return {(r, p): tuple(int(ea[k][r, p]) for k in COLS + ("installed",)) +
            (tuple(int(x) for x in nh[r, p]),) for r, p in changed}


def assert_state(st, areas, ea, W, roots=None, what=""):
    """copy of every global root (or `roots`) == the expectation"""
    roots = list(range(ea["metric"].shape[0])) if roots is None else list(roots)
    got = st.copy(roots, W)
    for k in COLS:
        bad = np.argwhere(got[k] != ea[k][roots])
        assert bad.size == 0, (what, k, bad[:5].tolist())
    nh = by_global(areas, ea)[roots]
    bad = np.argwhere(np.concatenate(got["nh"], axis=2) != nh)
    assert bad.size == 0, (what, "nh", bad[:5].tolist())


def only_one_areas_words(areas, eb, ea):
    """the cells whose only difference is the words of exactly one area"""
    hdr = np.zeros(eb["metric"].shape, bool)
    for k in COLS:
        hdr |= eb[k] != ea[k]
    _, gids = AR.union(areas)
    n = np.zeros(eb["metric"].shape, np.uint32)
    for a, (x, y) in enumerate(zip(eb["nh"], ea["nh"])):
        n[gids[a]] += (x != y).any(axis=2)
    return ~hdr & (n == 1)


# ---------------------------------------------------------------- events
def links_down(links, picks):
    """the picked links (positions) reported down: the neighbour lists stay"""
    out = list(links)
    for k in picks:
        out[k] = tuple(out[k][:4]) + ("down",)
    return out


def metric_bump(links, k, by=7):
    out = list(links)
    a, b, wab, wba = out[k][:4]
    out[k] = (a, b, wab + by, wba + by) + tuple(out[k][4:])
    return out


def toggled(overloaded, name):
    return set(overloaded) ^ {name}


def random_versions(seed, sizes, n_border, unit, hop=False):
    """four versions of AR.random_area_links as lists of areas: base; two links
    down in area 0 only; a metric bump in the last area and a border node's
    overload bit flipped in one area only; base again. Unchanged areas are the
    same dict objects, so a caller sees which areas an event touched."""
    spec = AR.random_area_links(seed, sizes, n_border, unit)
    base = [area_links(links, over, hop) for links, over in spec]
    l0, o0 = spec[0]
    # one of the two is the island's only link (the last of the list): its two
    # nodes lose each other
    v2 = [area_links(links_down(l0, (1, len(l0) - 1)), o0, hop)] + base[1:]
    ll, ol = spec[-1]
    # the bump on a link of a border node, so that other areas' roots see it
    k = next(i for i, ln in enumerate(ll) if ln[0] == "b02" or ln[1] == "b02")
    last = area_links(metric_bump(ll, k), toggled(ol, "b01"), hop)
    v3 = v2[:-1] + [last]
    return [base, v2, v3, base]


def random_table(areas, seed=5):
    """AR.random_entries with P > 64 (two chunks; entry counts 0, 1, 8, 9, 64,
    65 and 130 among them) and one prefix only an island node of area 0
    announces"""
    gnames, _ = AR.union(areas)
    table = AR.random_entries(areas, np.random.default_rng(seed), singles=60)
    return table + [[(gnames.index("mz1"), 0, 0, 0)]]


RANDOM_CASES = [(True, False, (60, 70), 5), (False, False, (60, 70), 5),
                (False, True, (45, 50, 40), 5), (False, False, (45, 50, 40), 5)]


def four_nodes(b_metric=10):
    """MultiAreaBestPathCalculation's graphs (DecisionTest.cpp): area "A" is
    1 - 2 - 4, area "B" 1 - 3 - 4; in name order B is area 0"""
    b = area_links([("1", "3", b_metric, b_metric), ("3", "4", b_metric, b_metric)])
    a = area_links([("1", "2", 10, 10), ("2", "4", 10, 10)])
    return [b, a]


def hub_links(dear=None):
    """area 0: a hub with 150 spokes (5 next-hop words), the spokes in pairs;
    area 1: the hub behind a handful of the spokes. `dear`: a spoke whose hub
    link costs 9 instead"""
    sp = [f"s{i:03d}" for i in range(150)]
    l0 = [("hub", s, 9 if s == dear else 1 + i % 3, 1 + i % 2) for i, s in enumerate(sp)]
    l0 += [(sp[i], sp[i + 1], 2, 2) for i in range(0, 60, 2)]
    l1 = [("hub", sp[i], 1 + i % 2, 2) for i in (5, 7, 9, 11)]
    l1 += [(sp[5], sp[7], 1, 1), (sp[9], "t0", 1, 1), ("t0", sp[11], 2, 1), ("t0", "t1", 1, 1)]
    l1 += [("t0" if i % 2 else "t1", sp[i], 1 + i % 4, 1 + i % 3) for i in range(20, 50)]
    return [(l0, ("s003",)), (l1, ("s007",))]


def random_table_hub(areas, seed=9):
    """P > 64 over the hub areas: long and short prefixes and the spokes one by one"""
    return AR.random_entries(areas, np.random.default_rng(seed), sizes=(0, 1, 2, 8, 9, 64, 65, 130),
                             singles=60)


def rebase_versions():
    """(before, after): area 0 is seldelta_ref.star_dbs(32, extra=1), where a
    link hub - x0 comes up (the hub goes from 32 to 33 neighbours, from one
    next-hop word to two); area 1 a small ring over the hub, x0 and two spokes"""
    import seldelta_ref as SR
    dbs = SR.star_dbs(32, extra=1)
    ring = [("hub", "s0003", 2, 2), ("s0003", "x0", 1, 1), ("x0", "s0009", 3, 1),
            ("s0009", "hub", 1, 2), ("x0", "y0", 1, 1)]
    a1 = area_links(ring)
    return [area(dbs), a1], [area(SR.link_up(dbs, "hub", "x0")), a1]


def rebase_table(areas, seed=3):
    return AR.random_entries(areas, np.random.default_rng(seed), sizes=(0, 1, 2, 3, 9, 20),
                             singles=12)


def other_attrs(table, seed=21):
    """the same entries with other class ranks and thresholds on a part of them"""
    rng = np.random.default_rng(seed)
    return [[(n, a, int(rng.integers(3)), int(rng.integers(5))) if rng.random() < 0.3
             else (n, a, r, m) for n, a, r, m in ents] for ents in table]


def swap_versions():
    """(before, after, table): in area 0 the root r reaches t over a at 3 and
    over b at 4, then over b at 3 and over a at 4; area 1 holds r and t at 20.
    The cell (r, t's prefix) keeps its six columns: only area 0's words move."""
    def a0(at, bt):
        return area_links([("r", "a", 1, 1), ("a", "t", at, at), ("r", "b", 1, 1), ("b", "t", bt, bt)])
    a1 = area_links([("r", "q", 10, 10), ("q", "t", 10, 10)])
    gnames, _ = AR.union([a0(2, 3), a1])
    t, q = gnames.index("t"), gnames.index("q")
    return [a0(2, 3), a1], [a0(3, 2), a1], [[(t, 0, 0, 0), (t, 1, 0, 0)], [(q, 1, 0, 0)]]


DEAR = "s020"  # the spoke of both hub areas whose hub link gets dearer


# ---------------------------------------------------------------- the LinkState tracker
def ls_areas(areas, host):
    """one LinkState per area ("a0", "a1", ...: the name order is the list's)
    loaded with the area's AdjDbs; host: on the host path, else on the device
    and allowed to degrade"""
    out = []
    for i, ar in enumerate(areas):
        ls = LinkState(area=f"a{i}")
        if host:
            ls.set_host_spf(True)
        else:
            ls.set_degrade(True)
        ls.apply(AdjDbStream.from_dbs(ar["dbs"]))
        out.append(ls)
    return out


def ls_load(lss, before, after):
    """apply the areas of `after` that are not `before`'s"""
    for ls, b, a in zip(lss, before, after):
        if a is not b:
            ls.apply(AdjDbStream.from_dbs(a["dbs"]))


def ls_prefixes(areas, table):
    """the table as linkstate.AreasTracker takes it: class rank r as path
    preference 1000 - r (the higher wins), threshold 0 as unset"""
    gnames, _ = AR.union(areas)
    return {f"p{p}": [(gnames[n], f"a{a}", 1000 - r, 0, 0, mn or None) for n, a, r, mn in ents]
            for p, ents in enumerate(table)}


def assert_tracked(tr, areas, table, hop=False):
    """tracked of every global name == the expectation"""
    gnames, _ = AR.union(areas)
    got = tr.tracked(gnames)
    W = tuple(int(w) for w in got["words"])
    assert W == words(areas)
    e, _ = AR.expect(areas, table, W, hop)
    for k in COLS + ("installed",):
        assert np.array_equal(got[k], e[k]), k
    assert np.array_equal(np.concatenate(got["nh"], axis=2), by_global(areas, e))


def assert_tracker_delta(tr, before, after, tb, ta, on_device, hop=False):
    """tr.delta() == the numpy diff; then tracked of all names. -> changed"""
    d = tr.delta()
    assert not d["full"] and d["on_device"] == on_device
    W = tuple(int(w) for w in d["words"])
    assert W == words(after)
    Wm = tuple(max(x, y) for x, y in zip(W, words(before)))
    changed, rebased, ea, _ = delta(before, after, tb, ta, Wm, hop)
    ea = dict(ea, nh=[x[:, :, :w] for x, w in zip(ea["nh"], W)])
    assert 0 < len(changed) < ea["metric"].size
    assert sorted(d["rebased"].tolist()) == rebased
    assert records(d["changes"], d["nh"]) == wanted(after, changed, ea)
    assert_tracked(tr, after, ta, hop)
    return changed


def grown_versions():
    """rebase_versions' first version, and the same with a node more in area 1"""
    v0, _ = rebase_versions()
    ring = [("hub", "s0003", 2, 2), ("s0003", "x0", 1, 1), ("x0", "s0009", 3, 1),
            ("s0009", "hub", 1, 2), ("x0", "y0", 1, 1), ("y0", "y1", 2, 2)]
    return v0, [v0[0], area_links(ring)]


def renamed(old, new, table):
    """`table` (global ids of `old`'s union) over `new`'s union; the entries
    stay ascending because both orders are name order"""
    go, gn = AR.union(old)[0], AR.union(new)[0]
    return [[(gn.index(go[n]), a, r, m) for n, a, r, m in ents] for ents in table]
