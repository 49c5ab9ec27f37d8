"""Oracle-derived expectation for the delta of the policy selection (shared by
the tests of ospf_selstate_*_policy).

A graph version is a seldelta_ref.Version; its expectation is
selpolicy_ref.expect (createRouteForPrefix's four steps over the CPU oracle's
SPF results) under one set of prefix attributes. The expected delta between
two (version, attributes) pairs is the numpy diff of their expectations over
all six columns (metric, count, links, need, best and the next-hop words); the
rebased roots are those whose select_ref.root_neighbor_ids differ. Nothing
here reads the code under test beyond LinkState's ingest."""
import numpy as np

import selpolicy_ref as PR
from openr_amd.adjdb import AdjDb, create_adjacency

COLS = ("metric", "count", "links", "need", "best")


def expect(version, table, pref, mnh, W, hop=False, roots=None):
    """(selpolicy_ref.expect's dict by node id, facts)"""
    spf = version.spf(not hop, roots)
    return PR.expect(spf, version.names, version.csr, table, pref, mnh, W, hop, roots)


def diff(eb, ea, rebased=()):
    """{(root, prefix)} where any column or word differs; rebased roots left out"""
    mask = (eb["nh"] != ea["nh"]).any(axis=2)
    for k in COLS:
        mask |= eb[k] != ea[k]
    mask[list(rebased)] = False
    return {(int(r), int(p)) for r, p in np.argwhere(mask)}


def delta(before, after, table, pol_before, pol_after, W, hop=False):
    """before / after: Versions; pol_*: (pref, mnh). -> (changed, rebased,
    expectation after, expectation before)"""
    assert before.names == after.names
    eb, _ = expect(before, table, *pol_before, W, hop)
    ea, _ = expect(after, table, *pol_after, W, hop)
    rebased = [r for r in range(before.V) if before.nbrs(r) != after.nbrs(r)]
    return diff(eb, ea, rebased), rebased, ea, eb


def only_column(eb, ea, key):
    """the cells where `key` is the only column that differs"""
    other = (eb["nh"] != ea["nh"]).any(axis=2)
    for k in COLS:
        if k != key:
            other |= eb[k] != ea[k]
    return (eb[key] != ea[key]) & ~other


def records(rec, nh):
    """update_policy()'s arrays -> {(root, prefix): (metric, count, links,
    need, best, installed, words tuple)}; asserts that no entry is listed twice"""
    out = {}
    for i in range(len(rec)):
        key = (int(rec["root"][i]), int(rec["prefix"][i]))
        assert key not in out, ("listed twice", key)
        out[key] = tuple(int(rec[k][i]) for k in COLS + ("installed",)) + \
            (tuple(int(x) for x in nh[i]),)
    return out


def wanted(changed, ea):
    return {(r, p): tuple(int(ea[k][r, p]) for k in COLS + ("installed",)) +
            (tuple(int(x) for x in ea["nh"][r, p]),) for r, p in changed}


def assert_state(st, ea, W, roots=None, what=""):
    """copy_policy of every root (or `roots`) == the expectation"""
    roots = list(range(ea["metric"].shape[0])) if roots is None else list(roots)
    got = st.copy_policy(roots, W)
    for k in PR.KEYS:
        bad = np.argwhere(got[k] != ea[k][roots])
        assert bad.size == 0, (what, k, bad[:5].tolist())


def column_dbs(down=()):
    """a (drained) - x = r (two equal links), x - t; `down`: (node, other,
    which) adjacencies reported down"""
    names = ["a", "r", "t", "x"]
    adjs = {nm: [] for nm in names}

    def link(p, q, tag=""):
        adjs[p].append(create_adjacency(q, f"{p}-{q}{tag}", f"{q}-{p}{tag}", 1))
        adjs[q].append(create_adjacency(p, f"{q}-{p}{tag}", f"{p}-{q}{tag}", 1))

    link("r", "x"), link("r", "x", "-2"), link("x", "t"), link("a", "x")
    for node, ifname in down:
        for adj in adjs[node]:
            if adj.if_name == ifname:
                adj.overloaded = True
    return [AdjDb(nm, adjs[nm], i + 1, overloaded=nm == "a") for i, nm in enumerate(names)]


def prefixes_by_name(names, table, pol):
    """the table in LinkState.track_select_policy's form: class rank c as
    path preference 1000 - c (the larger wins), threshold 0 as unset"""
    pref, mnh = pol
    return {f"p{p}": [(names[a], 1000 - c, 200, 1, m or None)
                      for a, c, m in zip(ann, pref[p], mnh[p])] for p, ann in enumerate(table)}


def assert_linkstate_delta(ls, before, after, table, pol_before, pol_after, hop=False):
    """policy_delta of `ls` == the numpy diff; the rebased roots and the
    whole baseline are read back with policy_tracked. -> changed"""
    d = ls.policy_delta()
    assert not d["full"]
    W = d["nh"].shape[1]
    assert W == after.words
    changed, rebased, ea, _ = delta(before, after, table, pol_before, pol_after,
                                    max(W, before.words), hop)
    ea = dict(ea, nh=ea["nh"][:, :, :W])
    assert sorted(d["rebased"].tolist()) == rebased
    assert records(d["changes"], d["nh"]) == wanted(changed, ea)
    got = ls.policy_tracked(after.names)
    for k in PR.KEYS + ("installed",):
        assert np.array_equal(got[k], ea[k]), k
    return changed
