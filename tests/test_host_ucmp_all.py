"""The argument behind the all-roots UCMP recursion (ucmp_ref, DESIGN.md §3
o'''), proved against the CPU oracle -- no device, no engine code.

For every root of every graph below, both propagation algorithms: the
oracle's resolveUcmpWeights(getSpfResult(root), min-cost announcers of that
root)[root] -- the advertised weight and the per-interface next-hop weights --
equals ucmp_ref's recursion over select_ref's expectation. The zero-weight
rule of SpfSolver::getNodeUcmpResult (:1139-1142, VOID) and the empty leaf set
(NONE) are restated here from the oracle's SPF results, not from the recursion.
Each case asserts that it exercises unequal next-hop weights, a gcd > 1, a
link multiplicity > 1, a VOID root and a NONE root."""
import numpy as np
import pytest

import select_ref as R
import ucmp_ref as U
from openr_amd.adjdb import AdjDb, AdjDbStream, create_adjacency
from openr_amd.linkstate import LinkState
from oracle import Oracle, parse_spf_text


def build_graph(seed, n=22, p=0.16, unit=False, parallel=0.3, equal=None, overload=(), mmax=3):
    """A seeded random graph with an island of two nodes (unreached from the
    rest). Metrics 1..mmax (ECMP is common); a pair gets 2-3 parallel links with
    probability `parallel`, their metrics equal / the last one dearer / random for
    equal = True / False / None. Link weights 1..5 per direction. `overload`:
    indices of the nodes reported overloaded."""
    rng = np.random.default_rng(seed)
    names = [f"n{i:02d}" for i in range(n)] + ["z0", "z1"]
    adjs = {nm: [] for nm in names}
    k = 0

    def link(a, b, ma, mb):
        nonlocal k
        ia, ib = f"{a}-{b}-{k}", f"{b}-{a}-{k}"
        k += 1
        adjs[a].append(create_adjacency(b, ia, ib, ma, weight=int(rng.integers(1, 6))))
        adjs[b].append(create_adjacency(a, ib, ia, mb, weight=int(rng.integers(1, 6))))

    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() > p and j != i + 1:  # the chain i - i+1 keeps it connected
                continue
            cnt = int(rng.integers(2, 4)) if rng.random() < parallel else 1
            ma, mb = (1, 1) if unit else (int(rng.integers(1, mmax + 1)), int(rng.integers(1, mmax + 1)))
            for t in range(cnt):
                if unit or equal is True or t == 0:
                    link(names[i], names[j], ma, mb)
                elif equal is False:  # the last of the group dearer: (m, m + 1) or (m, m, m + 1)
                    link(names[i], names[j], ma + (t == cnt - 1), mb + (t == cnt - 1))
                else:
                    link(names[i], names[j], int(rng.integers(1, mmax + 1)), int(rng.integers(1, mmax + 1)))
    link("z0", "z1", 1, 1)
    over = {names[i] for i in overload}
    return [AdjDb(nm, adjs[nm], i + 1, overloaded=nm in over) for i, nm in enumerate(names)]


class Case:
    """A graph, a weighted prefix table and everything derived from the
    oracle: per metric mode the SPF results, the selection and the constants."""

    def __init__(self, dbs, seed):
        self.dbs = dbs
        self.stream = AdjDbStream.from_dbs(dbs)
        ls = LinkState()
        ls.set_host_spf(True)
        ls.apply(self.stream)
        self.names, self.csr, self.keys = ls.node_names(), ls.csr(), ls.link_keys()
        self.V = len(self.names)
        self.orc = Oracle(self.stream)
        self.over = [i for i, nm in enumerate(self.names) if ls.is_overloaded(nm)]
        rng = np.random.default_rng(1000 + seed)
        V = self.V
        isl = [self.names.index("z0"), self.names.index("z1")]
        main = [v for v in range(V) if v not in isl]
        t = [[]] + [[v] for v in main[:6]]
        t += [sorted(rng.choice(main, size=s, replace=False).tolist()) for s in (2, 3, 4, 6)]
        t.append(sorted(self.over[:2] + main[:1]) if self.over else main[:3])  # overloaded announcers
        t.append(isl[:1])  # announced on the island only: NONE for the rest
        t.append(main[3:9])  # carries a zero-weight leaf
        self.table = t
        self.leaf_w = [[int(x) for x in rng.choice([2, 3, 4, 6, 9, 10], size=len(a))] for a in t]
        self.leaf_w[-1][2] = 0
        self.W = max(1, max((len(R.root_neighbor_ids(self.csr, r)) + 31) // 32 for r in range(V)))

    def mode(self, use_link_metric):
        spf = {nm: parse_spf_text(self.orc.spf_text(nm, use_link_metric)) for nm in self.names}
        sel = R.expect(spf, self.names, self.csr, self.table, self.W)
        consts = U.Consts(self.csr, self.names, self.dbs, self.keys, use_link_metric)
        return spf, sel, consts


def oracle_view(case, root, leaves, algo, use_link_metric):
    """the oracle's result of `root` -> (advertised, {next hop id: (ifaces, weight)})"""
    got = case.orc.ucmp(case.names[root], {case.names[a]: w for a, w in leaves.items()}, algo,
                        use_link_metric)
    w, hops = got[case.names[root]]
    by = {}
    for _, (nh, hw) in hops.items():
        k = case.names.index(nh)
        n, prev = by.get(k, (0, hw))
        assert prev == hw  # parallel tight links carry the same weight
        by[k] = (n + 1, hw)
    return w, by


def check(case, use_link_metric):
    spf, sel, consts = case.mode(use_link_metric)
    seen = dict(unequal=0, gcd=0, mult=0, void=0, none=0, ok=0, over_leaf=0, over_transit_root=0)
    for algo in U.ALGOS:
        res = U.resolve(sel, consts, case.table, case.leaf_w, algo)
        Wv, st, rounds = res
        assert rounds >= 2
        for r in range(case.V):
            for p, ann in enumerate(case.table):
                best = U.min_cost(spf[case.names[r]], case.names, ann)
                assert len(best) == sel[1][r, p]
                lw = dict(zip(ann, case.leaf_w[p]))
                if not best:
                    assert st[r, p] == U.NONE and Wv[r, p] == 0
                    seen["none"] += 1
                    continue
                if any(lw[a] == 0 for a in best):  # getNodeUcmpResult returns nullopt
                    assert st[r, p] == U.VOID, (r, p)
                    seen["void"] += 1
                    continue
                assert st[r, p] == U.OK, (r, p, int(st[r, p]))
                want_w, want_hops = oracle_view(case, r, {a: lw[a] for a in best}, algo,
                                                use_link_metric)
                mine = U.links(sel, consts, res, r, p)
                assert int(Wv[r, p]) == want_w, (algo, r, p)
                assert {k: (c, w) for k, c, w in mine} == want_hops, (algo, r, p)
                seen["ok"] += 1
                raw = [int(Wv[k, p]) for k, _, _ in mine]
                seen["unequal"] += len(set(raw)) > 1
                seen["gcd"] += bool(mine) and raw[0] != mine[0][2]
                seen["mult"] += any(c > 1 for _, c, _ in mine)
                seen["over_leaf"] += any(a in case.over for a in best) and r not in best
                seen["over_transit_root"] += r in case.over and bool(mine)
    for what in ("unequal", "gcd", "mult", "void", "none", "ok"):
        assert seen[what], (what, seen)
    return seen


CASES = {
    # name: (build_graph arguments, use_link_metric)
    "random-unit": (dict(seed=1, unit=True), True),
    "random-weighted": (dict(seed=2, mmax=6), True),
    "parallel-equal": (dict(seed=3, parallel=0.6, equal=True), True),
    "parallel-unequal": (dict(seed=4, parallel=0.6, equal=False), True),
    "overloaded-announcers": (dict(seed=5, overload=(2, 7, 11)), True),
    "overloaded-interior": (dict(seed=6, overload=(4, 9, 13, 16)), True),
    "link-metric": (dict(seed=7, mmax=4), True),
    "hop-count": (dict(seed=7, mmax=4), False),
    "hop-count-unequal-parallel": (dict(seed=4, parallel=0.6, equal=False), False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_recursion_equals_the_oracle_walk(name):
    kw, ulm = CASES[name]
    case = Case(build_graph(**kw), kw["seed"])
    seen = check(case, ulm)
    if name == "overloaded-announcers":
        assert seen["over_leaf"]  # an overloaded announcer is some other root's leaf
    if name == "overloaded-interior":
        # overloaded nodes that announce nothing in most prefixes: never a
        # transit, yet roots with next hops of their own
        assert seen["over_transit_root"]
    if name == "parallel-unequal":
        # the dearer parallel links are not tight under link metrics ...
        _, _, cm = case.mode(True)
        _, _, ch = case.mode(False)
        assert (ch.c > cm.c).any()  # ... and count under hop count


def test_overflow_status_is_the_recursions_own():
    """Leaf weights of 2^61 on a diamond with four tight links per hop: the
    sum leaves i63. The reference is undefined there (signed overflow), so
    only the status is pinned, and that it propagates upward."""
    adjs = {nm: [] for nm in "abcd"}

    def link(a, b, n):
        for t in range(n):
            adjs[a].append(create_adjacency(b, f"{a}-{b}-{t}", f"{b}-{a}-{t}", 1))
            adjs[b].append(create_adjacency(a, f"{b}-{a}-{t}", f"{a}-{b}-{t}", 1))

    link("a", "b", 1), link("b", "c", 4), link("c", "d", 1)
    dbs = [AdjDb(nm, adjs[nm], i + 1) for i, nm in enumerate("abcd")]
    case = Case.__new__(Case)
    case.dbs, case.stream = dbs, AdjDbStream.from_dbs(dbs)
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(case.stream)
    case.names, case.csr, case.keys = ls.node_names(), ls.csr(), ls.link_keys()
    case.V, case.W, case.orc = 4, 1, Oracle(case.stream)
    case.table, case.leaf_w = [[3]], [[1 << 61]]
    _, sel, consts = case.mode(True)
    Wv, st, rounds = U.resolve(sel, consts, case.table, case.leaf_w, "prefix")
    assert st[:, 0].tolist() == [U.OVERFLOW, U.OVERFLOW, U.OK, U.OK] and rounds == 3
    assert Wv[:, 0].tolist() == [0, 0, 1 << 61, 1 << 61]
    _, st, _ = U.resolve(sel, consts, case.table, case.leaf_w, "adj")
    assert (st[:, 0] == U.OK).all()


# ---------------------------------------------------------------- LinkState, host path
def tracked(case, use_link_metric, host=True):
    ls = LinkState()
    if host:
        ls.set_host_spf(True)
    ls.apply(case.stream)
    ls.track_select({f"p{i}": [case.names[a] for a in ann] for i, ann in enumerate(case.table)},
                    use_link_metric)
    return ls


def assert_linkstate(ls, case, use_link_metric, algo, overflow_free=True):
    """all_sources_ucmp / ucmp_tracked of `ls` == ucmp_ref (itself proved
    against the oracle above); -> the expectation"""
    _, sel, consts = case.mode(use_link_metric)
    res = U.resolve(sel, consts, case.table, case.leaf_w, algo)
    weight, status = ls.all_sources_ucmp(case.leaf_w, algo)
    assert np.array_equal(status, res[1]) and np.array_equal(weight, res[0])
    everyone = list(range(case.V))
    got = ls.ucmp_tracked(case.names)
    for g, w in zip(got, U.copy_expect(sel, consts, res, everyone)):
        assert np.array_equal(g, w)
    return res


@pytest.mark.parametrize("name", ["parallel-unequal", "overloaded-announcers", "hop-count"])
def test_linkstate_all_sources_ucmp_on_the_host_path(name):
    kw, ulm = CASES[name]
    case = Case(build_graph(**kw), kw["seed"])
    ls = tracked(case, ulm)
    for algo in U.ALGOS:
        assert_linkstate(ls, case, ulm, algo)
        assert ls.ucmp_info == dict(rounds=0, device=False, engine_ms=0.0)
    some = case.names[3:9]
    _, sel, consts = case.mode(ulm)
    res = U.resolve(sel, consts, case.table, case.leaf_w, "adj")
    for g, w in zip(ls.ucmp_host_loop(case.leaf_w, "adj", some),
                    U.copy_expect(sel, consts, res, range(3, 9))):
        assert np.array_equal(g, w)
    assert ls.counters()["engine_errors"] == 0


def test_linkstate_ucmp_contract_on_the_host_path():
    from openr_amd.linkstate import LinkStateError
    kw, ulm = CASES["random-weighted"]
    case = Case(build_graph(**kw), kw["seed"])
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(case.stream)
    with pytest.raises(LinkStateError):  # no tracked table
        ls.all_sources_ucmp([], "prefix")
    ls = tracked(case, ulm)
    with pytest.raises(LinkStateError):  # no result yet
        ls.ucmp_tracked(case.names[:2])
    short = [w[:-1] if w else w for w in case.leaf_w]
    with pytest.raises(LinkStateError):
        ls.all_sources_ucmp(short, "prefix")
    neg = [list(w) for w in case.leaf_w]
    neg[1][0] = -1
    with pytest.raises(LinkStateError):
        ls.all_sources_ucmp(neg, "prefix")
    ls.all_sources_ucmp(case.leaf_w, "prefix")
    # the topology moves: the tracked selection (and the result) is the old one's
    dbs = [d for d in case.dbs]
    import copy
    dbs = copy.deepcopy(case.dbs)
    dbs[0].adjs[0].metric += 3
    ls.apply(AdjDbStream.from_dbs(dbs))
    for call in (lambda: ls.all_sources_ucmp(case.leaf_w, "prefix"),
                 lambda: ls.ucmp_tracked(case.names[:2])):
        with pytest.raises(LinkStateError):
            call()
    ls.select_delta()
    with pytest.raises(LinkStateError):  # the weights were the old selection's
        ls.ucmp_tracked(case.names[:2])
    moved = Case(dbs, kw["seed"])
    assert_linkstate(ls, moved, ulm, "prefix")
