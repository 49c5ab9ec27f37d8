"""UCMP weights of every root and prefix as a recursion over the anycast
selection (shared by test_host_ucmp_all.py and test_gpu_ucmp_all.py).

SpfSolver::getNodeUcmpResult -> LinkState::resolveUcmpWeights
(openr/decision/SpfSolver.cpp:1091-1161, LinkState.cpp:913-1033) walks one
root's SPF DAG from the min-cost announcers to the root. Restated here without
a walk per root (DESIGN.md §3 o'''): the weight a node advertises in ANY
root's walk is the weight of its own selection,

    W(u) = leaf weight                              u announces (metric 0)
    W(u) = sum over u's selected next hops k of
             c(u, k) * W(k)                         prefix-weight propagation
             S(u, k)                                adjacency-weight propagation

with c(u, k) the tight links u-k (up, at the smallest metric u advertises on
an up link to k; every up link under hop count) and S(u, k) the sum of
weightFrom(u) over them. A root's per-link weights are W(k) on each tight
link to a selected next hop k, divided by their gcd when it is > 1.
An entry is OK only when its own weight and its next hops' weights are all
representable: a VOID or OVERFLOW next hop marks it in both algorithms (under
'adj' the sum itself does not need W(k); the per-link view does).

Inputs are select_ref's expectation (metric, count, next-hop words by node
id) and the CSR snapshot; nothing here reads the code under test beyond
LinkState's ingest (node ids, CSR, link keys), as select_ref does."""
from math import gcd

import numpy as np

import select_ref as R

OK, NONE, VOID, OVERFLOW = 0, 1, 2, 3
I63 = (1 << 63) - 1
ALGOS = ("adj", "prefix")


class Consts:
    """Per (node, distinct neighbour) slot, laid out like the engine's
    dn_off / dn: c = tight links, S = sum of the node's link weights on them."""

    def __init__(self, csr, names, dbs, link_keys, use_link_metric=True):
        V = len(names)
        wt = {(d.name, a.if_name): int(a.weight) for d in dbs for a in d.adjs}
        from_node = []  # link id -> {node name: weightFrom(node)}
        for key in link_keys:
            ends = {}
            if key:
                for end in key.split("|"):
                    node, iface = end.split("%")
                    ends[node] = wt[(node, iface)]
            from_node.append(ends)
        self.dn_off = np.zeros(V + 1, np.uint32)
        dn, c, S = [], [], []
        for u in range(V):
            nb = R.root_neighbor_ids(csr, u).tolist()
            lo, hi = int(csr["row_ptr"][u]), int(csr["row_ptr"][u + 1])
            up = {}  # neighbour -> its up entries (one pass: a hub of 2,100 spokes)
            for e in range(lo, hi):
                if csr["edge_up"][e]:
                    up.setdefault(int(csr["col"][e]), []).append(e)
            for k in nb:
                es = up.get(k, [])
                if use_link_metric and es:
                    m = min(int(csr["metric"][e]) for e in es)
                    es = [e for e in es if int(csr["metric"][e]) == m]
                c.append(len(es))
                S.append(sum(from_node[int(csr["link_id"][e])][names[u]] for e in es))
            dn += nb
            self.dn_off[u + 1] = len(dn)
        self.dn = np.array(dn, np.uint32)
        self.c = np.array(c, np.int64)
        # a sum beyond i63 (link weights the engine does not take) stays a Python integer
        self.S = np.array(S, np.int64 if max(S, default=0) <= I63 else object)

    def slots(self, u):
        return range(int(self.dn_off[u]), int(self.dn_off[u + 1]))

    def slot(self, u, k):
        """the slot of node u's distinct neighbour k"""
        lo = int(self.dn_off[u])
        return lo + self.dn[lo:int(self.dn_off[u + 1])].tolist().index(k)

    def with_S(self, sums):
        """a copy with S overridden: sums = {(node, neighbour): link weight sum}
        (the 'adj' limits are reached through S, whatever the links carry)"""
        import copy
        out = copy.copy(self)
        out.S = self.S.copy()
        for (u, k), s in sums.items():
            out.S[self.slot(u, k)] = s
        return out


def bits(words):
    """set bit positions of a next-hop mask, ascending"""
    return [32 * w + b for w, x in enumerate(words) for b in range(32) if (int(x) >> b) & 1]


def resolve(sel, consts, table, leaf_w, algo):
    """-> (W [V, P] i64 advertised weight (0 unless OK), status [V, P] u8,
    rounds = hop depth of the deepest selected path). leaf_w is parallel to
    table: leaf_w[p][i] the weight of announcer table[p][i]."""
    metric, count, nh = sel
    V, P = metric.shape
    W = [[0] * P for _ in range(V)]
    st = np.full((V, P), NONE, np.uint8)
    depth = np.zeros((V, P), np.int64)
    for p in range(P):
        lw = dict(zip(table[p], leaf_w[p]))
        for u in sorted(range(V), key=lambda v: int(metric[v, p])):
            if metric[u, p] == R.INF:
                continue
            if metric[u, p] == 0:  # u announces: its own entry, no next hop
                st[u, p] = OK if lw[u] > 0 else VOID
                W[u][p] = lw[u] if lw[u] > 0 else 0
                continue
            lo = int(consts.dn_off[u])
            hops = [(lo + b, int(consts.dn[lo + b])) for b in bits(nh[u, p])]
            assert hops and all(metric[k, p] < metric[u, p] for _, k in hops)
            depth[u, p] = 1 + max(int(depth[k, p]) for _, k in hops)
            kinds = {int(st[k, p]) for _, k in hops}
            assert NONE not in kinds
            total = 0
            for s, k in hops:
                total += int(consts.S[s]) if algo == "adj" else int(consts.c[s]) * W[k][p]
            if VOID in kinds:
                st[u, p] = VOID
            elif OVERFLOW in kinds or total > I63:
                st[u, p] = OVERFLOW
            else:
                st[u, p], W[u][p] = OK, total
    out = np.array([[w if w <= I63 else 0 for w in row] for row in W], np.int64).reshape(V, P)
    return out, st, int(depth.max()) if depth.size else 0


def links(sel, consts, res, r, p):
    """Root r's per-link view of prefix p: [(next hop id, tight links to it,
    normalised weight)] in next-hop bit order; [] unless the entry is OK."""
    W, st, _ = res
    if st[r, p] != OK:
        return []
    lo = int(consts.dn_off[r])
    hops = [(int(consts.dn[lo + b]), int(consts.c[lo + b])) for b in bits(sel[2][r, p])]
    g = 0
    for k, _ in hops:
        g = gcd(g, int(W[k, p]))
    return [(k, c, int(W[k, p]) // g if g > 1 else int(W[k, p])) for k, c in hops]


def copy_expect(sel, consts, res, roots):
    """ospf_selstate_ucmp_copy's outputs for `roots`: advertised [n, P],
    status [n, P], off [n * P + 1], wt [...] (one per set next-hop bit)."""
    W, st, _ = res
    P = W.shape[1]
    off, wt = [0], []
    for r in roots:
        for p in range(P):
            wt += [w for _, _, w in links(sel, consts, res, r, p)]
            off.append(len(wt))
    return W[list(roots)], st[list(roots)], np.array(off, np.uint64), np.array(wt, np.int64)


def min_cost(spf_of_root, names, ann):
    """announcer ids at the root's smallest metric (getNextHopsWithMetric)"""
    reach = [(spf_of_root[names[a]][0], a) for a in ann if names[a] in spf_of_root]
    if not reach:
        return []
    best = min(m for m, _ in reach)
    return [a for m, a in reach if m == best]
