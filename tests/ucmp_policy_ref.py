"""UCMP weights over the POLICY selection as a recursion (shared by
test_host_ucmp_policy.py and test_gpu_ucmp_policy.py): ucmp_ref's recursion
 plus the one rule the policy adds.

Under the policy an announcer need not select itself: an overloaded node k
reaches, as a root, nodes behind itself that its neighbours do not, so its own
entry may select a better class behind it, or -- drained beside an undrained
class-mate -- another announcer. For a root u whose next hop k is overloaded,
k is still a LEAF of u's walk (nothing transits k). Hence the rule: a selected
next hop whose no-transit bit is set contributes its leaf weight for the
prefix (VOID when that is 0) and is never waited for.

The recursion runs in rounds as the device does: round 0 settles the entries
without a reached announcer (NONE) and those that select themselves (metric
0); round t settles an entry when every next hop was settled in a round < t.
`leaf_rule=False` gives the recursion WITHOUT the rule (the non-vacuity check
of the tests). Inputs are selpolicy_ref's expectation and ucmp_ref.Consts."""
from math import gcd

import numpy as np

import ucmp_ref as U

INF = 0xFFFFFFFF


def policy_leaves(spf_of_root, names, ann, pref, drained):
    """L of one root and prefix: the four steps of selpolicy_ref.expect
    restated (reached, best class, drain filter, minimum) -> announcer ids"""
    R = [i for i, a in enumerate(ann) if names[a] in spf_of_root]
    if not R:
        return []
    top = min(pref[i] for i in R)
    S = [i for i in R if pref[i] == top]
    Sf = [i for i in S if not drained[ann[i]]] or S
    m = min(spf_of_root[names[ann[i]]][0] for i in Sf)
    return [ann[i] for i in Sf if spf_of_root[names[ann[i]]][0] == m]


def hop_weight(k, p, W, st, lw, drained, leaf_rule):
    """(status, weight) next hop k of prefix p contributes; None: not settled"""
    if leaf_rule and drained[k] and k in lw:
        return (U.OK, lw[k]) if lw[k] > 0 else (U.VOID, 0)
    if st[k][p] is None:
        return None
    return st[k][p], W[k][p]


def resolve(sel, consts, table, leaf_w, algo, drained, leaf_rule=True):
    """sel: selpolicy_ref.expect's dict. -> (W [V, P] i64, status [V, P] u8,
    rounds). An entry whose next hops never settle (possible only without the
    rule) raises."""
    metric, nh = sel["metric"], sel["nh"]
    V, P = metric.shape
    W = [[0] * P for _ in range(V)]
    st = [[None] * P for _ in range(V)]
    lws = [dict(zip(table[p], leaf_w[p])) for p in range(P)]
    pending = []
    for u in range(V):
        for p in range(P):
            if metric[u, p] == INF:
                st[u][p] = U.NONE
            elif metric[u, p] == 0:
                w = lws[p][u]
                st[u][p], W[u][p] = (U.OK, w) if w > 0 else (U.VOID, 0)
            else:
                pending.append((u, p))
    rounds = 0
    while pending:
        rounds += 1
        settled, left = [], []
        for u, p in pending:
            lo = int(consts.dn_off[u])
            hops = [(lo + b, int(consts.dn[lo + b])) for b in U.bits(nh[u, p])]
            assert hops
            got = [hop_weight(k, p, W, st, lws[p], drained, leaf_rule) for _, k in hops]
            if any(g is None for g in got):
                left.append((u, p))
                continue
            kinds = {g[0] for g in got}
            assert U.NONE not in kinds
            total = sum(int(consts.S[s]) if algo == "adj" else int(consts.c[s]) * g[1]
                        for (s, _), g in zip(hops, got))
            if U.VOID in kinds:
                settled.append((u, p, U.VOID, 0))
            elif U.OVERFLOW in kinds or total > U.I63:
                settled.append((u, p, U.OVERFLOW, 0))
            else:
                settled.append((u, p, U.OK, total))
        assert settled, "next hops that never settle"
        for u, p, s, w in settled:  # visible to the next round only
            st[u][p], W[u][p] = s, w
        pending = left
    return (np.array(W, np.int64).reshape(V, P), np.array(st, np.uint8).reshape(V, P), rounds)


def links(sel, consts, res, r, p, table, leaf_w, drained, leaf_rule=True):
    """root r's per-link view of prefix p: [(next hop id, tight links,
    normalised weight)] in bit order; [] unless the entry is OK"""
    W, st, _ = res
    if st[r, p] != U.OK:
        return []
    lw = dict(zip(table[p], leaf_w[p]))
    lo = int(consts.dn_off[r])
    hops = []
    for b in U.bits(sel["nh"][r, p]):
        k = int(consts.dn[lo + b])
        w = lw[k] if leaf_rule and drained[k] and k in lw else int(W[k, p])
        hops.append((k, int(consts.c[lo + b]), w))
    g = 0
    for _, _, w in hops:
        g = gcd(g, w)
    return [(k, c, w // g if g > 1 else w) for k, c, w in hops]


def copy_expect(sel, consts, res, roots, table, leaf_w, drained):
    """ospf_selstate_ucmp_copy's outputs for `roots`"""
    W, st, _ = res
    P = W.shape[1]
    off, wt = [0], []
    for r in roots:
        for p in range(P):
            wt += [w for _, _, w in links(sel, consts, res, r, p, table, leaf_w, drained)]
            off.append(len(wt))
    return W[list(roots)], st[list(roots)], np.array(off, np.uint64), np.array(wt, np.int64)
