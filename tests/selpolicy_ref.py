"""Oracle-derived expectation for route selection under the reference's
best-route policy (shared by test_host_select_policy.py and
test_gpu_select_policy.py).

The rule is restated as the four steps createRouteForPrefix takes
(openr/decision/SpfSolver.cpp:197-458), per root, over the CPU oracle's SPF
results -- never the packed key the engine uses, never the engine's rows:

  1. drop the announcers the root does not reach                (:229-244)
  2. keep the best class among the reached ones                 (:649-676)
  3. drop the drained ones unless all of the class are drained  (:709-731)
  4. take the minimum distance; withhold the route when it has fewer next-hop
     links than the largest minNexthop of step 3's set          (:990-1000)

A class is a rank per announcer entry (smaller wins); the drained bit is the
graph's no_transit column; the links r - k of a next hop k are counted from
the CSR columns (up entries at the smallest metric r advertises towards k;
every up entry under hop count)."""
import numpy as np

from openr_amd.linkstate import root_neighbor_ids

INF = 0xFFFFFFFF
KEYS = ("metric", "count", "nh", "links", "need", "best")


def link_counts(csr, r, hop):
    """{neighbour id: links r - k getNextHopsThrift emits for next hop k}"""
    lo, hi = int(csr["row_ptr"][r]), int(csr["row_ptr"][r + 1])
    per = {}
    for e in range(lo, hi):
        k = int(csr["col"][e])
        if k == r or not csr["edge_up"][e]:
            continue
        per.setdefault(k, []).append(int(csr["metric"][e]))
    return {k: (len(ms) if hop else ms.count(min(ms))) for k, ms in per.items()}


def expect(spf, names, csr, table, pref, mnh, W, hop=False, roots=None):
    """table / pref / mnh: per prefix the announcer ids (ascending), their
    class ranks and thresholds (0 = unset). -> (dict of metric / count / links
    / need / best [V, P], nh [V, P, W], installed [V, P] by node id, facts):
    facts counts the (root, prefix) cells that exercise each corner. With
    `roots` (node ids) only those rows are filled (spf needs only them)."""
    V, P = len(names), len(table)
    ids = {nm: i for i, nm in enumerate(names)}
    drained = np.asarray(csr["no_transit"]).astype(bool)
    out = {k: np.zeros((V, P), np.uint32) for k in KEYS if k != "nh"}
    out["metric"][:] = INF
    out["best"][:] = INF
    out["nh"] = np.zeros((V, P, W), np.uint32)
    facts = dict(fallback=0, filtered=0, all_drained=0, drained_root_skipped=0,
                 need_outside_L=0, withheld=0, best_outside=0, routes=0)
    for r in (range(V) if roots is None else roots):
        res = spf[names[r]]
        bit = {v: k for k, v in enumerate(root_neighbor_ids(csr, r).tolist())}
        c = link_counts(csr, r, hop)
        for p, ann in enumerate(table):
            # 1. the reached announcers
            R = [i for i, a in enumerate(ann) if names[a] in res]
            if not R:
                continue
            # 2. the best class
            top = min(pref[p][i] for i in R)
            S = [i for i in R if pref[p][i] == top]
            # 3. the drain filter
            Sf = [i for i in S if not drained[ann[i]]] or S
            # 4. the minimum
            m = min(res[names[ann[i]]][0] for i in Sf)
            L = [i for i in Sf if res[names[ann[i]]][0] == m]
            hops = set()
            for i in L:
                hops |= set(res[names[ann[i]]][1])
            links = 0
            for h in hops:
                k = bit[ids[h]]
                out["nh"][r, p, k // 32] |= np.uint32(1 << (k % 32))
                links += c[ids[h]]
            need = max(mnh[p][i] for i in Sf)
            s_ids = [ann[i] for i in S]
            best = r if r in s_ids else min(s_ids)
            out["metric"][r, p] = m
            out["count"][r, p] = len(L)
            out["links"][r, p] = links
            out["need"][r, p] = need
            out["best"][r, p] = best
            facts["routes"] += links > 0
            facts["fallback"] += top > min(pref[p])
            facts["filtered"] += len(Sf) != len(S)
            facts["all_drained"] += all(drained[ann[i]] for i in S)
            facts["drained_root_skipped"] += r in s_ids and r not in [ann[i] for i in Sf]
            facts["need_outside_L"] += need > max(mnh[p][i] for i in L)
            facts["withheld"] += need > links > 0
            facts["best_outside"] += best not in [ann[i] for i in Sf]
    out["installed"] = (out["links"] > 0) & (out["need"] <= out["links"])
    return out, facts


def random_policy(table, rng, classes=3, max_need=4):
    """per entry a class rank in 0 .. classes - 1 and a threshold in 0 .. max_need"""
    pref = [rng.integers(0, classes, size=len(a)).tolist() for a in table]
    mnh = [rng.integers(0, max_need + 1, size=len(a)).tolist() for a in table]
    return pref, mnh


def uniform_policy(table):
    return [[0] * len(a) for a in table], [[0] * len(a) for a in table]


def flat(cols):
    return np.array([x for a in cols for x in a], np.uint32)


def decode(nh_words, nbrs):
    """set of neighbour ids of a mask's set bits"""
    return {int(nbrs[k]) for k in range(len(nbrs)) if int(nh_words[k // 32]) >> (k % 32) & 1}


def assert_equal(got, want, keys=KEYS, ctx=""):
    for k in keys:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (ctx, k, bad[:5].tolist(),
                               [(int(got[k][tuple(b)]), int(want[k][tuple(b)])) for b in bad[:5]])
