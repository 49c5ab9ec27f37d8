"""Random link-state graphs shared by the CPU and GPU parity tests."""
import numpy as np

from openr_amd.adjdb import AdjDb, AdjDbStream, create_adjacency


def random_stream(seed, n=40, p=0.15, parallel=0.2, overload=0.1, down=0.1, wmax=20,
                  unit=False):
    rng = np.random.default_rng(seed)
    names = [f"r{int(x)}" for x in rng.permutation(10 * n)[:n]]
    adjs = {nm: [] for nm in names}
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            if rng.random() > p:
                continue
            for _ in range(2 if rng.random() < parallel else 1):
                a, b = names[i], names[j]
                ia, ib = f"{a}-{b}-{k}", f"{b}-{a}-{k}"
                k += 1
                m1 = 1 if unit else int(rng.integers(1, wmax + 1))
                m2 = 1 if unit else int(rng.integers(1, wmax + 1))
                adjs[a].append(create_adjacency(b, ia, ib, m1, overloaded=bool(rng.random() < down)))
                adjs[b].append(create_adjacency(a, ib, ia, m2))
    dbs = [AdjDb(nm, adjs[nm], i + 1, overloaded=bool(rng.random() < overload))
           for i, nm in enumerate(names)]
    return AdjDbStream.from_dbs([dbs[i] for i in rng.permutation(n)]), names


def drained_fabric(pods, planes, seed=0, drain=0.05, down=0.03, weighted_seed=None,
                   ssw_per_plane=None):
    """topology.fabric with a random share of drained (overloaded) nodes and
    of adjacencies reported overloaded (links down), seeded."""
    from openr_amd import topology as T
    from openr_amd.adjdb import AdjDbStream
    rng = np.random.default_rng(seed)
    kw = {} if ssw_per_plane is None else {"ssw_per_plane": ssw_per_plane}
    dbs = T.fabric(pods=pods, planes=planes, weighted_seed=weighted_seed, **kw).to_dbs()
    for d in dbs:
        if rng.random() < drain:
            d.overloaded = True
        for a in d.adjs:
            if rng.random() < down:
                a.overloaded = True
    return AdjDbStream.from_dbs(dbs)


def deep_ladder(S, stage_width=2, *, ends=False, seed_stage=None, islands=(), hub=0,
                weighted_seed=None):
    """AdjDbs of a unit-metric ladder of S stages of `stage_width` nodes: every
    node of stage i is linked to every node of stages i - 1 and i + 1, none
    inside a stage, so the nodes of a stage are twins (same neighbours, 2
    apart, stage_width ECMP next hops towards anything beyond) at every depth.

    Names (ids are name ranks): stage i holds s{i:03d}a, s{i:03d}b, ...; with
    `seed_stage` its first node is named a{i:03d} instead and so is the
    lowest-id transit node, where the engine seeds its depth bound:
    2 * max(seed_stage, S - 1 - seed_stage) + 2.
    ends: overloaded (non-transit) e0 on all of stage 0 and e1 on all of
    stage S - 1 (S + 1 hops apart; outside the bound, still roots and
    destinations). hub=n: overloaded h linked to every node of stages
    0 .. n - 1 (stage_width * n distinct neighbours as a root; shortens
    nothing). islands=(k, ...): k-node cliques z{j}a, z{j}b, ... unreachable
    from the ladder and back. weighted_seed: random metrics 1..30 per
    adjacency on the same links (for hop-count runs)."""
    rng = None if weighted_seed is None else np.random.default_rng(weighted_seed)
    stage = [[f"s{i:03d}{chr(97 + j)}" for j in range(stage_width)] for i in range(S)]
    if seed_stage is not None:
        stage[seed_stage][0] = f"a{seed_stage:03d}"
    adjs, over = {nm: [] for st in stage for nm in st}, set()

    def link(a, b):
        for x, y in ((a, b), (b, a)):
            m = 1 if rng is None else int(rng.integers(1, 31))
            adjs[x].append(create_adjacency(y, f"{x}-{y}", f"{y}-{x}", m))

    for i in range(S - 1):
        for a in stage[i]:
            for b in stage[i + 1]:
                link(a, b)
    extra = ([("e0", stage[0]), ("e1", stage[S - 1])] if ends else []) + \
        ([("h", [nm for st in stage[:hub] for nm in st])] if hub else [])
    for nm, nbrs in extra:
        adjs[nm] = []
        over.add(nm)
        for b in nbrs:
            link(nm, b)
    for j, k in enumerate(islands):
        isl = [f"z{j}{chr(97 + t)}" for t in range(k)]
        adjs.update({nm: [] for nm in isl})
        for t in range(k):
            for u in range(t + 1, k):
                link(isl[t], isl[u])
    return [AdjDb(nm, adjs[nm], i + 1, overloaded=nm in over) for i, nm in enumerate(sorted(adjs))]


def depth_bound(csr):
    """The engine's BFS level bound (transit_depth_bound, spf_engine.hip)
    restated over LinkState.csr(): 2 * ecc + 2, ecc the largest eccentricity,
    within the transit subgraph (usable links between nodes that may relay),
    of the lowest-id node of each of its components."""
    rp, col, up, nt = csr["row_ptr"], csr["col"], csr["edge_up"], csr["no_transit"]
    V = rp.size - 1
    lvl = [-1] * V
    ecc_max = 0
    for s in range(V):
        if nt[s] or lvl[s] >= 0:
            continue
        lvl[s] = 0
        q = [s]
        for u in q:
            for e in range(int(rp[u]), int(rp[u + 1])):
                x = int(col[e])
                if not up[e] or nt[x] or lvl[x] >= 0:
                    continue
                lvl[x] = lvl[u] + 1
                q.append(x)
        ecc_max = max(ecc_max, lvl[q[-1]])
    return 2 * ecc_max + 2


def path_dbs(n):
    """A path p000 - p001 - ... of n nodes with unit metrics: n - 1 levels
    deep from either end (names sort in path order)."""
    names = [f"p{i:04d}" for i in range(n)]
    adjs = {nm: [] for nm in names}
    for i in range(n - 1):
        a, b = names[i], names[i + 1]
        adjs[a].append(create_adjacency(b, f"{a}-{b}", f"{b}-{a}", 1))
        adjs[b].append(create_adjacency(a, f"{b}-{a}", f"{a}-{b}", 1))
    return [AdjDb(nm, adjs[nm], i + 1) for i, nm in enumerate(names)]


def metric_graph(links, overloaded=()):
    """AdjDbs of an explicit weighted graph. links: (a, b, w_ab, w_ba) or
    (a, b, w_ab, w_ba, "down") -- one adjacency per direction with its own
    metric; "down" reports a's side overloaded (the link is unusable both
    ways). `overloaded`: names of no-transit nodes. Ids are name ranks."""
    adjs = {}
    for k, ln in enumerate(links):
        a, b, wab, wba = ln[:4]
        down = len(ln) > 4 and ln[4] == "down"
        adjs.setdefault(a, []).append(create_adjacency(b, f"{a}-{b}-{k}", f"{b}-{a}-{k}", int(wab),
                                                       overloaded=down))
        adjs.setdefault(b, []).append(create_adjacency(a, f"{b}-{a}-{k}", f"{a}-{b}-{k}", int(wba)))
    return [AdjDb(nm, adjs[nm], i + 1, overloaded=nm in overloaded)
            for i, nm in enumerate(sorted(adjs))]


def furniture(at, island=2, tag="f", unit=False):
    """(links, overloaded names) of what every limit shape carries besides
    its critical path, hung off node `at`: an ECMP diamond at -> {fa, fb} ->
    fc (3 either way, asymmetric per direction), an overloaded node fo on fa
    and fc (a destination, never a relay), a down link fa - fb, and an
    island za - zb - ... of `island` nodes nothing else reaches. unit: every
    metric 1 (the diamond is 2 either way), for unit-metric shapes."""
    fa, fb, fc, fo = (tag + x for x in "abco")
    links = [(at, fa, 1, 2), (at, fb, 2, 1), (fa, fc, 2, 1), (fb, fc, 1, 2),
             (fa, fo, 1, 3), (fc, fo, 3, 1), (fa, fb, 1, 1, "down")]
    isl = [f"z{chr(97 + t)}" for t in range(island)]
    links += [(isl[t], isl[t + 1], 5 + t, 7 + t) for t in range(island - 1)]
    if unit:
        links = [ln[:2] + (1, 1) + ln[4:] for ln in links]
    return links, {fo}


def dist_bound(csr):
    """The engine's distance bound (the l_bound loop of ospf_load_graph)
    restated over LinkState.csr(): the sum over all nodes -- overloaded ones
    too -- of the largest metric on an out-entry whose link is up; a node
    with no usable entry adds 0."""
    rp, met, up = csr["row_ptr"], csr["metric"], csr["edge_up"]
    total = 0
    for u in range(rp.size - 1):
        row = [int(met[e]) for e in range(int(rp[u]), int(rp[u + 1])) if up[e]]
        total += max(row, default=0)
    return total


def bundle(a, b, routes, hops, tag, w=1):
    """links of `routes` edge-disjoint routes of `hops` links (metric w both
    ways) from a to b over private nodes {tag}{route:03d}_{hop:03d}"""
    links = []
    for r in range(routes):
        chain = [a] + [f"{tag}{r:03d}_{i:03d}" for i in range(1, hops)] + [b]
        links += [(chain[i], chain[i + 1], w, w) for i in range(hops)]
    return links
