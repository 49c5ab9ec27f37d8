"""Shapes and batches at the budgets of the in-place repair and their
oracle-derived expectation (shared by test_host_repair_limits.py and
test_gpu_repair_limits.py).

The repair (spf_update.hip, repair_kernel) fixes the next-hop words of a
finished run after a patch that moves no distance, within hard budgets
(DESIGN.md section 2, R1 - R5): 1,024 queued nodes, 8,192 re-derivations,
next-hop words re-derived 8 at a time, LINK and NODE changes in one call, and
distances up to the u32 distance bound. Every case below is a list of AdjDbs
before a batch and the same databases with the batch applied. Rows of both
sides come from the CPU oracle's runSpf restatement; the ospf_change tuples
and the update_links / update_nodes arguments from the two CSRs; the expected
status of a root from its two oracle dist rows (and, on the budget shapes, a
count of the repair's propagation over the oracle rows); the expected
affected flags from the header's predicate in numpy. No engine row appears
anywhere in this module."""
import copy
import functools
import heapq
from types import SimpleNamespace

import numpy as np

import metric_ref
from depth_ref import INF, make_shape, rows_of, words_of
from graphs import furniture, metric_graph, random_stream
from oracle import Oracle, parse_spf_text
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState

HEAP_CAP, POPS = 1024, 8192  # kHeapCap, kPops of spf_update.hip
LINK, NODE = 0, 1            # OSPF_CHANGE_LINK, OSPF_CHANGE_NODE


# --------------------------------------------------------------- batches
# one operation of a batch, on the AdjDbs:
#   ("down", x, y, k)            x's k-th adjacency to y reports overloaded
#   ("up", x, y, k)              neither side of that link reports overloaded
#   ("metric", x, y, k, wxy, wyx)
#   ("over", x, flag)            node x's overload bit
def _adj_pair(by_name, x, y, k):
    a = [ad for ad in by_name[x].adjs if ad.other == y][k]
    b = next(ad for ad in by_name[y].adjs if ad.other == x and ad.if_name == a.other_if)
    return a, b


def apply_batch(dbs, ops):
    """a deep copy of `dbs` with the batch applied"""
    out = copy.deepcopy(dbs)
    by_name = {d.name: d for d in out}
    for op in ops:
        if op[0] == "over":
            by_name[op[1]].overloaded = bool(op[2])
            continue
        a, b = _adj_pair(by_name, *op[1:4])
        if op[0] == "down":
            a.overloaded = True
        elif op[0] == "up":
            a.overloaded = b.overloaded = False
        else:
            a.metric, b.metric = int(op[4]), int(op[5])
    return out


def csr_delta(c0, c1, node_first=False):
    """(ospf_change tuples, update_links arguments, (nodes, no_transit bits)
    for update_nodes) of two CSRs of one structure: one LINK entry per link
    whose up flag or either metric differs (a = the endpoint with the lower
    id), one NODE entry per node whose overload bit differs; LINK entries
    first unless node_first."""
    rp = c0["row_ptr"].astype(np.int64)
    owner = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    diff = (c0["edge_up"] != c1["edge_up"]) | (c0["metric"] != c1["metric"])
    links, ups = [], []
    for l in sorted(set(c0["link_id"][diff].tolist())):
        e = np.nonzero(c0["link_id"] == l)[0]
        assert e.size == 2
        lo, hi = (e[0], e[1]) if owner[e[0]] <= owner[e[1]] else (e[1], e[0])
        links.append((LINK, int(owner[lo]), int(owner[hi]),
                      int(c0["edge_up"][lo]), int(c0["metric"][lo]), int(c0["metric"][hi]),
                      int(c1["edge_up"][lo]), int(c1["metric"][lo]), int(c1["metric"][hi])))
        ups.append((int(l), int(c1["edge_up"][lo]), int(c1["metric"][lo]), int(c1["metric"][hi])))
    nodes = np.nonzero(c0["no_transit"] != c1["no_transit"])[0]
    nch = [(NODE, int(x), 0, 0, 0, 0, 0, 0, 0) for x in nodes]
    bits = [int(c1["no_transit"][x]) for x in nodes]
    return (nch + links if node_first else links + nch), ups, ([int(x) for x in nodes], bits)


# ---------------------------------------------------------------- shapes
def _mix_links():
    """MIX: the diamond r - {a, b} - v with a tail v - t - u, a second,
    untight link a = v (metric 3 both ways) and the furniture on u."""
    f, ov = furniture("u")
    links = [("r", "a", 1, 1), ("r", "b", 1, 1), ("a", "v", 1, 1), ("a", "v", 3, 3),
             ("b", "v", 1, 1), ("v", "t", 1, 1), ("t", "u", 1, 1)]
    return links + f, ov


def _mix():
    return metric_graph(*_mix_links())


MIX_BATCHES = {
    # a drains: its link to v goes down and it sets overload in one batch
    "M1": [("down", "a", "v", 0), ("over", "a", True)],
    "M2": [("metric", "a", "v", 0, 5, 5), ("over", "a", True)],
    "M3": [("up", "a", "v", 0), ("over", "a", False)],           # from the drained state
    "M4": [("over", "a", True), ("down", "b", "v", 0)],          # distances move
    # the tight link of a = v goes down, the other takes its place a -> v only
    "M5": [("down", "a", "v", 0), ("metric", "a", "v", 1, 1, 3)],
    # for root a: itself, its neighbour r, the island's za (and b, which cuts r off v)
    "M6": [("over", "a", True), ("over", "r", True), ("over", "za", True), ("over", "b", True)],
}


def _mix_before(batch):
    dbs = _mix()
    return apply_batch(dbs, MIX_BATCHES["M1"]) if batch == "M3" else dbs


def _fan(N):
    """H*: root r; a and b on r; x on a and b; N leaves on x"""
    links = [("r", "a", 1, 1), ("r", "b", 1, 1), ("a", "x", 1, 1), ("b", "x", 1, 1)]
    links += [("x", f"l{i:04d}", 1, 1) for i in range(N)]
    return metric_graph(links)


P_HEADS = 1023


def _chains(total):
    """P*: the same head; x has 1,023 children, each the head of a chain;
    `total` chain nodes in all (lengths differ by one at most)"""
    links = [("r", "a", 1, 1), ("r", "b", 1, 1), ("a", "x", 1, 1), ("b", "x", 1, 1)]
    base, extra = divmod(total, P_HEADS)
    for i in range(P_HEADS):
        chain = ["x"] + [f"c{i:04d}_{k:02d}" for k in range(base + (1 if i < extra else 0))]
        links += [(chain[k], chain[k + 1], 1, 1) for k in range(len(chain) - 1)]
    return metric_graph(links)


def _wide(K):
    """W*: root h with K distinct neighbours n0000 .. (bit j = n{j}), each on
    the far node t, which has a tail t - t1 - t2; the last neighbour has two
    parallel links to h."""
    links = []
    for j in range(K):
        links += [("h", f"n{j:04d}", 1, 1), (f"n{j:04d}", "t", 1, 1)]
    links += [("h", f"n{K - 1:04d}", 1, 1), ("t", "t1", 1, 1), ("t1", "t2", 1, 1)]
    return metric_graph(links)


WIDE = {"W8": 256, "W9": 257, "W16": 512, "W17": 513}
WIDE_BITS = (0, 255, 256, 511, 512)

# random_stream arguments and the seed the batches are drawn with. Chosen so
# that the oracle alone meets test_host_repair_limits.py's non-vacuity
# conditions (every case has a root the batch leaves at status 0 with other
# next hops and one it moves a distance of).
RND_SEEDS = (
    dict(seed=2116, n=40, p=0.15, unit=True),
    dict(seed=2119, n=50, p=0.12, unit=False),
    dict(seed=2124, n=60, p=0.10, unit=True),
    dict(seed=2105, n=70, p=0.09, unit=False),
)
RND_BATCHES = 4  # per seed


def _rnd_dbs(k):
    s = RND_SEEDS[k]
    st, _ = random_stream(s["seed"], n=s["n"], p=s["p"], unit=s["unit"],
                          wmax=4 if not s["unit"] else 20)
    return st.to_dbs()


def _link_up(by_name, d, ad):
    back = next(b for b in by_name[ad.other].adjs if b.other == d.name and b.if_name == ad.other_if)
    return not (ad.overloaded or back.overloaded)


def _rnd_ops(k, j):
    """batch j of seed k: 1 to 6 changes from {link down, link up, metric
    change, overload set, overload cleared} on distinct links and nodes; even
    batches hold both kinds."""
    dbs = _rnd_dbs(k)
    by_name = {d.name: d for d in dbs}
    rng = np.random.default_rng(1000 * RND_SEEDS[k]["seed"] + j)
    n = 1 + (2 * j) % 6
    kinds = ["link" if rng.random() < 0.6 else "node" for _ in range(n)]
    if j % 2 == 0:
        kinds = (kinds + ["link", "node"])[-max(n, 2):]
        kinds[0], kinds[1] = "link", "node"
    ops, seen = [], set()
    for kind in kinds:
        for _ in range(100):
            d = dbs[int(rng.integers(len(dbs)))]
            if kind == "node":
                if d.name in seen:
                    continue
                seen.add(d.name)
                ops.append(("over", d.name, not d.overloaded))
                break
            if not d.adjs:
                continue
            ad = d.adjs[int(rng.integers(len(d.adjs)))]
            par = [x for x in d.adjs if x.other == ad.other]
            idx = next(i for i, x in enumerate(par) if x is ad)
            key = tuple(sorted((ad.if_name, ad.other_if)))
            if key in seen:
                continue
            seen.add(key)
            up = _link_up(by_name, d, ad)
            what = rng.random()
            if not up:
                ops.append(("up", d.name, ad.other, idx))
            elif what < 0.5:
                ops.append(("down", d.name, ad.other, idx))
            else:
                back = _adj_pair(by_name, d.name, ad.other, idx)[1]
                ops.append(("metric", d.name, ad.other, idx, ad.metric + int(rng.integers(1, 4)),
                            max(1, back.metric + int(rng.integers(-1, 3)))))
            break
    return ops


def _wide_ops(name, j):
    K = WIDE[name]
    return [("down", f"n{j:04d}", "t", 0), ("down", "h", f"n{K - 1:04d}", 0)]


def _wide_bits(name):
    K = WIDE[name]
    return [j for j in WIDE_BITS if j < K - 1] + [K - 1]


# case name -> (before AdjDbs, batch, root names or None = every node)
def _cases():
    out = {}
    for b in MIX_BATCHES:
        out[f"MIX-{b}"] = (lambda b=b: _mix_before(b), MIX_BATCHES[b], None)
    for k in range(len(RND_SEEDS)):
        for j in range(RND_BATCHES):
            out[f"RND{k}-{j}"] = (lambda k=k: _rnd_dbs(k), (lambda k=k, j=j: _rnd_ops(k, j)), None)
    head = ("r", "a", "b")
    out["H1024"] = (lambda: _fan(1024), [("down", "a", "x", 0)], head + ("l0000", "l1023"))
    out["H1025"] = (lambda: _fan(1025), [("down", "a", "x", 0)], head + ("l0000", "l1024"))
    out["P8192"] = (lambda: _chains(8191), [("down", "a", "x", 0)], head + ("c0000_00", "c1022_07"))
    out["P8193"] = (lambda: _chains(8192), [("down", "a", "x", 0)], head + ("c0000_00", "c1022_07"))
    for name, K in WIDE.items():
        for j in _wide_bits(name):
            roots = ("h",) if j == 0 else ("h", "t1", "n0000", "t2", f"n{K - 1:04d}")[:4 + j % 2]
            out[f"{name}-{j}"] = (lambda K=K: _wide(K), _wide_ops(name, j), roots)
    out["L7R"] = (lambda: metric_ref.dbs_of("U32_m2"), [("down", "fa", "fc", 0)], None)
    return out


CASES = _cases()
MIX_CASES = [c for c in CASES if c.startswith("MIX")]
RND_CASES = [c for c in CASES if c.startswith("RND")]
WIDE_CASES = [c for c in CASES if c[0] == "W"]
# name -> (root, pushes, pops, largest queue) the propagation counter must give
STATED = {
    "H1024": ("r", 1025, 1025, 1024),
    "H1025": ("r", 1026, 1026, 1025),
    "P8192": ("r", 8192, 8192, 1023),
    "P8193": ("r", 8193, 8193, 1023),
}
L7R_FAR = ("n0", 2 ** 32 - 13)  # root and its largest finite distance


@functools.lru_cache(maxsize=None)
def case(name):
    """before / after shapes of a case (depth_ref.make_shape), its batch and
    its root ids (ascending)"""
    build, ops, roots = CASES[name]
    dbs = build()
    ops = ops() if callable(ops) else ops
    g0 = make_shape(name + ":before", dbs)
    g1 = make_shape(name + ":after", apply_batch(dbs, ops))
    assert g0.names == g1.names
    ids = sorted(g0.ids[r] for r in roots) if roots else list(range(g0.V))
    return SimpleNamespace(name=name, g0=g0, g1=g1, ops=ops, roots=ids,
                           W=max(words_of(g0.csr, r) for r in ids))


@functools.lru_cache(maxsize=None)
def rows(name, use_link_metric=True):
    """The oracle's rows of the case's roots before and after the batch:
    (dist0 [n, V], nh0 [n, V, W], dist1, nh1), read only"""
    c = case(name)
    out = []
    for g in (c.g0, c.g1):
        dist = np.zeros((len(c.roots), g.V), np.uint32)
        nh = np.zeros((len(c.roots), g.V, c.W), np.uint32)
        for i, r in enumerate(c.roots):
            res = parse_spf_text(g.oracle.spf_text(g.names[r], use_link_metric))
            dist[i], nh[i] = rows_of(g, res, r, c.W)
        dist.setflags(write=False)
        nh.setflags(write=False)
        out += [dist, nh]
    return tuple(out)


# ------------------------------------------------- the propagation counter
def propagate(csr, root, dist, nh, changes, hop):
    """The repair's propagation restated sequentially over the oracle's rows
    of one root (dist [V], nh [V, W] before the batch; `csr` after it): the
    changes in order, then a min-heap on (dist, id), successors in row order;
    a node is queued when its next-hop words differ from what a pull over its
    tight, transit, reached in-neighbours gives. -> dict(pushes, pops, qmax,
    moved): the counts without any budget, and whether a distance would move.
    It exists to count against the budgets; rows never come from it."""
    rp, col, met, twin, up, nt = (csr[k] for k in ("row_ptr", "col", "metric", "twin", "edge_up",
                                                   "no_transit"))
    D = [int(x) for x in dist]
    H = [int.from_bytes(np.ascontiguousarray(w, "<u4").tobytes(), "little") for w in nh]
    nbr = sorted({int(x) for x in col[int(rp[root]):int(rp[root + 1])]} - {root})
    bit = {v: k for k, v in enumerate(nbr)}
    out = dict(pushes=0, pops=0, qmax=0, moved=False)
    heap = []

    def transit(x):
        return x == root or not nt[x]

    def wt(e):
        return 1 if hop else int(met[e])

    def rederive(y):
        if y == root:
            return
        best, acc = INF, 0
        for e in range(int(rp[y]), int(rp[y + 1])):
            x = int(col[e])
            if not up[e] or x == y or D[x] == INF or not transit(x):
                continue
            c = D[x] + wt(int(twin[e]))
            best = min(best, c)
            if c == D[y]:
                acc |= (1 << bit[y]) if x == root else H[x]
        if best != D[y]:
            out["moved"] = True
        elif acc != H[y]:
            H[y] = acc
            heapq.heappush(heap, (D[y], y))
            out["pushes"] += 1
            out["qmax"] = max(out["qmax"], len(heap))

    def successors(x, also_shorter):
        for e in range(int(rp[x]), int(rp[x + 1])):
            y = int(col[e])
            if not up[e] or y == x:
                continue
            nd = D[x] + wt(e)
            if also_shorter and nd < D[y]:
                out["moved"] = True
            if D[y] != INF and nd == D[y]:
                rederive(y)

    for ch in changes:
        if ch[0] == NODE:
            x = ch[1]
            if x != root and D[x] != INF:
                successors(x, transit(x))
            continue
        _, a, b, up0, wab0, wba0, up1, wab1, wba1 = ch
        for u, v, w0, w1 in ((a, b, wab0, wab1), (b, a, wba0, wba1)):
            if hop:
                w0 = w1 = 1
            if D[u] == INF:
                continue
            t0 = bool(up0) and D[u] + w0 == D[v]
            if not transit(u):
                if t0:
                    rederive(v)
                continue
            if up1 and D[u] + w1 < D[v]:
                out["moved"] = True
            if t0 != (bool(up1) and D[u] + w1 == D[v]):
                rederive(v)
    while heap:
        _, x = heapq.heappop(heap)
        out["pops"] += 1
        if transit(x):
            successors(x, False)
    return out


@functools.lru_cache(maxsize=None)
def counts(name, use_link_metric=True, node_first=False):
    """propagate() of every root of the case whose oracle dist row the batch
    leaves alone (None for the others), in root order"""
    c = case(name)
    d0, n0, d1, _ = rows(name, use_link_metric)
    ch = csr_delta(c.g0.csr, c.g1.csr, node_first)[0]
    return [propagate(c.g1.csr, r, d0[i], n0[i], ch, not use_link_metric)
            if np.array_equal(d0[i], d1[i]) else None for i, r in enumerate(c.roots)]


def expected_status(name, use_link_metric=True, node_first=False):
    """[n] u32: 1 where the oracle's dist row differs before and after, or
    where the propagation passes a budget (more than 1,024 queued at once or
    more than 8,192 re-derived nodes popped); else 0"""
    d0, _, d1, _ = rows(name, use_link_metric)
    moved = (d0 != d1).any(axis=1)
    over = [k is not None and (k["qmax"] > HEAP_CAP or k["pops"] > POPS)
            for k in counts(name, use_link_metric, node_first)]
    return (moved | np.array(over)).astype(np.uint32)


# -------------------------------------------------- the affected predicate
def affected(csr, dist, changes, hop):
    """ospf_affected_roots' stated predicate over before-distances dist
    [n, V], the change tuples and the patched CSR (read for NODE entries),
    transit ignored: [n] u8"""
    rp, col, met, up = (csr[k] for k in ("row_ptr", "col", "metric", "edge_up"))
    D = dist.astype(np.uint64)
    inf = np.uint64(INF)
    hit = np.zeros(D.shape[0], bool)
    for ch in changes:
        if ch[0] == NODE:
            x = ch[1]
            dx = D[:, x]
            live = (dx != inf) & (dx != 0)
            for e in range(int(rp[x]), int(rp[x + 1])):
                if up[e]:
                    w = np.uint64(1 if hop else int(met[e]))
                    hit |= live & (dx + w <= D[:, int(col[e])])
            continue
        _, a, b, up0, wab0, wba0, up1, wab1, wba1 = ch
        da, db = D[:, a], D[:, b]
        for du, dv, w0, w1 in ((da, db, wab0, wab1), (db, da, wba0, wba1)):
            w0, w1 = (np.uint64(1 if hop else w) for w in (w0, w1))
            if up0:
                hit |= (du != inf) & (du + w0 == dv)
            if up1:
                hit |= (du != inf) & (du + w1 <= dv)
    return hit.astype(np.uint8)


# ------------------------------------------- a drain through odl::LinkState
def drain_publications():
    """MIX, then a's AdjDb three times: overloaded with its link to v down
    (M1), back as it was (M3), overloaded with that link at metric 5 (M2)"""
    dbs = case("MIX-M1").g0.stream.to_dbs()
    out = []
    for b in ("M1", None, "M2"):
        after = apply_batch(dbs, MIX_BATCHES[b]) if b else dbs
        out.append(AdjDbStream.from_dbs([d for d in after if d.name == "a"]))
    return AdjDbStream.from_dbs(dbs), out


def check_linkstate_drain(host):
    first, pubs = drain_publications()
    o, p = Oracle(), LinkState()
    if host:
        p.set_host_spf(True)
    assert o.apply(first) == p.apply(first)
    p.set_incremental(True)
    names = p.node_names()
    p.prefetch(names)
    p.prefetch(names, False)
    for k, upd in enumerate(pubs):
        assert o.apply(upd) == p.apply(upd)
        for r in names:
            for mode in (True, False):
                assert p.spf_text(r, mode) == o.spf_text(r, mode), (k, r, mode)
    stats = p.incremental_stats()
    assert stats["patches"] > 0 and stats["kept"] > 0, stats
