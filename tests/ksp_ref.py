"""Shapes at the KSP2 path's trace and rerun budgets and their oracle-derived
expectation (shared by test_host_ksp_limits.py and test_gpu_ksp_limits.py).

The KSP2 path (spf_ksp2.hip, run_ksp2) has hard budgets, each with a fallback
that must be exact: 256 links per path, the
claimed links a trace's hash holds (1,536; 768 in front of the 16-wave
kernel; 384 in the decremental kernel), the record's words, the decremental
kernel's ignore list (256), affected set (192), map (384 keys) and scanned
out-links (4,096), the source cut (16 of the source's links) and the 16
candidates of a heavy round. Every shape below sits on one of them or just
past it. Paths and path counts come from the CPU oracle (kth_paths), masked
distances, affected sets and hints from a plain restatement over
LinkState.csr() -- never from the engine."""
import functools
import heapq

import numpy as np

from depth_ref import make_shape
from graphs import bundle, furniture, metric_graph, path_dbs

INF = 0xFFFFFFFF
RERUN, OVF1, OVF2 = 0x1, 0x2, 0x4


def _with_furniture(links, at, unit=True, island=2):
    f, ov = furniture(at, island=island, unit=unit)
    return metric_graph(links + f, ov)


def _ring(n_long, seed=None):
    """P*: a ring r0000 .. of n_long + 1 nodes; r0000 - r0001 is the direct
    link (metric 1), the long way round has n_long links. seed: metrics 1..30
    per direction on the other links (their sum stays above 1)."""
    N = n_long + 1
    rng = None if seed is None else np.random.default_rng(seed)
    links = []
    for i in range(N):
        a, b = f"r{i:04d}", f"r{(i + 1) % N:04d}"
        if i == 0 or rng is None:
            links.append((a, b, 1, 1))
        else:
            links.append((a, b, int(rng.integers(1, 31)), int(rng.integers(1, 31))))
    return _with_furniture(links, "r0000", unit=seed is None)


def _bundles(p1, h1, p2, h2, unit=True):
    """C* / D* / S*: s and d joined by p1 routes of h1 links (k = 1) and p2
    routes of h2 > h1 links (k = 2 once the first bundle is ignored)."""
    assert h2 > h1
    return _with_furniture(bundle("s", "d", p1, h1, "u") + bundle("s", "d", p2, h2, "v"), "s", unit)


def _fat(direct):
    """I256 / I257: s - n01 - ... - n31 - d over 8 parallel links of metric 1
    per hop (8 k = 1 paths, 256 links, 8 of them at s, 32 nodes behind them),
    a direct s - d link of metric `direct` (32: a ninth k = 1 path, 257 links;
    33: the k = 2 path) and a detour s - y - d of 20 + 20."""
    chain = ["s"] + [f"n{i:02d}" for i in range(1, 32)] + ["d"]
    links = [(chain[i], chain[i + 1], 1, 1) for i in range(32) for _ in range(8)]
    links += [("s", "d", direct, direct), ("s", "y", 20, 20), ("y", "d", 20, 20)]
    return _with_furniture(links, "s", unit=False)


def _comb(T):
    """A*: s - m is m's only tight support; behind m a chain t0001 .. of T
    nodes; the detour s - x1 - x2 - m. Ignoring s - m (the k = 1 path to m)
    moves m and the chain: T + 1 affected nodes."""
    chain = ["m"] + [f"t{i:04d}" for i in range(1, T + 1)]
    links = [("s", "m", 1, 1), ("s", "x1", 1, 1), ("x1", "x2", 1, 1), ("x2", "m", 1, 1)]
    links += [(chain[i], chain[i + 1], 1, 1) for i in range(T)]
    return _with_furniture(links, "s")


def _fan(n, other):
    """E* / F*: s - m (m's only tight support) and s - `other`; n leaves
    l0000 .. on both m and `other`, so ignoring s - m affects m alone and the
    leaves keep a support. m's row has n + 1 entries (kEdge). other = "q"
    sorts after m: the leaves' hint (their last support) stands, the map holds
    m alone; other = "b" sorts before m: every leaf loses its hint, n + 1 keys."""
    links = [("s", "m", 1, 1), ("s", other, 1, 1)]
    for i in range(n):
        links += [("m", f"l{i:04d}", 1, 1), (other, f"l{i:04d}", 1, 1)]
    return _with_furniture(links, "s")


H_PAD, H_CHAIN = 40, 4


def _heavy(fail, extra=()):
    """H*: d has c = fail + 2 tight predecessors p001 .. in row order, behind
    H_PAD untight ones (a000 ..: leaves of d), so the candidates straddle a
    64-lane chunk from fail = 24 on. Each p hangs on a private chain of
    H_CHAIN nodes; the chains of p001 .. p(c-1) end at b0, whose single link to
    s path 1 claims; p(c)'s chain ends at b1, the second source link."""
    c = fail + 2
    links = [("s", "b0", 1, 1), ("s", "b1", 1, 1)]
    links += [("d", f"a{i:03d}", 1, 1) for i in range(H_PAD)]
    for j in range(1, c + 1):
        chain = ["b1" if j == c else "b0"] + [f"q{j:03d}_{i}" for i in range(H_CHAIN)] + [f"p{j:03d}", "d"]
        links += [(chain[i], chain[i + 1], 1, 1) for i in range(len(chain) - 1)]
    return _with_furniture(links + list(extra), "s")


def _heavy2(fail):
    """G*: H* plus a side route s - e1 - .. - d one link shorter than the
    ways through the candidates: k = 1 is that route alone, ignoring it moves
    d and its leaves only, and the search with `fail` failing candidates runs
    in the k = 2 trace (the decremental kernel and the 16-wave kernel behind
    it, whose queue is counted)."""
    side = ["s"] + [f"e{i}" for i in range(1, H_CHAIN + 2)] + ["d"]
    return _heavy(fail, [(side[i], side[i + 1], 1, 1) for i in range(len(side) - 1)])


K_CAND = 6


def _look(row):
    """K16 / K17: d's tight predecessors p001 .. p006 in row order, each with
    a row of exactly `row` entries (d, its one tight predecessor, leaves);
    p001 .. p005 hang on b0, whose single link to s path 1 claims, p006 on b1.
    Path 2's search meets p002 (entered: b0 is not yet dead), then p003 as a
    call's first candidate and p004, p005 as later lanes' candidates with no
    open pathLink: probed and marked dead at 16 entries, entered at 17."""
    links = [("s", "b0", 1, 1), ("s", "b1", 1, 1)]
    for j in range(1, K_CAND + 1):
        p = f"p{j:03d}"
        links += [("b1" if j == K_CAND else "b0", p, 1, 1), (p, "d", 1, 1)]
        links += [(p, f"w{j:03d}_{i:02d}", 1, 1) for i in range(row - 2)]
    return _with_furniture(links, "s")


def _levels(far):
    """V252: overloaded s and t on the ends of a 251-node transit chain whose
    middle node a125 has the lowest id (depth bound 2 * 125 + 2 = 252); the
    direct s - t link is k = 1, the masked distance is 252 (level byte 253).
    V253 / V254 / V255 (far = the masked distance): a chain of far - 1 nodes
    whose lowest id a(far - 127) is 125 links from the far end and has a
    shortcut to c000, so the bound is still 252; the links s - c000, from the
    seed to the far end and on to t are doubled. k = 1 takes the shortcut (128
    links), the masked run must walk the whole chain over the second links:
    distance `far`, level byte far + 1."""
    deep = far > 252
    n = far - 1
    mid = n - 126 if deep else 125
    nm = [f"a{i:03d}" if i == mid else f"c{i:03d}" for i in range(n)]
    links = []
    for i in range(n - 1):
        links += [(nm[i], nm[i + 1], 1, 1)] * (2 if deep and i >= mid else 1)
    if deep:
        links += [(nm[mid], nm[0], 1, 1)] + [("s", nm[0], 1, 1)] * 2 + [(nm[-1], "t", 1, 1)] * 2
    else:
        links += [("s", nm[0], 1, 1), (nm[-1], "t", 1, 1), ("s", "t", 1, 1)]
    f, ov = furniture(nm[mid], unit=True)
    return metric_graph(links + f, ov | {"s", "t"})


X_FAN = 14


def _mixed():
    """X: two combs (s - m its only tight support, the detour s - x1 - x2 -
    m) with a two-level tree of 14 + 14 * 14 nodes behind each m over doubled
    links: every tree node's k = 1 path goes through s - m, ignoring it moves
    m and the whole tree (211 affected nodes: the decremental kernel gives
    each of these 420 runs up); dp (17 of the source's links) and dq (288
    ignored links) are presplit."""
    links = []
    for c in "ab":
        m = f"m{c}"
        links += [("s", m, 1, 1), ("s", f"x{c}1", 1, 1), (f"x{c}1", f"x{c}2", 1, 1), (f"x{c}2", m, 1, 1)]
        for i in range(X_FAN):
            ch = f"c{c}{i:02d}"
            links += [(m, ch, 1, 1)] * 2
            for k in range(X_FAN):
                links += [(ch, f"g{c}{i:02d}{k:02d}", 1, 1)] * 2
    links += bundle("s", "dp", 17, 2, "u") + bundle("s", "dp", 2, 3, "v")
    links += bundle("s", "dq", 9, 32, "y") + bundle("s", "dq", 2, 33, "z_")
    return _with_furniture(links, "s")


def _rec():
    """R / B: k = 1 of 2 routes x 2 links (7 record words), k = 2 of 2 routes
    x 3 links (9 words)."""
    return _bundles(2, 2, 2, 3)


BUILD = {
    "P256": lambda: _ring(256), "P257": lambda: _ring(257),
    "P256w": lambda: _ring(256, seed=256), "P257w": lambda: _ring(257, seed=257),
    "L256": lambda: path_dbs(257), "L257": lambda: path_dbs(258),
    "C768": lambda: _bundles(24, 32, 2, 33), "C800": lambda: _bundles(25, 32, 2, 33),
    "C1536": lambda: _bundles(48, 32, 2, 33), "C1568": lambda: _bundles(49, 32, 2, 33),
    "D384": lambda: _bundles(4, 7, 48, 8), "D392": lambda: _bundles(4, 7, 49, 8),
    "R": _rec,
    "I256": lambda: _fat(33), "I257": lambda: _fat(32),
    "S16": lambda: _bundles(16, 2, 2, 3), "S17": lambda: _bundles(17, 2, 2, 3),
    "A192": lambda: _comb(191), "A193": lambda: _comb(192),
    "E4096": lambda: _fan(4095, "q"), "E4097": lambda: _fan(4096, "q"),
    "F384": lambda: _fan(383, "b"), "F385": lambda: _fan(384, "b"),
    **{f"H{n}": (lambda n=n: _heavy(n)) for n in (15, 16, 17, 31, 32, 33, 64, 65)},
    **{f"G{n}": (lambda n=n: _heavy2(n)) for n in (15, 64, 65)},
    "K16": lambda: _look(16), "K17": lambda: _look(17),
    "V252": lambda: _levels(252),
    **{f"V{n}": (lambda n=n: _levels(n)) for n in (253, 254, 255)},
    "X": _mixed,
}

# what each shape states about its (src, dst) query. k1 / k2: (paths, links of
# each path); cap: the path_cap / ODL_KSP_CAP the query runs at; status: the
# engine's status word at that cap; route: who answers the k = 2 rerun
# ("decr": the decremental kernel, "full": it gives the run up, "presplit":
# sent to the full reruns before it starts, None: no rerun); nign / at_src:
# ignored links and how many touch src; A / edges / keys: affected nodes, row
# entries of the affected transit nodes, nodes whose hint is lost; cut: the
# ignored links are all the source has.
def _s(src, dst, k1, k2, cap=1024, status=RERUN, route="decr", **kw):
    return dict(src=src, dst=dst, k1=k1, k2=k2, cap=cap, status=status, route=route, **kw)


STATED = {
    "P256": _s("r0000", "r0001", (1, 1), (1, 256), nign=1, unit=True, deep=True),
    "P257": _s("r0000", "r0001", (1, 1), (1, 257), status=RERUN | OVF2, nign=1, unit=True, deep=True),
    "P256w": _s("r0000", "r0001", (1, 1), (1, 256), nign=1, unit=False, deep=True),
    "P257w": _s("r0000", "r0001", (1, 1), (1, 257), status=RERUN | OVF2, nign=1, unit=False, deep=True),
    # (the chain's first link is the source's only one: the decremental kernel
    # sees the source cut off and answers "no paths" before any budget counts)
    "L256": _s("p0000", "p0256", (1, 256), (0, 0), nign=256, at_src=1, A=256, cut=True, unit=True,
               deep=True),
    "L257": _s("p0000", "p0257", (1, 257), (0, 0), status=OVF1 | OVF2, route=None, unit=True, deep=True),
    "C768": _s("s", "d", (24, 32), (2, 33), nign=768, at_src=24, route="presplit", unit=True),
    "C800": _s("s", "d", (25, 32), (2, 33), nign=800, at_src=25, route="presplit", unit=True),
    "C1536": _s("s", "d", (48, 32), (2, 33), cap=2048, nign=1536, at_src=48, route="presplit", unit=True),
    "C1568": _s("s", "d", (49, 32), (2, 33), cap=2048, status=OVF1 | OVF2, route=None, unit=True),
    "D384": _s("s", "d", (4, 7), (48, 8), nign=28, at_src=4, A=25, unit=True),
    "D392": _s("s", "d", (4, 7), (49, 8), nign=28, at_src=4, A=25, route="full", unit=True),
    "R": _s("s", "d", (2, 2), (2, 3), nign=4, at_src=2, A=3, unit=True),
    "I256": _s("s", "d", (8, 32), (1, 1), nign=256, at_src=8, A=32, unit=False),
    "I257": _s("s", "d", (9, None), (1, 2), nign=257, at_src=9, A=32, route="presplit", unit=False),
    "S16": _s("s", "d", (16, 2), (2, 3), nign=32, at_src=16, A=17, unit=True),
    "S17": _s("s", "d", (17, 2), (2, 3), nign=34, at_src=17, A=18, route="presplit", unit=True),
    "A192": _s("s", "m", (1, 1), (1, 3), nign=1, at_src=1, A=192, unit=True, deep=True),
    "A193": _s("s", "m", (1, 1), (1, 3), nign=1, at_src=1, A=193, route="full", unit=True, deep=True),
    "E4096": _s("s", "m", (1, 1), (1, 3), nign=1, at_src=1, A=1, edges=4096, keys=1, unit=True),
    "E4097": _s("s", "m", (1, 1), (1, 3), nign=1, at_src=1, A=1, edges=4097, keys=1, route="full", unit=True),
    "F384": _s("s", "m", (1, 1), (1, 3), nign=1, at_src=1, A=1, edges=384, keys=384, unit=True),
    "F385": _s("s", "m", (1, 1), (1, 3), nign=1, at_src=1, A=1, edges=385, keys=385, route="full", unit=True),
    # affected: b0, b1, every chain and candidate, d and its leaves
    **{f"H{n}": _s("s", "d", (2, H_CHAIN + 3), (0, 0), nign=2 * (H_CHAIN + 3), at_src=2, unit=True,
                   fail=n, A=(H_CHAIN + 1) * (n + 2) + 3 + H_PAD,
                   route="decr" if (H_CHAIN + 1) * (n + 2) + 3 + H_PAD <= 192 else "full")
       for n in (15, 16, 17, 31, 32, 33, 64, 65)},
    # k = 1 is the side route; d, its leaves and the side route move
    **{f"G{n}": _s("s", "d", (1, H_CHAIN + 2), (2, H_CHAIN + 3), nign=H_CHAIN + 2, at_src=1,
                   A=1 + H_PAD + H_CHAIN + 1, unit=True, fail=n)
       for n in (15, 64, 65)},
    # affected: b0, b1, the candidates with their leaves, d
    "K16": _s("s", "d", (2, 3), (0, 0), nign=6, at_src=2, A=2 + K_CAND * 15 + 1, unit=True, row=16),
    "K17": _s("s", "d", (2, 3), (0, 0), nign=6, at_src=2, A=2 + K_CAND * 16 + 1, unit=True, row=17),
    "V252": _s("s", "t", (1, 1), (1, 252), nign=1, at_src=1, A=1, unit=True, at="a125", bound=252),
    # (255: past the level bytes of the multi-source reruns its route leads to)
    **{f"V{n}": _s("s", "t", (1, 128), (1, n), nign=128, at_src=1, route="full", unit=True,
                   status=RERUN | (OVF2 if n >= 255 else 0),
                   at=f"a{n - 127:03d}", bound=252, far=n) for n in (253, 254, 255)},
}
STATED["X"] = _s("s", "dp", (17, 2), (2, 3), nign=34, at_src=17, route="presplit", unit=True)
R_WORDS = (7, 9)  # the record words of R's k = 1 and k = 2


@functools.lru_cache(maxsize=None)
def shape(name):
    """stream, oracle, node names (id order), ids by name and CSR of a shape"""
    return make_shape(name, BUILD[name]())


@functools.lru_cache(maxsize=None)
def paths(name, dst=None):
    """the oracle's (k = 1 paths, k = 2 paths) of the shape's query, each path
    a list of link keys src -> dst. Shared by the tests: read only."""
    g, st = shape(name), STATED[name]
    dst = dst or st["dst"]
    return tuple(tuple(tuple(p) for p in g.oracle.kth_paths(st["src"], dst, k)) for k in (1, 2))


def mixed_dsts():
    """X's batch: every tree node of both combs (420 runs the decremental
    kernel gives up), the two presplit destinations, and s, an island node
    and a comb's m twice"""
    g = shape("X")
    tree = [nm for nm in g.names if nm[0] in "cg" and nm[1] in "ab"]
    return tree[:200] + ["dp", "s"] + tree[200:] + ["dq", "za", "ma", "ma"]


def past_levels(name):
    """the shape's k = 2 rerun goes to the multi-source reruns (depth bound <=
    253, given up by the decremental kernel) with a masked distance past
    their last level byte (254 is the last)"""
    st = STATED[name]
    return st.get("far", 0) >= 255 and st["route"] == "full" and st.get("bound", 254) <= 253


def claims(ps):
    return sum(len(p) for p in ps)


def record_words(ps):
    """words of an engine record: the path count, then per path its length
    and its link ids"""
    return 1 + sum(1 + len(p) for p in ps)


def key_ends(key):
    """the two node names of a link key "a%ifa|b%ifb" """
    return tuple(side.split("%")[0] for side in key.split("|"))


# ------------------------------------------------- the CSR restatement
def masked_dist(csr, src, ignore=()):
    """runSpf(src, link metrics, ignored link ids) restated over the CSR:
    dist [V] (INF: unreached). A node other than src relays only when it is
    not no_transit; links that are down or ignored are not used."""
    rp, col, met, lid, up, nt = (csr[k] for k in ("row_ptr", "col", "metric", "link_id", "edge_up",
                                                  "no_transit"))
    ign = set(int(x) for x in ignore)
    V = rp.size - 1
    dist = [INF] * V
    dist[src] = 0
    heap = [(0, src)]
    while heap:
        d, u = heapq.heappop(heap)
        if d != dist[u] or (u != src and nt[u]):
            continue
        for e in range(int(rp[u]), int(rp[u + 1])):
            x = int(col[e])
            if not up[e] or int(lid[e]) in ign or x == u:
                continue
            nd = d + int(met[e])
            if nd < dist[x]:
                dist[x] = nd
                heapq.heappush(heap, (nd, x))
    return dist


def route(csr, src, ignore, k2):
    """who answers a k = 2 rerun, from the budgets: more than 256 ignored
    links or 16 of the source's are presplit; a cut-off source is the
    decremental kernel's; more than 192 affected nodes, 384 keys, 4,096 row
    entries or 384 claimed links make it give the run up"""
    rp, col, lid = csr["row_ptr"], csr["col"], csr["link_id"]
    ign = set(int(x) for x in ignore)
    at_src = len({int(lid[e]) for e in range(int(rp[src]), int(rp[src + 1]))} & ign)
    if len(ign) > 256 or at_src > 16:
        return "presplit"
    if source_cut(csr, src, ignore):
        return "decr"
    A = affected(csr, src, ignore)
    full = len(A) > 192 or lost_hints(csr, src, ignore) > 384 or \
        owned_entries(csr, A, src) > 4096 or claims(k2) > 384
    return "full" if full else "decr"


def source_cut(csr, src, ignore):
    """every usable link of src is ignored: the masked rerun reaches only src"""
    rp, col, lid, up = (csr[k] for k in ("row_ptr", "col", "link_id", "edge_up"))
    ign = set(int(x) for x in ignore)
    return not any(up[e] and int(col[e]) != src and int(lid[e]) not in ign
                   for e in range(int(rp[src]), int(rp[src + 1])))


def affected(csr, src, ignore):
    """ids of the nodes whose masked distance differs from the source's row"""
    base, masked = masked_dist(csr, src), masked_dist(csr, src, ignore)
    return [v for v in range(len(base)) if base[v] != masked[v]]


def owned_entries(csr, A, src):
    """row entries of the affected nodes that may relay (what their expansion scans)"""
    rp, nt = csr["row_ptr"], csr["no_transit"]
    return sum(int(rp[v + 1]) - int(rp[v]) for v in A if v == src or not nt[v])


def supports(csr, src, base, v):
    """(tail, link id) of v's tight in-links in row order: u relays (or is
    src), the link is up, dist(u) + metric(u -> v) == dist(v)"""
    rp, col, met, lid, up, nt, twin = (csr[k] for k in ("row_ptr", "col", "metric", "link_id",
                                                        "edge_up", "no_transit", "twin"))
    out = []
    if v == src or base[v] == INF:
        return out
    for e in range(int(rp[v]), int(rp[v + 1])):
        u = int(col[e])
        if not up[e] or u == v or base[u] == INF or (u != src and nt[u]):
            continue
        if base[u] + int(met[int(twin[e])]) == base[v]:
            out.append((u, int(lid[e])))
    return out


def lost_hints(csr, src, ignore):
    """how many nodes lose their hint (their last support in row order): its
    link is ignored, or its tail is affected"""
    base = masked_dist(csr, src)
    A, ign = set(affected(csr, src, ignore)), set(int(x) for x in ignore)
    n = 0
    for v in range(len(base)):
        sup = supports(csr, src, base, v)
        if sup and (sup[-1][1] in ign or sup[-1][0] in A):
            n += 1
    return n
