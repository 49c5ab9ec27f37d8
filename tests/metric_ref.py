"""Weighted shapes at the engine's metric and distance limits and their
oracle-derived expectation (shared by test_host_metric_limits.py and
test_gpu_metric_limits.py).

The weighted half of the engine has hard-coded limits (DESIGN.md section 2,
L1 - L7): packed {colx, w | rw << 16} entries while every metric <= 0xFFFF;
the bucketed Dial's packed state with a distance field of 32 - K bits
(K = 8 / 16 next-hop bits); the ring Dial's 64 buckets; the lane derive's u16
slot table (metrics <= 0xFFFE); the cover graph's 16-bit leaf in-link metric;
the closure's 2^30; and the u32 range, refused from a distance bound of
2^32 - 1. Every shape below sits on one of them or just past it; dist rows,
next-hop rows and digests come from the CPU oracle's runSpf restatement --
never from the engine's rows."""
import functools

import numpy as np

from depth_ref import INF, expected_rows, make_shape, oracle_digests, words_of  # noqa: F401
from graphs import dist_bound, drained_fabric, furniture, metric_graph
from oracle import parse_spf_text
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState

M16 = 0xFFFF


def _ring(names, rng, choices, chords=()):
    """ring + chords over `names`, each direction's metric drawn on its own"""
    n = len(names)
    pairs = [(i, (i + 1) % n) for i in range(n)] + list(chords)
    return [(names[i], names[j], int(rng.choice(choices)), int(rng.choice(choices)))
            for i, j in pairs]


def _p(last):
    """P16 / P17: a 16-ring with chords, metrics from {1, 2, 0xFFFE, 0xFFFF}
    per direction; p03 -> p04 is 0xFFFF (P16) or 0x10000 (P17), 0xFFFF back,
    and the only short way from p03 to p04."""
    rng = np.random.default_rng(16)
    names = [f"p{i:02d}" for i in range(16)]
    links = _ring(names, rng, [1, 2, 0xFFFE, M16], chords=[(0, 7), (5, 12), (8, 14), (1, 10), (6, 13)])
    links = [ln for ln in links if {ln[0], ln[1]} != {"p03", "p04"}]
    links.append(("p03", "p04", last, M16))
    f, ov = furniture("p00")
    return links + f, ov


def _k(K, off, nbrs):
    """K8_* / K16_*: root k0 -- c1 -- c2 -- c3 -- c4 (4 links) and a diamond
    c4 -> {e1, e2} -> e3; dist(k0, e3) = (0xFFFFFFFF >> K) + off is the
    largest finite distance from k0. k0 has `nbrs` distinct neighbours: c1,
    the furniture's fa and fb, and pendant nodes q*."""
    target = (0xFFFFFFFF >> K) + off
    step = (target - 3) // 4
    fwd = [step, step + 1, step - 1, target - 3 - 3 * step]
    chain = ["k0", "c1", "c2", "c3", "c4"]
    links = [(chain[i], chain[i + 1], fwd[i], 2 + i) for i in range(4)]
    links += [("c4", "e1", 1, 2), ("c4", "e2", 2, 1), ("e1", "e3", 2, 1), ("e2", "e3", 1, 2)]
    links += [("k0", f"q{i:02d}", 1 + i % 3, 2) for i in range(nbrs - 3)]
    f, ov = furniture("k0")
    return links + f, ov


def _knbr():
    """KNBR: hubs h08, h09, h16, h17 with exactly 8, 9, 16 and 17 distinct
    neighbours (the others' links and pendant nodes), in a path with 0x7000
    onward and 0x4000 back between hubs: across the automatic K = 8 / 16 /
    unpacked choice, with distances on either side of 0xFFFF."""
    hubs = {"h08": 8, "h09": 9, "h16": 16, "h17": 17}
    order = list(hubs)
    links = [(order[i], order[i + 1], 0x7000, 0x4000 - i) for i in range(3)]
    f, ov = furniture("h08")
    for j, (h, n) in enumerate(hubs.items()):
        have = sum(h in (a, b) for a, b, *_ in links) + (2 if h == "h08" else 0)
        links += [(h, f"{h}q{i:02d}", 0x1000 * (1 + i % 3), 1 + j) for i in range(n - have)]
    return links + f, ov


def _r(M):
    """R63 / R64: a 22-ring with chords, metrics 1 .. 62, and r05 -> r06 at
    M = the largest metric beside r05's metric-1 edges (one relaxation spans
    the whole ring of buckets)."""
    rng = np.random.default_rng(63)
    names = [f"r{i:02d}" for i in range(22)]
    links = _ring(names, rng, np.arange(1, 63), chords=[(0, 9), (3, 15), (7, 18), (11, 20), (2, 13)])
    links = [ln for ln in links if "r05" not in ln[:2]]
    links += [("r05", "r06", M, 40), ("r04", "r05", 7, 1), ("r05", "r16", 1, 9)]
    f, ov = furniture("r00", island=2 if M == 63 else 3)  # R64: V = 29, not a multiple of 4
    return links + f, ov


def _h(top):
    """H129_*: hubs h0 and h1 over the same 129 spokes s000 .. s128 with
    different metrics (a run for the lane kernel's shared slot rows); a ring
    s000 .. s127 of metric 1 gives the hubs ECMP; s128 hangs off the hubs
    alone, h0 -> s128 = `top` (h0's and the graph's largest metric, and the
    shortest way there: bit 128, word 4); s010 is overloaded, h0 - s020 is
    down. A 5-node island brings V to 140 (V % 4 == 0: vector loads)."""
    links = []
    for i in range(128):
        links.append(("h0", f"s{i:03d}", 10 + i % 3, 7 + i % 5) + (("down",) if i == 20 else ()))
        links.append(("h1", f"s{i:03d}", 20 + i % 4, 9 + i % 2))
        links.append((f"s{i:03d}", f"s{(i + 1) % 128:03d}", 1, 1))
    links += [("h0", "s128", top, 3), ("h1", "s128", 0xFFFD, 4)]
    f, ov = furniture("s000", island=5)
    return links + f, ov | {"s010"}


def _c(inlink):
    """C65535 / C65536: an 8-ring with chords (metrics 1 .. 50,000) and a leaf
    lf on c01 and c02: c01 -> lf = `inlink` (the cover -> leaf direction), c02
    -> lf = 65530 with c01 - c02 at 5, so at 65535 both ways to lf tie."""
    rng = np.random.default_rng(5)
    names = [f"c{i:02d}" for i in range(8)]
    links = _ring(names, rng, np.arange(1, 50001), chords=[(0, 4), (2, 6), (3, 7)])
    links = [ln for ln in links if {ln[0], ln[1]} != {"c01", "c02"}]
    links += [("c01", "c02", 5, 5), ("c01", "lf", inlink, 3), ("c02", "lf", 65530, 4)]
    f, ov = furniture("c00")
    return links + f, ov


def _u(bound):
    """U32_*: leaf root lr with neighbours n0 and n1; n0's only other link is
    to the overloaded fo, so its only way onward is back through lr:
    w(lr -> n0) + D_n0(n1) = A + (16 + A) = 2^32 with A = 2^31 - 8, while
    dist(n0, x) = 16 + A + (2^31 - 24) = 2^32 - 16 is a true distance. The
    island link's metric tops the distance bound up to `bound`."""
    A = 2 ** 31 - 8
    links = [("lr", "n0", A, 16), ("lr", "n1", A, 3), ("n1", "x", 2 ** 31 - 24, 2)]
    f, ov = furniture("x")
    links += f[:-1] + [("n0", "fo", 1, 1)]
    base = dist_bound(LinkState(stream=AdjDbStream.from_dbs(
        metric_graph(links + [("za", "zb", 1, 1)], ov))).csr())
    return links + [("za", "zb", bound - base + 1, 1)], ov


def _cl(bound):
    """CL30_*: the fabric plan_wcover takes the closure on, one rack uplink
    (rack -> fabric switch: no leaf in-link) raised so that the distance
    bound is exactly `bound`. 40 pods is the smallest tried that keeps the
    closure: with 6, 8, 12, 16 or 24 pods (4 spines per plane; 12 and 24 with
    2) the cover sweep plans the Dial for every cover row."""
    dbs = drained_fabric(40, 4, seed=5, drain=0.0, down=0.0, weighted_seed=11,
                         ssw_per_plane=4).to_dbs()
    base = dist_bound(LinkState(stream=AdjDbStream.from_dbs(dbs)).csr())
    rack = next(d for d in dbs if d.name == "3-7-5")
    rest = max(a.metric for a in rack.adjs)
    rack.adjs[0].metric = bound - (base - rest)
    assert rack.adjs[0].metric > rest
    return dbs


BUILD = {
    "P16": lambda: _p(M16), "P17": lambda: _p(0x10000),
    "K16_m1": lambda: _k(16, -1, 12), "K16_0": lambda: _k(16, 0, 12), "K16_p1": lambda: _k(16, 1, 12),
    "K8_m1": lambda: _k(8, -1, 7), "K8_0": lambda: _k(8, 0, 7), "K8_p1": lambda: _k(8, 1, 7),
    "KNBR": _knbr,
    "R63": lambda: _r(63), "R64": lambda: _r(64),
    "H129_fffe": lambda: _h(0xFFFE), "H129_ffff": lambda: _h(M16),
    "C65535": lambda: _c(65535), "C65536": lambda: _c(65536),
    "U32_m2": lambda: _u(2 ** 32 - 2), "U32_m1": lambda: _u(2 ** 32 - 1),
    "CL30_m1": lambda: _cl(2 ** 30 - 1), "CL30_0": lambda: _cl(2 ** 30),
}

# name -> dict(V, bound = dist_bound, wmax = largest usable metric, root and
# far = the largest finite distance from it, nbrs = {root: distinct neighbours},
# leaves = names shard.leaf_set must make leaves, unreached = nodes the root
# does not reach)
STATED = {
    "P16": dict(V=22, wmax=0xFFFF, nbrs={}),
    "P17": dict(V=22, wmax=0x10000, nbrs={}),
    "K16_m1": dict(V=23, root="k0", far=0xFFFE, nbrs={"k0": 12}, unreached=2),
    "K16_0": dict(V=23, root="k0", far=0xFFFF, nbrs={"k0": 12}, unreached=2),
    "K16_p1": dict(V=23, root="k0", far=0x10000, nbrs={"k0": 12}, unreached=2),
    "K8_m1": dict(V=18, root="k0", far=0xFFFFFE, nbrs={"k0": 7}, unreached=2),
    "K8_0": dict(V=18, root="k0", far=0xFFFFFF, nbrs={"k0": 7}, unreached=2),
    "K8_p1": dict(V=18, root="k0", far=0x1000000, nbrs={"k0": 7}, unreached=2),
    "KNBR": dict(V=52, nbrs={"h08": 8, "h09": 9, "h16": 16, "h17": 17}),
    "R63": dict(V=28, wmax=63, nbrs={}),
    "R64": dict(V=29, wmax=64, nbrs={}),
    "H129_fffe": dict(V=140, wmax=0xFFFE, root="h0", nbrs={"h0": 129, "h1": 129}, unreached=5,
                      leaves=("s128",)),
    "H129_ffff": dict(V=140, wmax=0xFFFF, root="h0", nbrs={"h0": 129, "h1": 129}, unreached=5,
                      leaves=("s128",)),
    "C65535": dict(V=15, wmax=65535, leaves=("lf",), nbrs={"lf": 2}),
    "C65536": dict(V=15, wmax=65536, leaves=("lf",), nbrs={"lf": 2}),
    "U32_m2": dict(V=10, bound=2 ** 32 - 2, root="n0", far=2 ** 32 - 16 + 3, leaves=("lr",),
                   nbrs={"lr": 2, "n0": 2}, unreached=2),
    "U32_m1": dict(V=10, bound=2 ** 32 - 1, root="n0", far=2 ** 32 - 16 + 3, leaves=("lr",),
                   nbrs={"lr": 2, "n0": 2}, unreached=2),
    "CL30_m1": dict(bound=2 ** 30 - 1, nbrs={}),
    "CL30_0": dict(bound=2 ** 30, nbrs={}),
}


def dbs_of(name):
    made = BUILD[name]()
    return metric_graph(*made) if isinstance(made, tuple) else made


@functools.lru_cache(maxsize=None)
def shape(name):
    """stream, oracle, node names (id order), ids by name and CSR of a shape"""
    return make_shape(name, dbs_of(name))


@functools.lru_cache(maxsize=None)
def spf(name, root, use_link_metric=True):
    """the oracle's runSpf of one root name -> {node: (metric, next hops, ..)}"""
    return parse_spf_text(shape(name).oracle.spf_text(root, use_link_metric))


@functools.lru_cache(maxsize=None)
def expected(name, use_link_metric=True, roots=None):
    """Rows of `roots` (a tuple of ids; None = every node) by next-hop word
    count, as depth_ref.expected_rows. Shared by the tests: read only."""
    return expected_rows(shape(name), lambda r: spf(name, r, use_link_metric), roots)


@functools.lru_cache(maxsize=None)
def dist_rows(name, use_link_metric=True):
    """The oracle's dist rows of every root, node id order, [V, V] u32"""
    g = shape(name)
    out = np.zeros((g.V, g.V), np.uint32)
    for grp, dist, _ in expected(name, use_link_metric).values():
        out[grp] = dist
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def digests(name, use_link_metric=True, fast=False):
    """{reached, sumDist, digest} of every root, node id order, [V, 3] u64"""
    return oracle_digests(shape(name), use_link_metric, fast)
