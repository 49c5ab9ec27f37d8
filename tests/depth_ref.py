"""Deep ladders at the level-byte limits and their oracle-derived expectation
(shared by test_host_depth_limits.py and test_gpu_depth_limits.py).

The engine stores BFS levels in a byte on every unit-metric path: dist + 1
with 0x7F = unreached in the derive sweep (admitted for a depth bound <= 123;
the bound 2 * ecc + 2 is even, so 122 and level byte 0x7B are the largest that
occur), and per-(node, root) bytes in the bit-plane multi-source BFS while the
bound is <= 253. The shapes below sit on and just past those limits; dist
rows, next-hop rows and digests come from the CPU oracle's runSpf
restatement -- never from the engine's rows."""
import functools
from types import SimpleNamespace

import numpy as np

from graphs import deep_ladder
from oracle import Oracle, parse_spf_text
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState, root_neighbor_ids

INF = 0xFFFFFFFF

# deep_ladder arguments; D122a's 3-node island brings V to a multiple of 4
# (vector stores, 128-byte aligned sweep rows; 247 takes the packed pitch)
SHAPES = {
    "D122": dict(S=121, seed_stage=60, ends=True, hub=38, islands=(2,)),
    "D122a": dict(S=121, seed_stage=60, ends=True, hub=70, islands=(3,)),
    "D124": dict(S=121, seed_stage=61, ends=True, hub=38, islands=(2,)),
    "M252": dict(S=251, seed_stage=125, ends=True, islands=(2,)),
    "M254": dict(S=251, seed_stage=126, ends=True, islands=(2,)),
}
# name -> (depth bound, largest finite distance, V, next-hop words of the hub)
STATED = {
    "D122": (122, 122, 247, 3),
    "D122a": (122, 122, 248, 5),
    "D124": (124, 122, 247, 3),
    "M252": (252, 252, 506, None),
    "M254": (254, 252, 506, None),
}


def ladder_dbs(name, weighted_seed=None):
    return deep_ladder(weighted_seed=weighted_seed, **SHAPES[name])


def make_shape(name, dbs):
    """stream, oracle, node names (id order), ids by name and read-only CSR of
    a list of AdjDbs (the one definition metric_ref.py shares)"""
    st = AdjDbStream.from_dbs(dbs)
    ls = LinkState(stream=st)
    names = ls.node_names()
    csr = ls.csr()
    for a in csr.values():
        a.setflags(write=False)
    return SimpleNamespace(name=name, stream=st, oracle=Oracle(st), names=names,
                           ids={nm: i for i, nm in enumerate(names)}, csr=csr, V=len(names))


@functools.lru_cache(maxsize=None)
def shape(name, weighted_seed=None):
    """stream, oracle, node names (id order), ids by name and CSR of a shape"""
    return make_shape(name, ladder_dbs(name, weighted_seed))


def words_of(csr, r):
    return max(1, (root_neighbor_ids(csr, r).size + 31) // 32)


@functools.lru_cache(maxsize=None)
def spf(name, root, use_link_metric=True, weighted_seed=None):
    """the oracle's runSpf of one root name -> {node: (metric, next hops, ..)}"""
    return parse_spf_text(shape(name, weighted_seed).oracle.spf_text(root, use_link_metric))


def rows_of(g, res, r, W):
    """One oracle result as the engine's rows of root id r: dist [V] u32
    (0xFFFFFFFF where the oracle has no entry), nh [V, W] u32 (bit k = the
    root's k-th distinct neighbour in ascending id order)."""
    dist = np.full(g.V, INF, np.uint32)
    nh = np.zeros((g.V, W), np.uint32)
    bit = {int(v): k for k, v in enumerate(root_neighbor_ids(g.csr, r).tolist())}
    for nm, ent in res.items():
        v = g.ids[nm]
        dist[v] = ent[0]
        for hop in ent[1]:
            k = bit[g.ids[hop]]
            nh[v, k // 32] |= np.uint32(1 << (k % 32))
    return dist, nh


def expected_rows(g, spf_of, roots=None):
    """Rows of `roots` (ids; None = every node) of shape g by next-hop word
    count, spf_of(root name) -> the oracle's parsed runSpf:
    {W: (root ids [n] u32 ascending, dist [n, V] u32, nh [n, V, W] u32)},
    read only."""
    rs = np.arange(g.V, dtype=np.uint32) if roots is None else np.array(sorted(roots), np.uint32)
    words = np.array([words_of(g.csr, int(r)) for r in rs])
    out = {}
    for W in sorted(set(words.tolist())):
        grp = rs[words == W]
        dist = np.zeros((grp.size, g.V), np.uint32)
        nh = np.zeros((grp.size, g.V, W), np.uint32)
        for j, r in enumerate(grp.tolist()):
            dist[j], nh[j] = rows_of(g, spf_of(g.names[r]), r, W)
        for a in (grp, dist, nh):
            a.setflags(write=False)
        out[W] = (grp, dist, nh)
    return out


def oracle_digests(g, use_link_metric=True, fast=False):
    """{reached, sumDist, digest} of every root of shape g, node id order,
    [V, 3] u64, read only (fast: the oracle's CSR-Dijkstra restatement)"""
    f = g.oracle.fast_digests if fast else g.oracle.digests
    d = f(g.names, use_link_metric, threads=8)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(name, use_link_metric=True, weighted_seed=None, roots=None):
    """Rows of `roots` (a tuple of ids; None = every node) by next-hop word
    count: {W: (root ids [n] u32 ascending, dist [n, V] u32, nh [n, V, W]
    u32)}. Shared by the tests: read only."""
    return expected_rows(shape(name, weighted_seed),
                         lambda r: spf(name, r, use_link_metric, weighted_seed), roots)


@functools.lru_cache(maxsize=None)
def digests(name, use_link_metric=True, weighted_seed=None):
    """{reached, sumDist, digest} of every root, node id order, [V, 3] u64"""
    return oracle_digests(shape(name, weighted_seed), use_link_metric)


def sample_roots(name):
    """The named roots of a 251-stage shape whose rows are compared: both
    ends, both nodes of stages 0, 1, 125, 249 and 250, the seed, an island
    node and a stride through the rest (at least 32 in all)."""
    g = shape(name)
    S = SHAPES[name]["S"]
    seed = f"a{SHAPES[name]['seed_stage']:03d}"
    pick = ["e0", "e1", seed, "z0a"]
    for i in (0, 1, 125, S - 2, S - 1):
        pick += [nm for nm in g.names if nm[1:4] == f"{i:03d}" and nm[0] in "as"]
    pick += g.names[5::23]
    out = sorted({g.ids[nm] for nm in pick})
    assert len(out) >= 32
    return tuple(out)
