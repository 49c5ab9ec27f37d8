"""Oracle-derived expectation for anycast route selection (shared by
test_gpu_select.py and test_host_select.py).

The expected metric / count / next-hop mask of every (root, prefix) come from
the CPU oracle's SPF results and the reference loop of
SpfSolver::getNextHopsWithMetric (openr/decision/SpfSolver.cpp:1043-1089)
restated in Python -- never from the engine's rows."""
import functools

import numpy as np

from graphs import drained_fabric, random_stream
from oracle import Oracle, parse_spf_text
from openr_amd.linkstate import root_neighbor_ids

INF = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def graph(kind, seed, n=70):
    """(stream, oracle) of a seeded test graph: 'unit' / 'weighted' are
    random_stream(seed, n) as test_gpu_sweep.py uses it, 'sparse-unit' /
    'sparse-weighted' the same generator at p = 0.05 (roots with unreached
    nodes), 'fabric' is drained_fabric(6, 4, seed)."""
    if kind == "fabric":
        st = drained_fabric(6, 4, seed=seed)
    else:
        kw = dict(p=0.05) if kind.startswith("sparse-") else {}
        st, _ = random_stream(seed, n=n, unit=kind.endswith("unit"), wmax=50, **kw)
    return st, Oracle(st)


@functools.lru_cache(maxsize=None)
def oracle_spf(kind, seed, n, names, use_link_metric):
    """{root name: {node: (metric, next-hop names, ...)}} for every name."""
    _, orc = graph(kind, seed, n)
    return {r: parse_spf_text(orc.spf_text(r, use_link_metric)) for r in names}


def unreached(spf, names):
    """{root name: names it does not reach} (roots reaching everything left out)"""
    out = {}
    for r in names:
        miss = [x for x in names if x not in spf[r]]
        if miss:
            out[r] = miss
    return out


def expect(spf, names, csr, table, W):
    """The reference loop for every root: table = list of announcer id lists.
    -> metric [V, P], count [V, P], nh [V, P, W] by node id; bit k of a mask
    = the root's k-th distinct neighbour in ascending id order."""
    V, P = len(names), len(table)
    ids = {nm: i for i, nm in enumerate(names)}
    metric = np.full((V, P), INF, np.uint32)
    count = np.zeros((V, P), np.uint32)
    nh = np.zeros((V, P, W), np.uint32)
    for r, rname in enumerate(names):
        res = spf[rname]
        nb = root_neighbor_ids(csr, r).tolist()
        bit = {v: k for k, v in enumerate(nb)}
        for p, ann in enumerate(table):
            shortest, min_cost = None, []
            for a in ann:
                ent = res.get(names[a])
                if ent is None:  # not in the SPF result: skipped (:1065-1068)
                    continue
                if shortest is None or ent[0] <= shortest:
                    if shortest is None or ent[0] < shortest:
                        shortest, min_cost = ent[0], []
                    min_cost.append(a)
            if shortest is None:
                continue
            metric[r, p] = shortest
            count[r, p] = len(min_cost)
            for a in min_cost:
                for hop in res[names[a]][1]:
                    k = bit[ids[hop]]
                    nh[r, p, k // 32] |= np.uint32(1 << (k % 32))
    return metric, count, nh


def csr_table(table):
    """list of id lists -> (offsets, nodes) of ospf_select_table"""
    off = np.zeros(len(table) + 1, np.uint32)
    off[1:] = np.cumsum([len(a) for a in table])
    nodes = np.array([x for a in table for x in a], np.uint32)
    return off, nodes


def random_table(V, rng, extra=()):
    """The random-graph table: an empty prefix, every single-node prefix,
    prefixes of 2, 3, 8, 9 and 63 / 64 / 65 announcers (both sides of the
    engine's lane-per-prefix threshold and of one wave's 64 announcers), all
    V nodes, then `extra`."""
    table = [[]] + [[v] for v in range(V)]
    for k in (2, 3, 8, 9, 63, 64, 65):
        table.append(sorted(rng.choice(V, size=k, replace=False).tolist()))
    table.append(list(range(V)))
    table.extend(sorted(a) for a in extra)
    return table


def fabric_table(names, rng):
    """The fabric table (topology.fabric names: spines 1-plane-i, fabric
    switches 2-pod-plane, racks 3-pod-i): every spine (more than 2 x 64
    announcers, many of them tight, with differing masks), each pod's fabric
    switches, 65 racks, and a rack together with its own pod's fabric switches
    (the root-is-announcer and the distance-1 cases)."""
    ids = {nm: i for i, nm in enumerate(names)}
    kind = lambda k: [i for i, nm in enumerate(names) if nm.startswith(k + "-")]  # noqa: E731
    spines, fsw, racks = kind("1"), kind("2"), kind("3")
    pods = sorted({names[i].split("-")[1] for i in fsw}, key=int)
    table = [spines]
    for d in pods:
        table.append([i for i in fsw if names[i].split("-")[1] == d])
    table.append(sorted(rng.choice(racks, size=65, replace=False).tolist()))
    rack = names[racks[len(racks) // 2]]
    table.append(sorted([ids[rack]] + [i for i in fsw if names[i].split("-")[1] == rack.split("-")[1]]))
    return table
