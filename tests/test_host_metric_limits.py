"""The shapes of metric_ref.py are what test_gpu_metric_limits.py says they
are (checked on the host against the oracle and the CSR, never the engine, so
the GPU tests cannot be vacuous): the engine's distance bound restated over
the CSR, the largest usable metric, the largest finite distance from the
named root and that it occurs, the named roots' distinct-neighbour and word
counts, the leaves shard.leaf_set picks, the unreached nodes, and for U32_m2
that the term a plain u32 add would wrap really passes 2^32 while the true
distance does not."""
import numpy as np
import pytest

import metric_ref as M
from graphs import dist_bound, metric_graph
from openr_amd import shard
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState, root_neighbor_ids

SMALL = [n for n in M.BUILD if not n.startswith("CL30")]


def usable_max(csr):
    return int(csr["metric"][csr["edge_up"] != 0].max())


def metric_of(g, a, b):
    """the usable metrics a -> b (one per parallel adjacency)"""
    rp, col, met, up = (g.csr[k] for k in ("row_ptr", "col", "metric", "edge_up"))
    u = g.ids[a]
    return [int(met[e]) for e in range(int(rp[u]), int(rp[u + 1])) if col[e] == g.ids[b] and up[e]]


@pytest.mark.parametrize("name", SMALL)
def test_shape_is_what_it_claims(name):
    st, g = M.STATED[name], M.shape(name)
    assert g.V == st["V"]
    if "bound" in st:
        assert dist_bound(g.csr) == st["bound"]
    if "wmax" in st:
        assert usable_max(g.csr) == st["wmax"]
    for r, n in st["nbrs"].items():
        assert root_neighbor_ids(g.csr, g.ids[r]).size == n, r
        assert M.words_of(g.csr, g.ids[r]) == max(1, (n + 31) // 32), r
    if "root" in st:
        res = M.spf(name, st["root"])
        assert g.V - len(res) == st["unreached"]
        assert not any(nm.startswith("z") for nm in res)
        if "far" in st:
            assert max(e[0] for e in res.values()) == st["far"]
    leaf = shard.leaf_set(g.csr["row_ptr"], g.csr["col"])
    for nm in st.get("leaves", ()):
        assert leaf[g.ids[nm]], nm
    # the furniture: a two-way ECMP diamond, a no-transit node that is still
    # a destination, a down link, an island
    at = next(a for a in g.names if metric_of(g, a, "fa") and a not in ("fb", "fc", "fo"))
    assert M.spf(name, at)["fc"][0] == 3 and set(M.spf(name, at)["fc"][1]) == {"fa", "fb"}
    assert g.csr["no_transit"][g.ids["fo"]] == 1 and "fo" in M.spf(name, at)
    assert M.spf(name, "fo")["fa"][0] == 2 and not metric_of(g, "fa", "fb")
    assert g.ids["fb"] in root_neighbor_ids(g.csr, g.ids["fa"])  # down: still a next-hop bit
    assert set(M.spf(name, "za")) == {nm for nm in g.names if nm.startswith("z")}


def test_dist_bound_restatement_small_cases():
    """Every node adds its largest usable out-metric: an overloaded node
    counts, a down link counts for neither end, parallel links once."""
    def bound(links, ov=()):
        return dist_bound(LinkState(stream=AdjDbStream.from_dbs(metric_graph(links, ov))).csr())

    assert bound([("a", "b", 5, 7)]) == 12
    assert bound([("a", "b", 5, 7), ("a", "b", 9, 1)]) == 16
    assert bound([("a", "b", 5, 7), ("b", "c", 100, 3)]) == 5 + 100 + 3
    assert bound([("a", "b", 5, 7), ("b", "c", 100, 3)], {"b"}) == 5 + 100 + 3
    assert bound([("a", "b", 5, 7), ("b", "c", 100, 3, "down")]) == 12
    assert bound([("a", "b", 5, 7), ("c", "b", 3, 100, "down")]) == 12


def test_p16_p17_differ_in_one_direction_of_one_adjacency():
    a, b = M.shape("P16"), M.shape("P17")
    for k in ("row_ptr", "col", "link_id", "edge_up", "no_transit"):
        assert np.array_equal(a.csr[k], b.csr[k]), k
    diff = np.flatnonzero(a.csr["metric"] != b.csr["metric"])
    assert diff.size == 1
    assert (int(a.csr["metric"][diff[0]]), int(b.csr["metric"][diff[0]])) == (0xFFFF, 0x10000)
    assert metric_of(b, "p03", "p04") == [0x10000] and metric_of(b, "p04", "p03") == [0xFFFF]
    assert set(np.unique(a.csr["metric"]).tolist()) >= {1, 2, 0xFFFE, 0xFFFF}
    # the adjacency carries shortest paths in both states
    assert M.spf("P16", "p03")["p04"][0] == 0xFFFF and M.spf("P17", "p03")["p04"][0] == 0x10000
    assert M.STATED["P16"]["V"] % 4 != 0


@pytest.mark.parametrize("K,name", [(16, "K16"), (8, "K8")])
def test_k_shapes_straddle_the_distance_field(K, name):
    """infk - 1, infk, infk + 1 from k0, reached over the ECMP diamond at the
    far end of a 4-link chain; k0's neighbour count picks K."""
    infk = 0xFFFFFFFF >> K
    for sfx, off in (("m1", -1), ("0", 0), ("p1", 1)):
        nm = f"{name}_{sfx}"
        res = M.spf(nm, "k0")
        assert res["e3"][0] == infk + off == M.STATED[nm]["far"]
        assert sorted(d for d, *_ in res.values())[-2] == infk + off - 1  # e2, one short of e3
        n = M.STATED[nm]["nbrs"]["k0"]
        assert int(shard.neighbor_caps(np.array([n]))[0]) == K
        assert M.spf(nm, "c4")["e3"][0] == 3 and res["e3"][1] == ("c1",)
        assert M.shape(nm).V % 4 != 0


def test_knbr_hubs_cross_the_class_boundaries():
    g = M.shape("KNBR")
    caps = {h: int(shard.neighbor_caps(np.array([n]))[0]) for h, n in M.STATED["KNBR"]["nbrs"].items()}
    assert caps == {"h08": 8, "h09": 16, "h16": 16, "h17": 32}
    far = {h: max(e[0] for e in M.spf("KNBR", h).values()) for h in caps}
    assert far["h16"] < 0xFFFF < far["h09"], far  # K = 16 runs that fit and that do not
    assert g.V % 4 == 0


@pytest.mark.parametrize("name,top", [("R63", 63), ("R64", 64)])
def test_ring_shapes_relax_across_the_whole_ring(name, top):
    g = M.shape(name)
    out = sorted(metric_of(g, "r05", b)[0] for b in ("r04", "r06", "r16"))
    assert out == [1, 1, top]
    assert M.spf(name, "r05")["r06"][0] <= top
    assert (g.V % 4 != 0) == (name == "R64")  # both store paths of the ring Dial


@pytest.mark.parametrize("name,top", [("H129_fffe", 0xFFFE), ("H129_ffff", 0xFFFF)])
def test_hub_shapes(name, top):
    g = M.shape(name)
    h0, h1 = g.ids["h0"], g.ids["h1"]
    assert h1 == h0 + 1  # consecutive roots: a run for the shared slot rows
    assert np.array_equal(root_neighbor_ids(g.csr, h0), root_neighbor_ids(g.csr, h1))
    rp, met, up = g.csr["row_ptr"], g.csr["metric"], g.csr["edge_up"]
    own = [int(met[e]) for e in range(int(rp[h0]), int(rp[h0 + 1])) if up[e]]
    assert max(own) == top == usable_max(g.csr)
    assert len(own) == 128  # h0 - s020 is down, still one of the 129 slots
    res = M.spf(name, "h0")
    assert res["s128"][0] == top and res["s128"][1] == ("s128",)  # bit 128: word 4
    assert root_neighbor_ids(g.csr, h0).tolist().index(g.ids["s128"]) == 128
    assert sum(len(e[1]) > 1 for e in res.values()) >= 20  # real ECMP from the hub
    assert g.csr["no_transit"][g.ids["s010"]] == 1 and "s010" in res["s010"][1]
    assert [metric_of(g, "h0", f"s{i:03d}") != metric_of(g, "h1", f"s{i:03d}") for i in (0, 1, 2)] == [True] * 3
    assert g.V % 4 == 0


@pytest.mark.parametrize("name,inlink", [("C65535", 65535), ("C65536", 65536)])
def test_cover_shapes(name, inlink):
    g = M.shape(name)
    assert metric_of(g, "c01", "lf") == [inlink] and metric_of(g, "lf", "c01") == [3]
    leaf = shard.leaf_set(g.csr["row_ptr"], g.csr["col"])
    others = [int(g.csr["metric"][g.csr["twin"][e]]) for v in np.flatnonzero(leaf)
              for e in range(int(g.csr["row_ptr"][v]), int(g.csr["row_ptr"][v + 1]))
              if g.names[v] != "lf"]
    assert max(others, default=0) <= 0xFFFF  # lf's in-link alone decides
    res = M.spf(name, "c01")["lf"]
    if inlink == 65535:  # on shortest paths: the direct link ties with c02's
        assert res[0] == 65535 and set(res[1]) == {"lf", "c02"}
    else:
        assert res[0] == 65535 and res[1] == ("c02",)


def test_u32_shapes():
    for name in ("U32_m2", "U32_m1"):
        g = M.shape(name)
        assert dist_bound(g.csr) == M.STATED[name]["bound"]
        assert root_neighbor_ids(g.csr, g.ids["n0"]).tolist() == sorted([g.ids["fo"], g.ids["lr"]])
    g = M.shape("U32_m2")
    w = metric_of(g, "lr", "n0")[0]
    d_n0 = M.spf("U32_m2", "n0")
    assert w + d_n0["n1"][0] >= 2 ** 32  # the term a plain u32 add wraps
    assert (w + d_n0["n1"][0]) % 2 ** 32 < M.spf("U32_m2", "lr")["n1"][0]  # and it would win
    assert M.spf("U32_m2", "lr")["n1"][0] == metric_of(g, "lr", "n1")[0] < 2 ** 31
    assert d_n0["x"][0] == 2 ** 32 - 16
    far = max(max(e[0] for e in M.spf("U32_m2", r).values()) for r in g.names)
    assert 2 ** 32 - 16 <= far < M.STATED["U32_m2"]["bound"]


def test_closure_fabric_bounds():
    for name in ("CL30_m1", "CL30_0"):
        g = M.shape(name)
        assert dist_bound(g.csr) == M.STATED[name]["bound"]
        leaf = shard.leaf_set(g.csr["row_ptr"], g.csr["col"])
        assert leaf[g.ids["3-7-5"]]
        twin_in = [int(g.csr["metric"][g.csr["twin"][e]]) for v in np.flatnonzero(leaf)
                   for e in range(int(g.csr["row_ptr"][v]), int(g.csr["row_ptr"][v + 1]))]
        assert max(twin_in) <= 0xFFFF
