"""The level-byte kernels at their depth limits, against the CPU oracle.

Every unit-metric path keeps BFS levels in a byte. The derive sweep
(spf_levels.hip, spf_leaf.hip, spf_twin.hip, spf_msbfs.hip's nh_derive
kernels) stores dist + 1 with 0x7F = unreached / padding and is admitted for
a depth bound <= 123; the bound is even, so bound 122 and level byte 0x7B
are the deepest it ever sees (D122 / D122a: a 121-stage ladder of twins with
overloaded ends 122 hops apart, an overloaded hub of 3 or 5 next-hop words
whose neighbour rows hold the deepest bytes, and an island so that every
ladder root has 0x7F bytes beside deep ones). D124 is the same ladder seeded
one stage off centre: bound 124, refused. The bit-plane multi-source BFS
(variant 5) defers its rows through level bytes while the bound is <= 253:
M252 / M254 are 251-stage ladders on either side of that switch.

Expected dist rows, next-hop rows and digests are depth_ref.py's, from the
oracle's runSpf restatement; nothing is compared with another engine path.
test_host_depth_limits.py proves the shapes' bounds and distances."""
import numpy as np
import pytest
import torch

import depth_ref as D
from openr_amd.adjdb import AdjDbStream
from openr_amd.engine import Engine, EngineError, Sweep
from openr_amd.linkstate import LinkState, root_neighbor_ids
from oracle import Oracle

pytestmark = pytest.mark.gpu


def engine_for(name, weighted_seed=None):
    """An engine with the shape loaded; the oracle's bit order (ascending
    distinct neighbour ids) spot-checked against the engine's."""
    g = D.shape(name, weighted_seed)
    eng = Engine()
    eng.load(g.csr)
    assert eng.V == g.V
    for nm in ("e0", "e1", "z0a", g.names[0], g.names[g.V // 2]) + (("h",) if "h" in g.ids else ()):
        r = g.ids[nm]
        assert np.array_equal(eng.root_neighbors(r), root_neighbor_ids(g.csr, r)), nm
    return g, eng


def sweep_digests(sw):
    d = np.zeros((max(1, sw.n_roots), 3), np.uint64)
    sw._check(sw._L.ospf_sweep_digests_host(sw._h, d.ctypes.data))
    return dict(zip(sw.roots.tolist(), d[: sw.n_roots]))


def first_diff(g, grp, got, want):
    """(root, node, got, want) of the first differing row entry, for the message"""
    j, v = [int(x[0]) for x in np.nonzero(got != want)[:2]]
    return g.names[int(grp[j])], g.names[v], got[j, v].tolist(), want[j, v].tolist()


def check_rows(g, exp, rows_of_group, tag):
    """exp: depth_ref.expected(...); rows_of_group(grp, W) -> (dist, nh)"""
    for W, (grp, dist, nh) in exp.items():
        got_d, got_n = rows_of_group(grp, W)
        assert np.array_equal(got_d, dist), (tag, W, "dist") + first_diff(g, grp, got_d, dist)
        assert np.array_equal(got_n, nh), (tag, W, "nh") + first_diff(g, grp, got_n, nh)


def check_digests(g, got, want, tag):
    bad = [g.names[r] for r in range(g.V) if not np.array_equal(got[r], want[r])]
    assert not bad, (tag, len(bad), bad[:6])


def check_sweep(g, sw, exp, want_dig, tag):
    assert sorted(sw.roots.tolist()) == list(range(g.V))
    check_digests(g, sweep_digests(sw), want_dig, tag)
    check_rows(g, exp, sw.rows, tag)


def kernels_of(sw):
    return [(p["name"], p["kernel"], p["nh_words"]) for p in sw.profile(1)]


def assert_landmarks(name, exp):
    """The rows the limits are about, spelled out (they are part of what every
    configuration is compared with): the two overloaded ends 122 hops apart,
    i.e. level byte 0x7B, over two ECMP next hops; the hub's W-word row."""
    g = D.shape(name)
    S, hub = D.SHAPES[name]["S"], D.SHAPES[name]["hub"]
    W_hub = D.STATED[name][3]
    grp, dist, nh = exp[1]
    e0, e1 = g.ids["e0"], g.ids["e1"]
    j0, j1 = int(np.searchsorted(grp, e0)), int(np.searchsorted(grp, e1))
    assert dist[j0, e1] == dist[j1, e0] == S + 1 == 122 == 0x7B - 1
    assert nh[j0, e1, 0] == nh[j1, e0, 0] == 0b11
    assert (dist[j0] == D.INF).sum() == sum(D.SHAPES[name]["islands"])  # the island
    grp, dist, nh = exp[W_hub]
    assert grp.tolist() == [g.ids["h"]]
    assert dist[0, e1] == S - hub + 2 and (dist[0] == 1).sum() == 2 * hub
    far = np.zeros(W_hub, np.uint32)  # through both nodes of the hub's last stage
    for nm in g.names:
        if nm[1:4] == f"{hub - 1:03d}":
            k = root_neighbor_ids(g.csr, g.ids["h"]).tolist().index(g.ids[nm])
            far[k // 32] |= np.uint32(1 << (k % 32))
    assert np.array_equal(nh[0, e1], far) and far[W_hub - 1] != 0


# ------------------------------------------------- a. derive sweep at the limit
CONFIGS = {
    "plain": ({}, True),
    "twin": ({"OSPF_SWEEP_TWIN": "1"}, True),
    "twinlv": ({"OSPF_SWEEP_TWINLV": "1"}, True),
    "notwinlv": ({"OSPF_SWEEP_NOTWINLV": "1"}, True),
    "wide1": ({"OSPF_DERIVE_WIDE1": "1"}, True),
    "eager": ({}, False),
}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["D122", "D122a"])
def test_derive_sweep_at_the_limit(name, config, monkeypatch):
    """Bound 122 is admitted; every root's dist row, next-hop row and digest
    == the oracle's, with the twin next-hop kernel forced, twin levels forced
    and off, nh_derive_wide_kernel in place of the planned wide kernel, and
    without the captured graph."""
    env, hip_graph = CONFIGS[config]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    exp, want_dig = D.expected(name), D.digests(name)
    assert_landmarks(name, exp)
    g, eng = engine_for(name)
    try:
        sw = Sweep(eng, mode="derive", hip_graph=hip_graph)
        try:
            assert sw.mode == "derive" and sw.hip_graph == hip_graph
            assert sw.max_nh_words == D.STATED[name][3]
            sw.run()
            eng.sync()
            check_sweep(g, sw, exp, want_dig, (name, config))
            units = kernels_of(sw)
            kern = " ".join(k for _, k, _ in units)
            assert any(n == "levels" for n, _, _ in units), units
            twin_lv = any(n.startswith("twin_levels") for n, _, _ in units)
            if config == "twin":
                assert "nh_twin4_kernel" in kern, units
            if config == "twinlv":
                assert twin_lv and "twin_levels_kernel" in kern, units
            if config == "notwinlv":
                assert not twin_lv, units
            wide = [k for _, k, w in units if w == D.STATED[name][3]]
            assert wide, units
            if name == "D122":  # 3 words: the 16-node-tile kernel (no twin class of 38 slots)
                assert any("nh_derive16_kernel" in k or "nh_twin4_kernel" in k for k in wide), wide
            elif config == "wide1":
                assert any("nh_derive_wide_kernel" in k for k in wide), wide
        finally:
            sw.close()
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["D122", "D122a"])
def test_derive_sweep_replay_reaches_the_last_level(name):
    """The captured graph holds the seed BFS at the depth the eager run
    reached: two replays, digests poisoned in between, both == the oracle
    down to the deepest level."""
    exp, want_dig = D.expected(name), D.digests(name)
    g, eng = engine_for(name)
    try:
        sw = Sweep(eng, mode="derive", hip_graph=True)
        try:
            assert sw.hip_graph
            for rep in range(2):
                sw.poison()
                sw.run()
                eng.sync()
                check_sweep(g, sw, exp, want_dig, (name, "replay", rep))
        finally:
            sw.close()
    finally:
        eng.close()


# ------------------------------------------------------- b. the derive ABI pair
def derive_abi(g, eng, hop=False):
    """ospf_levels_dev + ospf_nh_derive_dev for every root -> level rows
    [V, pitch] u8, dist [V, V], {W: (grp, nh, digest)}"""
    dev = torch.device("cuda", 0)
    V, pitch = g.V, eng.lev_pitch
    ids = np.arange(V, dtype=np.uint32)
    d_all = torch.from_numpy(ids.view(np.int32)).to(dev)
    lev = torch.zeros((V, pitch), dtype=torch.uint8, device=dev)  # padding is the kernel's to write
    dist = torch.empty((V, V), dtype=torch.int32, device=dev)
    ldg = torch.empty((V, 3), dtype=torch.int64, device=dev)
    eng.levels_dev(d_all.data_ptr(), V, lev.data_ptr(), d_dist=dist.data_ptr(),
                   d_lev_digest=ldg.data_ptr(), hop_count=hop)
    words = np.array([D.words_of(g.csr, int(r)) for r in ids])
    out = {}
    for W in sorted(set(words.tolist())):
        grp = ids[words == W]
        d_r = torch.from_numpy(grp.view(np.int32)).to(dev)
        nh = torch.empty((grp.size, V, W), dtype=torch.int32, device=dev)
        dg = torch.empty((grp.size, 3), dtype=torch.int64, device=dev)
        eng.nh_derive_dev(d_r.data_ptr(), grp.size, W, lev.data_ptr(), d_all.data_ptr(),
                          nh.data_ptr(), d_lev_digest=ldg.data_ptr(), d_digest=dg.data_ptr())
        eng.sync()
        out[W] = (grp, nh.cpu().numpy().view(np.uint32), dg.cpu().numpy().view(np.uint64))
    eng.sync()
    return lev.cpu().numpy(), dist.cpu().numpy().view(np.uint32), out


@pytest.mark.parametrize("ctiles", [None, "1"])
@pytest.mark.parametrize("name", ["D122", "D122a"])
def test_derive_abi_pair_at_the_limit(name, ctiles, monkeypatch):
    """Level rows: byte = dist + 1 where the oracle has an entry, 0x7F exactly
    where it has none and in the row padding, 0x7B the largest below 0x7F;
    next-hop rows (nh_derive16_kernel at 1 and 3 words, nh_derive_wide_kernel
    at D122a's 5) and digests == the oracle's."""
    if ctiles:
        monkeypatch.setenv("OSPF_DERIVE_CTILES", ctiles)
    exp, want_dig = D.expected(name), D.digests(name)
    g, eng = engine_for(name)
    try:
        lev, dist, out = derive_abi(g, eng)
    finally:
        eng.close()
    want_d = np.zeros((g.V, g.V), np.uint32)
    for W, (grp, d, _) in exp.items():
        want_d[grp] = d
    want_lev = np.full(lev.shape, 0x7F, np.uint8)
    want_lev[:, : g.V] = np.where(want_d == D.INF, 0x7F, want_d + 1).astype(np.uint8)
    assert int(want_lev[want_lev != 0x7F].max()) == 0x7B  # (what the shape is for)
    assert np.array_equal(lev[:, g.V:], want_lev[:, g.V:]), "row padding"
    assert np.array_equal(lev == 0x7F, want_lev == 0x7F), first_diff(g, np.arange(g.V), lev, want_lev)
    assert np.array_equal(lev, want_lev), first_diff(g, np.arange(g.V), lev, want_lev)
    assert int(lev[lev != 0x7F].max()) == 0x7B
    assert np.array_equal(dist, want_d), first_diff(g, np.arange(g.V), dist, want_d)
    got_dig = {}
    for W, (grp, nh, dg) in out.items():
        assert np.array_equal(grp, exp[W][0])
        assert np.array_equal(nh, exp[W][2]), (W,) + first_diff(g, grp, nh, exp[W][2])
        got_dig.update(zip(grp.tolist(), dg))
    check_digests(g, got_dig, want_dig, (name, ctiles))


# ------------------------------------------------ c. refusal just past the limit
def test_bound_124_is_refused_and_auto_steps_aside(monkeypatch):
    """D124 (bound 124, the same ladder and distances): the derive sweep and
    ospf_levels_dev refuse it with OSPF_E_RANGE; without the LDS sweep AUTO
    takes derive on D122 and another path on D124, both == the oracle."""
    g, eng = engine_for("D124")
    try:
        with pytest.raises(EngineError) as ei:
            Sweep(eng, mode="derive")
        assert ei.value.code == -4, ei.value
        dev = torch.device("cuda", 0)
        d_all = torch.arange(g.V, dtype=torch.int32, device=dev)
        lev = torch.empty((g.V, eng.lev_pitch), dtype=torch.uint8, device=dev)
        with pytest.raises(EngineError) as ei:
            eng.levels_dev(d_all.data_ptr(), g.V, lev.data_ptr())
        assert ei.value.code == -4, ei.value
    finally:
        eng.close()
    monkeypatch.setenv("OSPF_SWEEP_NOLDS", "1")
    for name in ("D122", "D124"):
        g, eng = engine_for(name)
        try:
            sw = Sweep(eng)
            try:
                assert (sw.mode == "derive") == (name == "D122"), (name, sw.mode)
                sw.run()
                eng.sync()
                check_sweep(g, sw, D.expected(name), D.digests(name), (name, "auto", sw.mode))
            finally:
                sw.close()
        finally:
            eng.close()


# ------------------------------------------------------------ d. hop-count mode
@pytest.mark.parametrize("name", ["D122", "D122a"])
def test_derive_hop_count_at_the_limit(name):
    """Random metrics 1..30 on the same links: the derive sweep in hop-count
    mode == the oracle's runSpf(root, useLinkMetric = false)."""
    exp, want_dig = D.expected(name, False, 5), D.digests(name, False, 5)
    g, eng = engine_for(name, 5)
    try:
        assert eng.info().unit_metric == 0
        with pytest.raises(EngineError):
            Sweep(eng, mode="derive")  # link metrics: not the derive sweep's
        sw = Sweep(eng, mode="derive", hop_count=True)
        try:
            sw.run()
            eng.sync()
            check_sweep(g, sw, exp, want_dig, (name, "hop"))
        finally:
            sw.close()
    finally:
        eng.close()


# ------------------------------- e. LDS sweep and per-root BFS variants at depth
def test_lds_sweep_at_depth_122():
    g, eng = engine_for("D122")
    try:
        sw = Sweep(eng, mode="lds")
        try:
            sw.run()
            eng.sync()
            check_sweep(g, sw, D.expected("D122"), D.digests("D122"), "lds")
        finally:
            sw.close()
    finally:
        eng.close()


def test_lds_sweep_at_depth_252():
    """u16 levels and a u16 queue per wave, 252 levels deep: every root's
    digest, the named roots' rows."""
    g, eng = engine_for("M252")
    try:
        sw = Sweep(eng, mode="lds")
        try:
            sw.run()
            eng.sync()
            check_digests(g, sweep_digests(sw), D.digests("M252"), "lds")
            check_rows(g, D.expected("M252", roots=D.sample_roots("M252")), sw.rows, "lds")
        finally:
            sw.close()
    finally:
        eng.close()


def run_batch(g, eng, variant, must_run=True):
    """eng.run of every root by word class under a forced variant ->
    rows_of_group for check_rows, digests by root, the W classes the forced
    variant took (the planner keeps its own choice where it does not fit)."""
    rows, dig, took = {}, {}, []
    for W in sorted({D.words_of(g.csr, r) for r in range(g.V)}):
        grp = np.array([r for r in range(g.V) if D.words_of(g.csr, r) == W], np.uint32)
        if eng.plan(W, n_roots=grp.size)["variant"] != variant:
            assert not must_run, (variant, W, eng.plan(W, n_roots=grp.size))
            continue
        took.append(W)
        out = eng.run(grp, W, want_digest=True)
        rows[W] = (out["dist"], out["nh"])
        dig.update(zip(grp.tolist(), out["digest"]))
    return rows, dig, took


@pytest.mark.parametrize("variant", [4, 3])
def test_per_root_bfs_variants_at_depth_122(variant, monkeypatch):
    """Variants 4 and 3 (a workgroup per root, LDS bitmaps): every root of
    D122 == the oracle. Variant 4 must take every word class; variant 3 runs
    where the planner admits it."""
    monkeypatch.setenv("OSPF_FORCE_VARIANT", str(variant))
    exp, want_dig = D.expected("D122"), D.digests("D122")
    g, eng = engine_for("D122")
    try:
        rows, dig, took = run_batch(g, eng, variant, must_run=variant == 4)
    finally:
        eng.close()
    assert 1 in took, took
    check_rows(g, {W: exp[W] for W in took}, lambda grp, W: rows[W], variant)
    bad = [g.names[r] for r in dig if not np.array_equal(dig[r], want_dig[r])]
    assert not bad, bad[:6]


# ------------------------------- f. bit-plane BFS on both sides of the defer switch
@pytest.mark.parametrize("name,nodefer", [("M252", False), ("M252", True), ("M254", False)])
def test_msbfs_both_sides_of_the_defer_switch(name, nodefer, monkeypatch):
    """Variant 5 over all 506 roots (eight 64-root batches, the last ragged):
    M252 defers its rows through level bytes (the check level past the bound
    is byte 254), M254 writes them per level, and so does M252 with
    OSPF_MS_NODEFER: every digest and the named roots' rows == the oracle."""
    monkeypatch.setenv("OSPF_FORCE_VARIANT", "5")
    if nodefer:
        monkeypatch.setenv("OSPF_MS_NODEFER", "1")
    want_dig = D.digests(name)
    exp = D.expected(name, roots=D.sample_roots(name))
    assert list(exp) == [1] and exp[1][0].size >= 32
    g, eng = engine_for(name)
    try:
        roots = np.arange(g.V, dtype=np.uint32)
        assert eng.plan(1, n_roots=g.V)["variant"] == 5
        out = eng.run(roots, 1, want_digest=True)
    finally:
        eng.close()
    check_digests(g, out["digest"], want_dig, (name, nodefer))
    check_rows(g, exp, lambda grp, W: (out["dist"][grp], out["nh"][grp]), (name, nodefer))
    e0, e1 = g.ids["e0"], g.ids["e1"]
    assert out["dist"][e0, e1] == out["dist"][e1, e0] == 252


# ------------------------------------------------------------ g. LinkState level
@pytest.mark.parametrize("incremental", [False, True])
def test_linkstate_derive_sweep_then_seed_overloaded(incremental, monkeypatch):
    """odl::LinkState's all-sources prefetch on D122 without the LDS sweep
    takes the derive sweep; overloading the seed node moves the transit seed
    to stage 0 (bound >= 124: no derive sweep any more). getSpfResult of every
    root == the oracle's after each step."""
    from graphs import depth_bound
    monkeypatch.setenv("OSPF_SWEEP_NOLDS", "1")
    dbs = D.ladder_dbs("D122")
    st = AdjDbStream.from_dbs(dbs)
    o, p = Oracle(), LinkState()
    assert o.apply(st) == p.apply(st)
    p.set_incremental(incremental)
    names = p.node_names()

    def check(step):
        p.prefetch_all()
        for r in names:
            assert p.spf_text(r) == o.spf_text(r), (step, r)
        return p.sweep_stats()

    assert depth_bound(p.csr()) == 122
    stats = check("load")
    assert stats["sweeps"] == 1 and stats["mode"] == "derive", stats
    seed = next(d for d in dbs if d.name == "a060")
    seed.overloaded = True
    upd = AdjDbStream.from_dbs([seed])
    assert o.apply(upd) == p.apply(upd)
    assert depth_bound(p.csr()) == 242 >= 124
    stats = check("seed overloaded")
    assert stats["sweeps"] == 2 and stats["mode"] != "derive", stats
    seed.overloaded = False
    upd = AdjDbStream.from_dbs([seed])
    assert o.apply(upd) == p.apply(upd)
    assert depth_bound(p.csr()) == 122
    stats = check("seed back")
    assert stats["sweeps"] == 3 and stats["mode"] == "derive", stats
