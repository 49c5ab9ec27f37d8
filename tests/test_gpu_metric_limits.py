"""The weighted kernels at their metric and distance limits, against the CPU
oracle.

  L1  packed {colx, w | rw << 16} entries: every metric <= 0xFFFF (P16), one
      of 0x10000 (P17), and the patch from one to the other and back;
  L2  the bucketed Dial's packed state: the largest distance at infk - 1,
      infk, infk + 1 for K = 16 and K = 8, roots of 8 / 9 / 16 / 17 neighbours;
  L3  the ring Dial: largest metric 63 (admitted) and 64;
  L4  the lane derive's u16 slot table: a 129-neighbour hub whose largest
      metric is 0xFFFE (admitted) and 0xFFFF (refused when the sweep is
      created, AUTO steps aside);
  L5  the cover graph's 16-bit leaf in-link metric: 65535 and 65536;
  L6  the closure over the cover: distance bound 2^30 - 1 and 2^30;
  L7  the u32 range: distance bound 2^32 - 2 (distances up to 2^32 - 13, a
      derive term that passes 2^32) and 2^32 - 1 (refused).

Expected dist rows, next-hop rows and digests are metric_ref.py's, from the
oracle's runSpf restatement; nothing is compared with another engine path.
test_host_metric_limits.py proves the shapes sit where this file says. The
per-root batches pass the roots' neighbour class as max_root_neighbors (as
the sweeps and odl::LinkState do): without it the Dial never packs."""
import numpy as np
import pytest
import torch

import metric_ref as M
from openr_amd import _native as N
from openr_amd import shard
from openr_amd.engine import Engine, EngineError, Sweep
from openr_amd.linkstate import LinkState, LinkStateError, root_neighbor_ids
from test_gpu_depth_limits import check_digests, check_rows, check_sweep, first_diff, sweep_digests
from test_gpu_wderive import cover_pipeline

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
WD_KNOBS = {
    "default": {},
    "tagged": {"OSPF_WD_DELTA": "3"},
    "unpacked": {"OSPF_WD_PACK": "0"},
    "pack16": {"OSPF_WD_PACK": "16"},
}


def engine_for(name, csr=None):
    g = M.shape(name)
    eng = Engine()
    eng.load({k: v.copy() for k, v in (csr or g.csr).items()})
    assert eng.V == g.V
    for r in (0, g.V // 2, g.V - 1):
        assert np.array_equal(eng.root_neighbors(r), root_neighbor_ids(g.csr, r))
    return g, eng


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def run_classes(g, eng, hop=False):
    """Every root through ospf_run_batch_dev, one batch per neighbour class
    (8, 16, 32 x words) with the class as max_root_neighbors -> rows_of_group
    for check_rows, digests [V, 3]."""
    nb = shard.distinct_neighbors(g.csr["row_ptr"], g.csr["col"])
    caps = shard.neighbor_caps(nb)
    flags = N.OSPF_WANT_DIST | N.OSPF_WANT_NH | N.OSPF_WANT_DIGEST | (N.OSPF_HOP_COUNT if hop else 0)
    dist = np.zeros((g.V, g.V), np.uint32)
    dig = np.zeros((g.V, 3), np.uint64)
    nh = {}
    for cap in sorted(set(caps.tolist())):
        grp = np.flatnonzero(caps == cap).astype(np.uint32)
        W = max(1, (cap + 31) // 32)
        d_r = dev_u32(grp)
        d_d = torch.empty((grp.size, g.V), dtype=torch.int32, device=DEV)
        d_n = torch.empty((grp.size, g.V, W), dtype=torch.int32, device=DEV)
        d_g = torch.empty((grp.size, 3), dtype=torch.int64, device=DEV)
        eng.run_dev(d_r.data_ptr(), grp.size, W, flags=flags, d_dist=d_d.data_ptr(),
                    d_nh=d_n.data_ptr(), d_digest=d_g.data_ptr(), max_root_neighbors=int(cap))
        eng.sync()
        dist[grp] = host_u32(d_d)
        dig[grp] = d_g.cpu().numpy().view(np.uint64)
        n_h = host_u32(d_n)
        nh.update({int(r): n_h[j] for j, r in enumerate(grp)})
    return (lambda grp, W: (dist[grp], np.stack([nh[int(r)] for r in grp]))), dig


def check_batches(name, g, eng, hop=False, tag=None, exp_name=None):
    rows, dig = run_classes(g, eng, hop)
    ref = exp_name or name
    check_rows(g, M.expected(ref, not hop), rows, (name, tag, hop))
    check_digests(g, dig, M.digests(ref, not hop), (name, tag, hop))


def check_whole_sweep(name, g, sw, tag, runs=1):
    for rep in range(runs):
        if rep:
            sw.poison()
        sw.run()
        sw.engine.sync()
        check_sweep(g, sw, M.expected(name), M.digests(name), (name, tag, rep))


def unit_names(sw):
    return [p["name"] for p in sw.profile(1)]


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------- L1. packed edge entries
@pytest.mark.parametrize("knob", list(WD_KNOBS))
@pytest.mark.parametrize("name", ["P16", "P17"])
def test_l1_dial_with_and_without_packed_entries(name, knob, monkeypatch):
    """Variant 7 over metrics {1, 2, 0xFFFE, 0xFFFF} (packed entries) and with
    one 0x10000 (the separate arrays): every root, link metrics and hop count."""
    set_env(monkeypatch, {"OSPF_FORCE_VARIANT": "7", **WD_KNOBS[knob]})
    g, eng = engine_for(name)
    try:
        assert eng.plan(1)["variant"] == 7
        assert eng.info().max_metric == M.STATED[name]["wmax"]
        check_batches(name, g, eng, False, knob)
        check_batches(name, g, eng, True, knob)
    finally:
        eng.close()


def test_l1_patch_across_0xffff_and_back(monkeypatch):
    """ospf_update_links takes p03 -> p04 from 0xFFFF to 0x10000 and back. The
    first step drops the packed entries, and they stay dropped until the next
    load (the later steps run the separate arrays over metrics that would fit
    again): every root == the oracle of that state after each step."""
    monkeypatch.setenv("OSPF_FORCE_VARIANT", "7")
    g, eng = engine_for("P16")
    try:
        rp, col, lid = g.csr["row_ptr"], g.csr["col"], g.csr["link_id"]
        a, b = g.ids["p03"], g.ids["p04"]
        assert a < b  # metric_lo is the lower id's direction
        e = next(e for e in range(int(rp[a]), int(rp[a + 1])) if col[e] == b)
        check_batches("P16", g, eng, tag="load")
        for step, (m, state) in enumerate([(0x10000, "P17"), (0xFFFF, "P16"), (0x10000, "P17")]):
            eng.update_links([(int(lid[e]), 1, m, 0xFFFF)], version=2 + step)
            check_batches("P16", g, eng, tag=("patched", step), exp_name=state)
            check_batches("P16", g, eng, hop=True, tag=("patched", step), exp_name=state)
    finally:
        eng.close()


# --------------------------------------------- L2. the Dial's packed distance field
K_SHAPES = ["K16_m1", "K16_0", "K16_p1", "K8_m1", "K8_0", "K8_p1"]


@pytest.mark.parametrize("group", ["1", "16"])
@pytest.mark.parametrize("pack", [None, "8", "16", "0"])
@pytest.mark.parametrize("name", K_SHAPES)
def test_l2_packed_distance_field_limits(name, pack, group, monkeypatch):
    """dist(k0, e3) = infk - 1 stays packed, infk and infk + 1 abort the
    packed run and rerun the root unpacked (infk itself is the field's INF):
    k0's row and every other root's == the oracle, at a wave and a 16-wave
    group per root, K automatic, forced and off."""
    set_env(monkeypatch, {"OSPF_FORCE_VARIANT": "7", "OSPF_WD_GROUP": group})
    if pack is not None:
        monkeypatch.setenv("OSPF_WD_PACK", pack)
    g, eng = engine_for(name)
    try:
        k0, e3 = g.ids["k0"], g.ids["e3"]
        grp, dist, nh = M.expected(name)[1]
        assert dist[np.searchsorted(grp, k0), e3] == M.STATED[name]["far"]
        check_batches(name, g, eng, False, (pack, group))
    finally:
        eng.close()


@pytest.mark.parametrize("group", [None, "1"])
def test_l2_neighbour_counts_across_the_k_choice(group, monkeypatch):
    """Roots of exactly 8, 9, 16 and 17 distinct neighbours (K = 8, 16, 16,
    unpacked), distances on either side of 0xFFFF."""
    monkeypatch.setenv("OSPF_FORCE_VARIANT", "7")
    if group:
        monkeypatch.setenv("OSPF_WD_GROUP", group)
    g, eng = engine_for("KNBR")
    try:
        check_batches("KNBR", g, eng, False, group)
    finally:
        eng.close()


@pytest.mark.parametrize("hub", ["h08", "h09", "h16", "h17"])
def test_l2_exact_neighbour_bound_picks_k(hub, monkeypatch):
    """Each hub alone with max_root_neighbors = its exact neighbour count (8,
    9, 16, 17; OSPF_WD_PACK unset): the engine's own K choice sees 9 and 17.
    A K too small for the root would raise device error bit 1."""
    monkeypatch.setenv("OSPF_FORCE_VARIANT", "7")
    g, eng = engine_for("KNBR")
    try:
        r, n = g.ids[hub], M.STATED["KNBR"]["nbrs"][hub]
        assert eng.root_neighbors(r).size == n
        flags = N.OSPF_WANT_DIST | N.OSPF_WANT_NH | N.OSPF_WANT_DIGEST
        d_r = dev_u32([r])
        d_d = torch.empty((1, g.V), dtype=torch.int32, device=DEV)
        d_n = torch.empty((1, g.V, 1), dtype=torch.int32, device=DEV)
        d_g = torch.empty((1, 3), dtype=torch.int64, device=DEV)
        eng.run_dev(d_r.data_ptr(), 1, 1, flags=flags, d_dist=d_d.data_ptr(), d_nh=d_n.data_ptr(),
                    d_digest=d_g.data_ptr(), max_root_neighbors=n)
        eng.sync()
        exp = M.expected("KNBR", roots=(r,))
        check_rows(g, exp, lambda grp, W: (host_u32(d_d), host_u32(d_n)), (hub, n))
        assert np.array_equal(d_g.cpu().numpy().view(np.uint64)[0], M.digests("KNBR")[r])
    finally:
        eng.close()


# ------------------------------------------------------------- L3. ring Dial
@pytest.mark.parametrize("name", ["R63", "R64"])
def test_l3_ring_dial_admission(name, monkeypatch):
    """Largest metric 63: variant 6 (64 buckets) is admitted and == the
    oracle; 64: the planner keeps another variant, == the oracle too."""
    monkeypatch.setenv("OSPF_FORCE_VARIANT", "6")
    g, eng = engine_for(name)
    try:
        assert eng.info().max_metric == M.STATED[name]["wmax"]
        assert (eng.plan(1)["variant"] == 6) == (name == "R63"), eng.plan(1)
        roots = np.arange(g.V, dtype=np.uint32)
        out = eng.run(roots, 1, want_digest=True)
        check_rows(g, M.expected(name), lambda grp, W: (out["dist"][grp], out["nh"][grp]), name)
        check_digests(g, out["digest"], M.digests(name), name)
    finally:
        eng.close()


# ------------------------------------------------------- L4. u16 slot table
def wide_from_oracle(g, eng, name, W, roots, offset=0):
    """ospf_wderive_wide_dev over the oracle's dist rows (row v = node v), at
    `offset` words off a 16-B boundary -> (nh [n, V, W], digests [n, 3])"""
    V = g.V
    src = torch.zeros(V * V + offset, dtype=torch.int32, device=DEV)
    src[offset:] = dev_u32(M.dist_rows(name).reshape(-1))
    d_pos = dev_u32(np.arange(V))
    d_r = dev_u32(roots)
    nh = torch.empty(len(roots) * V * W + offset, dtype=torch.int32, device=DEV)
    dg = torch.empty((len(roots), 3), dtype=torch.int64, device=DEV)
    eng.wderive_wide_dev(d_r.data_ptr(), len(roots), W, src.data_ptr() + 4 * offset,
                         d_pos.data_ptr(), nh.data_ptr() + 4 * offset, d_digest=dg.data_ptr())
    eng.sync()
    return host_u32(nh[offset:]).reshape(len(roots), V, W), dg.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("ctiles", [None, "1"])
def test_l4_lane_derive_at_0xfffe(ctiles, offset, monkeypatch):
    """h0 -> s128 at 0xFFFE is the largest value the u16 slot table holds
    (0xFFFF marks an empty slot) and the only way to s128: bit 128 of word 4.
    Both hubs as one run, from the oracle's dist rows, vector and scalar
    loads; the narrower classes through the same entry point."""
    if ctiles:
        monkeypatch.setenv("OSPF_WL_CTILES", ctiles)
    name = "H129_fffe"
    g, eng = engine_for(name)
    try:
        assert g.V % 4 == 0
        for W, (grp, _, want) in M.expected(name).items():
            nh, dg = wide_from_oracle(g, eng, name, W, grp, offset)
            assert np.array_equal(nh, want), (W,) + first_diff(g, grp, nh, want)
            assert np.array_equal(dg, M.digests(name)[grp]), W
        grp, _, want = M.expected(name)[5]
        assert grp.tolist() == [g.ids["h0"], g.ids["h1"]]
        assert want[0, g.ids["s128"]].tolist() == [0, 0, 0, 0, 1]
    finally:
        eng.close()


@pytest.mark.parametrize("hip_graph", [False, True])
@pytest.mark.parametrize("nonh", [False, True])
def test_l4_cover_sweep_at_0xfffe(nonh, hip_graph, monkeypatch):
    if nonh:
        set_env(monkeypatch, {"OSPF_SEED_NONH": "1", "OSPF_CLOSURE_NONH": "1"})
    g, eng = engine_for("H129_fffe")
    try:
        sw = Sweep(eng, mode="wcover", hip_graph=hip_graph)
        try:
            assert sw.mode == "wcover" and sw.hip_graph == hip_graph and sw.max_nh_words == 5
            if nonh:
                assert "wderive_wide_w5" in unit_names(sw), unit_names(sw)
            check_whole_sweep("H129_fffe", g, sw, (nonh, hip_graph), runs=2 if hip_graph else 1)
        finally:
            sw.close()
    finally:
        eng.close()


def test_l4_wmulti_sweep_at_0xfffe():
    """The multi-root sweep plans the same lane derive for the hubs."""
    g, eng = engine_for("H129_fffe")
    try:
        sw = Sweep(eng, mode="wmulti")
        try:
            assert sw.mode == "wmulti" and "wderive_wide_w5" in unit_names(sw), unit_names(sw)
            check_whole_sweep("H129_fffe", g, sw, "wmulti", runs=2)
        finally:
            sw.close()
    finally:
        eng.close()


def test_l4_0xffff_is_refused_when_the_sweep_is_created(monkeypatch):
    """A hub metric of 0xFFFF cannot enter the slot table: the ABI call and an
    explicit cover or multi-root sweep refuse it with OSPF_E_RANGE at create
    -- a deferred sweep too, whose first launch is the caller's run -- and
    AUTO takes a mode without the table, == the oracle."""
    name = "H129_ffff"
    g, eng = engine_for(name)
    try:
        grp = M.expected(name)[5][0]
        with pytest.raises(EngineError) as ei:
            wide_from_oracle(g, eng, name, 5, grp)
        assert ei.value.code == N.OSPF_E_RANGE, ei.value
        for env in ({}, {"OSPF_SEED_NONH": "1", "OSPF_CLOSURE_NONH": "1"}):
            set_env(monkeypatch, env)
            for kw in (dict(), dict(defer=True, hip_graph=False)):
                for mode in ("wcover", "wmulti"):  # both plan the lane derive for the hubs
                    with pytest.raises(EngineError) as ei:
                        Sweep(eng, mode=mode, **kw)
                    assert ei.value.code == N.OSPF_E_RANGE, (env, kw, mode, ei.value)
            sw = Sweep(eng)
            try:
                assert sw.mode != "wcover", sw.mode
                check_whole_sweep(name, g, sw, ("auto", sw.mode, tuple(env)), runs=2)
            finally:
                sw.close()
    finally:
        eng.close()


# ------------------------------------------------- L5. leaf in-link metric
def test_l5_cover_pipeline_at_65535():
    """c01 -> lf at 65535 fills the high half of lf's ladj word: cover rows,
    leaf rows and next hops of every root through cover_prepare /
    cover_dist_dev / wderive_dev / wderive_wide_dev == the oracle."""
    name = "C65535"
    g, eng = engine_for(name)
    try:
        got, cover, dist, pos = cover_pipeline(eng, g.csr)
        want_d = M.dist_rows(name)
        assert np.array_equal(dist[pos[cover]], want_d[cover]), first_diff(g, cover, dist[pos[cover]], want_d[cover])
        assert sorted(got) == list(range(g.V)) and g.ids["lf"] not in cover.tolist()
        for W, (grp, d, nh) in M.expected(name).items():
            for j, r in enumerate(grp.tolist()):
                assert np.array_equal(got[r][0], d[j]), g.names[r]
                assert np.array_equal(got[r][1], nh[j]), g.names[r]
                assert np.array_equal(got[r][2], M.digests(name)[r]), g.names[r]
    finally:
        eng.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_l5_cover_sweep_at_65535(tiled, monkeypatch):
    if tiled:
        monkeypatch.setenv("OSPF_COVER_ROWS_TILED", "1")
    g, eng = engine_for("C65535")
    try:
        sw = Sweep(eng, mode="wcover")
        try:
            assert sw.mode == "wcover"
            check_whole_sweep("C65535", g, sw, tiled, runs=2)
        finally:
            sw.close()
    finally:
        eng.close()


def test_l5_65536_is_refused_and_auto_steps_aside():
    name = "C65536"
    g, eng = engine_for(name)
    try:
        leaf = shard.leaf_set(g.csr["row_ptr"], g.csr["col"])
        with pytest.raises(EngineError) as ei:
            eng.cover_prepare(leaf)
        assert ei.value.code == N.OSPF_E_RANGE and "65535" in str(ei.value), ei.value
        with pytest.raises(EngineError) as ei:
            Sweep(eng, mode="wcover")
        assert ei.value.code == N.OSPF_E_RANGE, ei.value
        sw = Sweep(eng)
        try:
            assert sw.mode != "wcover", sw.mode
            check_whole_sweep(name, g, sw, ("auto", sw.mode), runs=2)
        finally:
            sw.close()
    finally:
        eng.close()


# ------------------------------------------------------------ L6. closure
@pytest.mark.parametrize("name", ["CL30_m1", "CL30_0"])
def test_l6_closure_distance_bound(name):
    """Distance bound 2^30 - 1: the cover sweep takes the closure; 2^30: it
    runs every cover row by the Dial. Digests of all roots and the rows of
    sampled roots == the oracle either way."""
    g, eng = engine_for(name)
    try:
        sw = Sweep(eng, mode="wcover")
        try:
            assert ("cover_closure" in unit_names(sw)) == (name == "CL30_m1"), unit_names(sw)
            sw.run()
            eng.sync()
            assert sorted(sw.roots.tolist()) == list(range(g.V))
            check_digests(g, sweep_digests(sw), M.digests(name, fast=True), name)
            pick = tuple(sorted({g.ids[n] for n in ("3-7-5", "2-7-0", "1-0-0", "3-0-0")} |
                                set(range(3, g.V, 211))))
            check_rows(g, M.expected(name, roots=pick), sw.rows, name)
        finally:
            sw.close()
    finally:
        eng.close()


# ---------------------------------------------------------- L7. u32 range
def leaf_rows_from_oracle(g, eng, name, lr):
    """ospf_wderive_dev of the leaf roots over the oracle's dist rows"""
    V = g.V
    src = dev_u32(M.dist_rows(name))
    d_pos, d_r = dev_u32(np.arange(V)), dev_u32(lr)
    dist = torch.empty((lr.size, V), dtype=torch.int32, device=DEV)
    nh = torch.empty((lr.size, V), dtype=torch.int32, device=DEV)
    dg = torch.empty((lr.size, 3), dtype=torch.int64, device=DEV)
    eng.wderive_dev(d_r.data_ptr(), lr.size, src.data_ptr(), d_pos.data_ptr(), dist.data_ptr(),
                    d_nh=nh.data_ptr(), d_digest=dg.data_ptr())
    eng.sync()
    return host_u32(dist), host_u32(nh).reshape(lr.size, V, 1), dg.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("pack", [None, "0"])
def test_l7_dial_at_bound_2_32_minus_2(pack, monkeypatch):
    monkeypatch.setenv("OSPF_FORCE_VARIANT", "7")
    if pack:
        monkeypatch.setenv("OSPF_WD_PACK", pack)
    g, eng = engine_for("U32_m2")
    try:
        assert int(M.dist_rows("U32_m2")[g.ids["n0"], g.ids["x"]]) == 2 ** 32 - 16
        check_batches("U32_m2", g, eng, False, pack)
    finally:
        eng.close()


def test_l7_derive_kernels_at_bound_2_32_minus_2():
    """wderive_dev of the leaves from the oracle's rows (lr's term through n0
    passes 2^32: the saturating add), wderive_wide_dev of the cover roots,
    and the cover pipeline."""
    name = "U32_m2"
    g, eng = engine_for(name)
    try:
        leaf = shard.leaf_set(g.csr["row_ptr"], g.csr["col"])
        lr = np.flatnonzero(leaf).astype(np.uint32)
        assert g.ids["lr"] in lr.tolist()
        grp, want_d, want_n = M.expected(name)[1]
        dist, nh, dg = leaf_rows_from_oracle(g, eng, name, lr)
        assert np.array_equal(dist, want_d[lr]), first_diff(g, lr, dist, want_d[lr])
        assert np.array_equal(nh, want_n[lr]), first_diff(g, lr, nh, want_n[lr])
        assert np.array_equal(dg, M.digests(name)[lr])
        cover = np.flatnonzero(~leaf).astype(np.uint32)
        nh, dg = wide_from_oracle(g, eng, name, 1, cover)
        assert np.array_equal(nh, want_n[cover]), first_diff(g, cover, nh, want_n[cover])
        assert np.array_equal(dg, M.digests(name)[cover])
        got, cover2, cd, pos = cover_pipeline(eng, g.csr)
        assert np.array_equal(cd[pos[cover2]], want_d[cover2])
        for r in range(g.V):
            assert np.array_equal(got[r][0], want_d[r]) and np.array_equal(got[r][1], want_n[r]), g.names[r]
            assert np.array_equal(got[r][2], M.digests(name)[r]), g.names[r]
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ["wderive", "batch", "wcover"])
def test_l7_sweeps_at_bound_2_32_minus_2(mode):
    g, eng = engine_for("U32_m2")
    try:
        sw = Sweep(eng, mode=mode)
        try:
            assert sw.mode == mode
            check_whole_sweep("U32_m2", g, sw, mode, runs=2)
        finally:
            sw.close()
    finally:
        eng.close()


def armed(stream):
    """A LinkState that does not degrade and whose next engine call fails: a
    query raises "injected" exactly when it goes to the engine."""
    p = LinkState(stream=stream)
    p.set_degrade(False)
    p.inject_engine_error(1)
    return p


def test_l7_linkstate_stays_on_the_engine_at_bound_2_32_minus_2():
    """odl::LinkState's own switch to its host path is the same comparison
    (bound >= 2^32 - 1): at 2^32 - 2 link-metric SPF and KSP2 == the oracle
    and are answered by the engine, shown by the armed engine error."""
    g = M.shape("U32_m2")
    p = LinkState(stream=g.stream)
    p.set_degrade(False)
    for src in ("lr", "n0"):
        assert p.ksp2_text(src, g.names) == g.oracle.ksp2_text(src, g.names), src
    for r in g.names:
        assert p.spf_text(r) == g.oracle.spf_text(r), r
    assert p.counters()["engine_errors"] == 0 and p.counters()["engine_degraded"] == 0
    for query in (lambda q: q.ksp2_text("lr", g.names), lambda q: q.spf_text("n0")):
        with pytest.raises(LinkStateError, match="injected"):
            query(armed(g.stream))


def test_l7_bound_2_32_minus_1_is_refused():
    """Every link-metric entry point refuses a distance bound of 2^32 - 1
    with OSPF_E_RANGE; hop count still answers; odl::LinkState answers link
    metrics from its host path of its own accord and hop count from the engine."""
    name = "U32_m1"
    g, eng = engine_for(name)
    try:
        V = g.V
        leaf = shard.leaf_set(g.csr["row_ptr"], g.csr["col"])
        lr = np.flatnonzero(leaf).astype(np.uint32)
        d_all = dev_u32(np.arange(V))
        buf = torch.zeros((V, V), dtype=torch.int32, device=DEV)
        eng.cover_prepare(leaf)  # the graph itself is a valid cover input
        calls = {
            "run": lambda: eng.run(np.arange(V, dtype=np.uint32), 1),
            "sweep": lambda: Sweep(eng),
            "sweep_batch": lambda: Sweep(eng, mode="batch"),
            "wderive": lambda: leaf_rows_from_oracle(g, eng, name, lr),
            "wderive_wide": lambda: wide_from_oracle(g, eng, name, 1, np.flatnonzero(~leaf)),
            "cover_dist": lambda: eng.cover_dist_dev(d_all.data_ptr(), 1, buf.data_ptr()),
            "ksp2": lambda: eng.ksp2(g.ids["lr"], np.arange(V, dtype=np.uint32)),
        }
        for what, call in calls.items():
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == N.OSPF_E_RANGE, (what, ei.value)
        out = eng.run(np.arange(V, dtype=np.uint32), 1, hop_count=True, want_digest=True)
        check_rows(g, M.expected(name, False), lambda grp, W: (out["dist"][grp], out["nh"][grp]), "hop")
        check_digests(g, out["digest"], M.digests(name, False), "hop")
    finally:
        eng.close()
    # LinkState chooses its host path by itself (nothing forces it): the
    # armed engine error never fires for link metrics, and fires for hop count
    p = armed(g.stream)
    for r in g.names:
        assert p.spf_text(r) == g.oracle.spf_text(r), r
    assert p.ksp2_text("lr", g.names) == g.oracle.ksp2_text("lr", g.names)
    assert p.counters()["engine_errors"] == 0 and p.counters()["engine_degraded"] == 0
    with pytest.raises(LinkStateError, match="injected"):
        p.spf_text("lr", False)
    p = LinkState(stream=g.stream)
    p.set_degrade(False)
    for r in g.names:
        assert p.spf_text(r, False) == g.oracle.spf_text(r, False), r


def test_l7_cover_shortcut_weight_reaching_2_32_minus_1_is_refused():
    """ABI: a shortcut c01 -> lf -> c02 of weight 2^31 + (2^31 - 1) = 2^32 - 1
    is refused by ospf_cover_prepare; one less is not a shortcut overflow."""
    g = M.shape("C65535")
    rp, col = g.csr["row_ptr"], g.csr["col"]

    def entry(a, b):
        return next(e for e in range(int(rp[g.ids[a]]), int(rp[g.ids[a] + 1])) if col[e] == g.ids[b])

    leaf = shard.leaf_set(rp, col)
    for into, msg in ((2 ** 31, "shortcut weight overflow"), (2 ** 31 - 1, "leaf in-link metric")):
        csr = {k: v.copy() for k, v in g.csr.items()}
        csr["metric"][entry("c01", "lf")] = into
        csr["metric"][entry("lf", "c02")] = 2 ** 31 - 1
        _, eng = engine_for("C65535", csr)
        try:
            with pytest.raises(EngineError) as ei:
                eng.cover_prepare(leaf)
            assert ei.value.code == N.OSPF_E_RANGE and msg in str(ei.value), ei.value
        finally:
            eng.close()
