"""Device-side anycast route selection over a sweep's resident rows
(ospf_sweep_select*, ospf_msweep_select, LinkState.all_sources_select):
SpfSolver::getNextHopsWithMetric (openr/decision/SpfSolver.cpp:1043-1089)
for every root and every prefix of a table.

Expected values come from the CPU oracle, never from the engine's rows: per
root parse_spf_text(Oracle.spf_text(root)), the reference loop in Python
(select_ref.expect: min over the announcers present, the tie set, the union of
their next-hop names) and the names mapped to bits through the root's
neighbour order (checked against Engine.root_neighbors).

random_stream(seed, n=70) at seeds 0-3 reaches every node from every root
(unit and weighted), so the prefix "announced only by nodes a root does not
reach" is tested on the same generator at p = 0.05, where the test asserts
that such a root exists."""
import numpy as np
import pytest
import torch

import select_ref as R
from openr_amd.engine import Engine, EngineError, Multi, MultiSweep, Sweep
from openr_amd.linkstate import LinkState

pytestmark = pytest.mark.gpu

A5 = 0xA5A5A5A5


def engine_for(kind, seed, n=70):
    st, _ = R.graph(kind, seed, n)
    ls = LinkState()
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    eng = Engine()
    eng.load(csr)
    for r in range(0, eng.V, 9):  # the bit order the expectation uses is the engine's
        assert np.array_equal(eng.root_neighbors(r), R.root_neighbor_ids(csr, r))
    return names, csr, eng


def by_node(sw, arrs):
    out = []
    for a in arrs:
        b = np.zeros_like(a)
        b[sw.roots] = a
        out.append(b)
    return out


def modes_for(kind, hop):
    if hop or kind.endswith("unit"):
        return ("lds", "derive", "wderive", "batch")
    return ("wderive", "batch", "wcover")


def check_modes(kind, seed, n, hop, table, modes=None, nh_words=0):
    """Every sweep mode's select == the oracle-derived expectation, for every
    root; modes outside a kernel's contract (EngineError -4) are skipped as in
    test_gpu_sweep.py, but at least one must run."""
    names, csr, eng = engine_for(kind, seed, n)
    spf = R.oracle_spf(kind, seed, n, tuple(names), not hop)
    off, nodes = R.csr_table(table)
    ran, wants = [], {}
    try:
        for mode in modes or modes_for(kind, hop):
            try:
                sw = Sweep(eng, mode=mode, hop_count=hop)
            except EngineError as e:
                assert e.code == -4, (mode, e)
                continue
            try:
                assert sorted(sw.roots.tolist()) == list(range(eng.V))
                sw.run()
                eng.sync()
                W = nh_words or sw.max_nh_words
                if W not in wants:
                    wants[W] = R.expect(spf, names, csr, table, W)
                want = wants[W]
                got = by_node(sw, sw.select(off, nodes, nh_words))
                for what, g, w in zip(("metric", "count", "nh"), got, want):
                    bad = np.argwhere(g != w)
                    assert bad.size == 0, (mode, hop, what, bad[:5].tolist())
                ran.append(mode)
            finally:
                sw.close()
    finally:
        eng.close()
    assert ran, "no sweep mode ran"
    return ran


@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("kind", ["unit", "weighted"])
def test_select_random_graphs_every_mode(kind, seed, hop):
    table = R.random_table(70, np.random.default_rng(100 + seed))
    ran = check_modes(kind, seed, 70, hop, table)
    assert "batch" in ran


@pytest.mark.parametrize("kind,seed", [("sparse-unit", 0), ("sparse-weighted", 1)])
def test_select_prefix_of_unreached_nodes(kind, seed):
    """A prefix made only of nodes unreachable from some root (picked from the
    oracle's result): that root gets OSPF_DIST_INF, count 0 and a zero mask."""
    names, csr, eng = engine_for(kind, seed)
    eng.close()
    spf = R.oracle_spf(kind, seed, 70, tuple(names), True)
    miss = R.unreached(spf, names)
    assert miss, "this seed must have a root with unreached nodes"
    root = sorted(miss)[0]
    only = [names.index(x) for x in miss[root]]
    table = R.random_table(70, np.random.default_rng(7), extra=[only])
    want = R.expect(spf, names, csr, table, 1)
    r = names.index(root)
    assert want[0][r, -1] == R.INF and want[1][r, -1] == 0 and not want[2][r, -1].any()
    check_modes(kind, seed, 70, False, table)


@pytest.mark.parametrize("nh_words", [3, 4])
def test_select_fabric_all_roots(nh_words):
    """drained_fabric(6, 4): 456 roots, W = 1 (racks, spines) and W = 3
    (fabric switches) in one sweep; nh_words 4 checks the zero padding."""
    names, csr, eng = engine_for("fabric", 3)
    assert eng.V == 456
    assert sorted({eng.nh_words(r) for r in range(eng.V)}) == [1, 3]
    eng.close()
    table = R.fabric_table(names, np.random.default_rng(11))
    assert len(table[0]) == 144 and all(len(a) == 4 for a in table[1:7]) and len(table[7]) == 65
    ran = check_modes("fabric", 3, 70, False, table, modes=("derive", "lds"), nh_words=nh_words)
    assert ran == ["derive", "lds"]


def hub_stream():
    """A hub with 150 spokes (5 next-hop words: the engine's lane-per-word
    path), the spokes in a ring with a few chords, some metrics > 1."""
    from openr_amd.adjdb import AdjDb, AdjDbStream, create_adjacency
    rng = np.random.default_rng(21)
    n = 150
    names = ["hub"] + [f"s{i:03d}" for i in range(n)]
    adjs = {nm: [] for nm in names}

    def link(a, b, m):
        adjs[a].append(create_adjacency(b, f"{a}-{b}", f"{b}-{a}", m))
        adjs[b].append(create_adjacency(a, f"{b}-{a}", f"{a}-{b}", m))

    for i in range(n):
        link("hub", names[1 + i], int(rng.integers(1, 4)))
        link(names[1 + i], names[1 + (i + 1) % n], int(rng.integers(1, 4)))
    for i in range(0, n, 17):
        link(names[1 + i], names[1 + (i + 40) % n], 1)
    return AdjDbStream.from_dbs([AdjDb(nm, adjs[nm], i + 1) for i, nm in enumerate(names)])


def test_select_wide_root():
    """A root with more than 4 next-hop words takes the lane-per-word path:
    single announcers, ties across many spokes, more than 64 announcers."""
    from oracle import Oracle, parse_spf_text
    st = hub_stream()
    ls = LinkState()
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    orc = Oracle(st)
    spf = {r: parse_spf_text(orc.spf_text(r, True)) for r in names}
    eng = Engine()
    eng.load(csr)
    try:
        hub = names.index("hub")
        assert eng.nh_words(hub) == 5
        V = eng.V
        rng = np.random.default_rng(3)
        table = [[], [hub], [3], list(range(V))]
        for k in (2, 9, 64, 65, 130):
            table.append(sorted(rng.choice(V, size=k, replace=False).tolist()))
        off, nodes = R.csr_table(table)
        ran = 0
        wants = {W: R.expect(spf, names, csr, table, W) for W in (5, 7)}
        for mode in ("batch", "wderive", "wcover"):
            try:
                sw = Sweep(eng, mode=mode)
            except EngineError as e:
                assert e.code == -4, (mode, e)
                continue
            try:
                sw.run()
                eng.sync()
                for W in (5, 7):
                    got = by_node(sw, sw.select(off, nodes, W))
                    for g, w in zip(got, wants[W]):
                        assert np.array_equal(g, w), (mode, W)
                ran += 1
            finally:
                sw.close()
        assert ran
    finally:
        eng.close()


def test_select_row_pitch_padding():
    """V % 4 != 0 (the sweep's rows keep the packed pitch there)."""
    table = R.random_table(71, np.random.default_rng(5))
    assert check_modes("unit", 2, 71, False, table, modes=("derive",)) == ["derive"]


def test_select_dev_on_a_stream_writes_every_word():
    """select_dev on a non-null stream == select, into buffers filled with
    0xA5 first: every output word is written (zero padding included)."""
    names, csr, eng = engine_for("fabric", 3)
    table = R.fabric_table(names, np.random.default_rng(11)) + [[]]
    off, nodes = R.csr_table(table)
    sw = Sweep(eng, mode="derive")
    try:
        sw.run()
        eng.sync()
        n, P, W = sw.n_roots, len(table), 4
        want = sw.select(off, nodes, W)
        fill = A5 - (1 << 32)  # the same bits as an int32
        d_m = torch.full((n, P), fill, dtype=torch.int32, device="cuda")
        d_c = torch.full((n, P), fill, dtype=torch.int32, device="cuda")
        d_nh = torch.full((n, P, W), fill, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        sw.select_dev(off, nodes, W, d_metric=d_m.data_ptr(), d_count=d_c.data_ptr(),
                      d_nh=d_nh.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got = [t.cpu().numpy().view(np.uint32) for t in (d_m, d_c, d_nh)]
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert not (got[1] == A5).any() and not (got[2] == A5).any()
        # outputs not asked for stay untouched
        d_c.fill_(fill)
        sw.select_dev(off, nodes, W, d_metric=d_m.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert (d_c.cpu().numpy().view(np.uint32) == A5).all()
        assert np.array_equal(d_m.cpu().numpy().view(np.uint32), want[0])
    finally:
        sw.close()
        eng.close()


def test_msweep_select_equals_single_sweep():
    """Multi([0, 0]): two parts select for their own roots; by node id the
    result is the single sweep's."""
    names, csr, eng = engine_for("fabric", 3)
    table = R.fabric_table(names, np.random.default_rng(11))
    off, nodes = R.csr_table(table)
    sw = Sweep(eng, mode="derive")
    try:
        sw.run()
        eng.sync()
        want = by_node(sw, sw.select(off, nodes, 3))
    finally:
        sw.close()
        eng.close()
    m = Multi([0, 0])
    try:
        m.load(csr)
        ms = MultiSweep(m, mode="derive")
        ms.run()
        a, b = ms.part_roots(0), ms.part_roots(1)
        assert a.size and b.size and a.size + b.size == m.V
        got = ms.select(off, nodes)
        assert got[2].shape == (m.V, len(table), 3)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert ms.select(off[:1], nodes[:0])[0].shape == (m.V, 0)  # no prefix: nothing to do
        ms.close()
    finally:
        m.close()


def test_select_contract():
    """A descending list, an id >= V and nh_words too small are OSPF_E_INVAL
    (-1); after each the sweep still answers a good table."""
    names, csr, eng = engine_for("fabric", 3)
    spf = R.oracle_spf("fabric", 3, 70, tuple(names), True)
    sw = Sweep(eng, mode="derive")
    try:
        sw.run()
        eng.sync()
        good = [[5, 9, 200], [], [455]]
        off, nodes = R.csr_table(good)
        want = R.expect(spf, names, csr, good, 3)

        def still_good():
            for g, w in zip(by_node(sw, sw.select(off, nodes)), want):
                assert np.array_equal(g, w)

        still_good()
        bad_tables = [
            ([0, 3], [9, 5, 200]),          # descending
            ([0, 2], [7, 7]),               # not strictly ascending
            ([0, 1], [eng.V]),              # id >= V
            ([0, 2, 1, 3], [1, 2, 3]),      # offsets not monotone
        ]
        for boff, bnodes in bad_tables:
            with pytest.raises(EngineError) as ei:
                sw.select(boff, bnodes)
            assert ei.value.code == -1, (boff, bnodes, ei.value)
            still_good()
        assert sw.max_nh_words == 3
        with pytest.raises(EngineError) as ei:
            sw.select(off, nodes, 2)
        assert ei.value.code == -1
        still_good()
        m, c, nh = sw.select([0], [])  # no prefix: OSPF_OK, nothing written
        assert m.shape == (sw.n_roots, 0)
    finally:
        sw.close()
        eng.close()


def fabric_prefixes(names, table):
    return {f"p{i}": [names[a] for a in ann] for i, ann in enumerate(table)}


def test_linkstate_all_sources_select():
    st, _ = R.graph("fabric", 3)
    ls = LinkState()
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    spf = R.oracle_spf("fabric", 3, 70, tuple(names), True)
    table = R.fabric_table(names, np.random.default_rng(11))
    got = ls.all_sources_select(fabric_prefixes(names, table))
    assert ls.sweep_stats()["sweeps"] == 1 and ls.sweep_stats()["rows_copied"] == 0
    for g, w in zip(got, R.expect(spf, names, csr, table, 3)):
        assert np.array_equal(g, w)
    # by name: the decoded next hops of a rack towards the spines are its
    # usable fabric switches, as the oracle has them
    rack = next(nm for nm in names if nm.startswith("3-"))
    r = names.index(rack)
    hops = set(ls.next_hop_names(rack, got[2][r, 0], csr, names))
    tight = [names[a] for a in table[0] if names[a] in spf[rack] and spf[rack][names[a]][0] == got[0][r, 0]]
    assert hops == set().union(*[set(spf[rack][a][1]) for a in tight])
    assert ls.counters()["engine_errors"] == 0


def test_linkstate_select_multi_device():
    st, _ = R.graph("fabric", 3)
    ls = LinkState(devices=[0, 0])
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    spf = R.oracle_spf("fabric", 3, 70, tuple(names), True)
    table = R.fabric_table(names, np.random.default_rng(11))
    got = ls.all_sources_select(fabric_prefixes(names, table))
    assert ls.sweep_stats()["devices"] == 2
    for g, w in zip(got, R.expect(spf, names, csr, table, 3)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("after", [1, 2, 3, 4])
def test_linkstate_select_degrades_to_host_path(after):
    """An injected device error (load, sweep create, run or select itself)
    with degrade on: the same arrays from the host path, engine_errors rises."""
    st, _ = R.graph("fabric", 3)
    ls = LinkState()
    ls.set_degrade(True)
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    spf = R.oracle_spf("fabric", 3, 70, tuple(names), True)
    table = R.fabric_table(names, np.random.default_rng(11))
    before = ls.counters()["engine_errors"]
    ls.inject_engine_error(after)
    got = ls.all_sources_select(fabric_prefixes(names, table))
    for g, w in zip(got, R.expect(spf, names, csr, table, 3)):
        assert np.array_equal(g, w)
    c = ls.counters()
    assert c["engine_errors"] == before + 1 and c["engine_degraded"] == 1
