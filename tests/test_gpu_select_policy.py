"""Device-side route selection under the reference's best-route policy
(ospf_sweep_select_policy*, ospf_msweep_select_policy,
LinkState.all_sources_select_policy): createRouteForPrefix's four steps
(openr/decision/SpfSolver.cpp:229-244, 649-676, 709-731, 990-1000) for every
root and every prefix.

Expected values come from selpolicy_ref.expect: the four steps restated in
Python over the CPU oracle's SPF results and the CSR columns, never the
engine's rows or its packed key."""
import numpy as np
import pytest
import torch

import select_ref as R
import selpolicy_ref as PR
from graphs import metric_graph
from openr_amd.adjdb import AdjDb, AdjDbStream, create_adjacency
from openr_amd.engine import Engine, EngineError, Multi, MultiSweep, Sweep
from openr_amd.linkstate import LinkState
from oracle import Oracle, parse_spf_text

pytestmark = pytest.mark.gpu

FF = 0xFFFFFFFF
GUARD = 16  # poisoned words kept before and after every device output


def load(stream):
    ls = LinkState()
    ls.apply(stream)
    names, csr = ls.node_names(), ls.csr()
    eng = Engine()
    eng.load(csr)
    return names, csr, eng


def engine_for(kind, seed, n=70):
    return load(R.graph(kind, seed, n)[0])


def oracle_of(stream, names, use_link_metric=True):
    orc = Oracle(stream)
    return {r: parse_spf_text(orc.spf_text(r, use_link_metric)) for r in names}


def by_node(sw, arrs):
    out = {}
    for k, a in arrs.items():
        b = np.zeros_like(a)
        b[sw.roots] = a
        out[k] = b
    return out


def modes_for(kind, hop):
    if hop or kind.endswith("unit"):
        return ("lds", "derive", "wderive", "batch")
    return ("wderive", "batch", "wcover")


def sweeps(eng, modes, hop=False):
    """every mode's sweep, run; modes outside a kernel's contract
    (EngineError -4) are skipped as in test_gpu_sweep.py"""
    for mode in modes:
        try:
            sw = Sweep(eng, mode=mode, hop_count=hop)
        except EngineError as e:
            assert e.code == -4, (mode, e)
            continue
        try:
            sw.run()
            eng.sync()
            yield mode, sw
        finally:
            sw.close()


def select(sw, table, pref, mnh, nh_words=0, want=PR.KEYS):
    off, nodes = R.csr_table(table)
    return by_node(sw, sw.select_policy(off, nodes, PR.flat(pref), PR.flat(mnh), nh_words, want))


# ---------------------------------------------------------------- every mode
@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("kind,seed", [("unit", 0), ("weighted", 1), ("sparse-weighted", 1)])
def test_policy_every_sweep_mode(kind, seed, hop):
    names, csr, eng = engine_for(kind, seed)
    try:
        assert np.asarray(csr["no_transit"]).any(), "this seed must have drained nodes"
        spf = R.oracle_spf(kind, seed, 70, tuple(names), not hop)
        rng = np.random.default_rng(200 + seed)
        table = R.random_table(70, rng)
        pref, mnh = PR.random_policy(table, rng, classes=3, max_need=4)
        wants, ran = {}, []
        for mode, sw in sweeps(eng, modes_for(kind, hop), hop):
            W = sw.max_nh_words
            if W not in wants:
                wants[W] = PR.expect(spf, names, csr, table, pref, mnh, W, hop)
            want, facts = wants[W]
            for k in ("filtered", "need_outside_L", "withheld", "best_outside"):
                assert facts[k] > 0, (k, facts)
            if kind.startswith("sparse"):
                assert facts["fallback"] > 0, facts
            PR.assert_equal(select(sw, table, pref, mnh), want, ctx=(mode, hop))
            ran.append(mode)
        assert "batch" in ran
    finally:
        eng.close()


def test_uniform_policy_is_the_plain_selection():
    """All pref 0, no drained node, no threshold: metric / count / nh are the
    oracle expectation of the plain selection (select_ref.expect)."""
    dbs = metric_graph([("a", "b", 1, 2), ("b", "c", 3, 1), ("c", "d", 1, 1), ("d", "a", 2, 2),
                        ("a", "c", 5, 5), ("d", "e", 1, 4), ("e", "f", 2, 2), ("f", "b", 1, 1),
                        ("g", "h", 1, 1)])
    st = AdjDbStream.from_dbs(dbs)
    names, csr, eng = load(st)
    try:
        assert not np.asarray(csr["no_transit"]).any()
        spf = oracle_of(st, names)
        V = len(names)
        table = [[]] + [[v] for v in range(V)] + [[0, 3], [1, 4, 5], [2, 6], list(range(V)), [6, 7]]
        pref, mnh = PR.uniform_policy(table)
        plain = R.expect(spf, names, csr, table, 1)
        ran = 0
        for mode, sw in sweeps(eng, ("wderive", "batch")):
            got = select(sw, table, pref, mnh)
            for k, w in zip(("metric", "count", "nh"), plain):
                assert np.array_equal(got[k], w), (mode, k)
            assert not got["need"].any()
            off, nodes = R.csr_table(table)
            old = sw.select(off, nodes)
            for k, o in zip(("metric", "count", "nh"), old):  # and the old kernel's answer
                b = np.zeros_like(o)
                b[sw.roots] = o
                assert np.array_equal(got[k], b), (mode, k)
            ran += 1
        assert ran
    finally:
        eng.close()


# ---------------------------------------------------------------- key edges
def test_key_edges_unsigned_and_high_word_first():
    """The 64-bit key at its edges: pref 2^31 - 1 on a drained announcer
    beside 2^31 - 2 (the high word reads 0xFFFFFFFF / 0xFFFFFFFC), a pref of
    2^30 against 1 (bit 31 of the high word), and distances with bit 31 set.
    An adjacency metric is an i32 (the ingest refuses 0x80000005 on one link),
    so the largest it admits is used: a -> b costs 0x7FFFFFFF and b -> c 6,
    which puts c at 0x80000005 from a and everything behind it above 2^31; the
    way back costs 1, so the distance bound stays below 2^32 - 1. A signed
    compare of either half, or the low half compared first, picks another
    announcer in at least one of these prefixes."""
    m31 = 0x7FFFFFFF
    dbs = metric_graph([("a", "b", m31, 1), ("b", "c", 6, 1), ("b", "d", 8, 2), ("c", "d", 1, 1),
                        ("c", "e", 4, 4)], overloaded=("d",))
    st = AdjDbStream.from_dbs(dbs)
    names, csr, eng = load(st)
    try:
        a, b, c, d, e = range(5)
        assert names == ["a", "b", "c", "d", "e"] and csr["no_transit"][d]
        spf = oracle_of(st, names)
        far = 0x80000005
        assert spf["a"]["b"][0] == m31 and spf["a"]["c"][0] == far and spf["a"]["e"][0] == far + 4
        top = 2 ** 31 - 1
        table = [[c, d], [b, c], [a, c], [a, e], [b, e], [c, e], [a, b, c, d, e], [b, c]]
        pref = [[top - 1, top], [top, top - 1], [0, 0], [2 ** 30, 1], [2 ** 30, 1], [0, 0],
                [top, top, top, top - 1, top], [7, 7]]
        mnh = [[1, 3], [0, 2], [0, 0], [0, 0], [1, 0], [0, 0], [0, 0, 0, 5, 0], [0, 0]]
        want, _ = PR.expect(spf, names, csr, table, pref, mnh, 1)
        # what the wrong compares would get wrong, from the oracle's numbers
        assert want["metric"][a, 2] == 0 and want["metric"][a, 7] == m31  # low half signed: c
        assert want["best"][a, 3] == e and want["best"][a, 4] == e       # high half signed: a / b
        assert want["best"][a, 0] == c and want["best"][a, 1] == c        # low half first: d / b
        assert want["metric"][a, 5] == far and want["best"][a, 6] == d
        ran = 0
        for mode, sw in sweeps(eng, ("wderive", "batch", "wcover")):
            PR.assert_equal(select(sw, table, pref, mnh), want, ctx=mode)
            ran += 1
        assert ran, "no sweep mode admits the 0x7FFFFFFF metric"
    finally:
        eng.close()


# ---------------------------------------------------------------- links
@pytest.mark.parametrize("hop", [False, True])
def test_links_count_parallel_up_links_at_the_smallest_metric(hop):
    dbs = metric_graph([("r", "x", 1, 1), ("r", "x", 1, 1),          # two equal links: 2
                        ("r", "y", 1, 1), ("r", "y", 3, 1),          # unequal: 1, 2 under hop count
                        ("r", "z", 1, 1), ("r", "z", 1, 1, "down"),  # a down link never counts
                        ("x", "t", 1, 1), ("y", "t", 1, 1)])
    st = AdjDbStream.from_dbs(dbs)
    names, csr, eng = load(st)
    try:
        r, t, x, y, z = (names.index(n) for n in "rtxyz")
        spf = oracle_of(st, names, not hop)
        table = [[x], [y], [z], [t], [x, y, z]]
        pref, mnh = PR.uniform_policy(table)
        mnh[3] = [4]
        want, _ = PR.expect(spf, names, csr, table, pref, mnh, 1, hop)
        assert want["links"][r].tolist() == [2, 2 if hop else 1, 1, 4 if hop else 3, 5 if hop else 4]
        assert bool(want["installed"][r, 3]) == hop  # need 4: 3 links under link metric
        ran = 0
        for mode, sw in sweeps(eng, ("wderive", "batch", "derive"), hop):
            PR.assert_equal(select(sw, table, pref, mnh), want, ctx=mode)
            ran += 1
        assert ran
    finally:
        eng.close()


# ---------------------------------------------------------------- wide root
def hub_stream():
    """A hub with 150 spokes (5 next-hop words: the lane-per-word path), two
    of them over two parallel links, the spokes in a ring with a few chords,
    some metrics > 1, a few spokes drained."""
    rng = np.random.default_rng(21)
    n = 150
    names = ["hub"] + [f"s{i:03d}" for i in range(n)]
    adjs = {nm: [] for nm in names}

    def link(a, b, m, tag=""):
        adjs[a].append(create_adjacency(b, f"{a}-{b}{tag}", f"{b}-{a}{tag}", m))
        adjs[b].append(create_adjacency(a, f"{b}-{a}{tag}", f"{a}-{b}{tag}", m))

    for i in range(n):
        m = int(rng.integers(1, 4))
        link("hub", names[1 + i], m)
        if i in (40, 140):
            link("hub", names[1 + i], m, "-2")
        link(names[1 + i], names[1 + (i + 1) % n], int(rng.integers(1, 4)))
    for i in range(0, n, 17):
        link(names[1 + i], names[1 + (i + 40) % n], 1)
    return AdjDbStream.from_dbs([AdjDb(nm, adjs[nm], i + 1, overloaded=nm in ("s007", "s090"))
                                 for i, nm in enumerate(names)])


def test_policy_wide_root():
    """A root of 5 next-hop words: prefixes of 1, 9 and 65 announcers (and
    more), `links` summed across the words."""
    st = hub_stream()
    names, csr, eng = load(st)
    try:
        hub = names.index("hub")
        assert eng.nh_words(hub) == 5
        V = eng.V
        spf = oracle_of(st, names)
        rng = np.random.default_rng(3)
        table = [[], [hub], [3]] + [sorted(rng.choice(V, size=k, replace=False).tolist())
                                    for k in (9, 65, 130)] + [list(range(1, V))]
        pref, mnh = PR.random_policy(table, rng, classes=2, max_need=4)
        pref[-1], mnh[-1] = [0] * (V - 1), [0] * (V - 2) + [200]
        wants = {W: PR.expect(spf, names, csr, table, pref, mnh, W)[0] for W in (5, 7)}
        # every spoke at once: the nearest ones' next hops lie in all five words
        assert wants[5]["nh"][hub, -1].all() and wants[5]["links"][hub, -1] >= 32
        ran = 0
        for mode, sw in sweeps(eng, ("batch", "wderive", "wcover")):
            for W in (5, 7):
                PR.assert_equal(select(sw, table, pref, mnh, W), wants[W], ctx=(mode, W))
            ran += 1
        assert ran
    finally:
        eng.close()


# ---------------------------------------------------------------- layout
def test_policy_row_pitch_padding_and_one_word():
    """V % 4 != 0 (the sweep's rows keep the packed pitch) and Wout = 1."""
    names, csr, eng = engine_for("unit", 2, 71)
    try:
        spf = R.oracle_spf("unit", 2, 71, tuple(names), True)
        rng = np.random.default_rng(5)
        table = R.random_table(71, rng)
        pref, mnh = PR.random_policy(table, rng)
        want, _ = PR.expect(spf, names, csr, table, pref, mnh, 1)
        ran = 0
        for mode, sw in sweeps(eng, ("derive",)):
            assert sw.max_nh_words == 1
            PR.assert_equal(select(sw, table, pref, mnh, 1), want)
            ran += 1
        assert ran
    finally:
        eng.close()


class Fabric:
    """drained_fabric(6, 4) with its derive sweep, table and expectation"""

    def __init__(self):
        self.names, self.csr, self.eng = engine_for("fabric", 3)
        self.spf = R.oracle_spf("fabric", 3, 70, tuple(self.names), True)
        rng = np.random.default_rng(11)
        self.table = R.fabric_table(self.names, rng) + [[]]
        self.pref, self.mnh = PR.random_policy(self.table, rng)
        self.off, self.nodes = R.csr_table(self.table)
        self.sw = Sweep(self.eng, mode="derive")
        self.sw.run()
        self.eng.sync()
        self._want = {}

    def want(self, W):
        if W not in self._want:
            self._want[W] = PR.expect(self.spf, self.names, self.csr, self.table, self.pref,
                                      self.mnh, W)[0]
        return self._want[W]

    def args(self):
        return self.off, self.nodes, PR.flat(self.pref), PR.flat(self.mnh)

    def close(self):
        self.sw.close()
        self.eng.close()


@pytest.fixture(scope="module")
def fabric():
    f = Fabric()
    yield f
    f.close()


@pytest.mark.parametrize("W", [3, 4, 5])
def test_policy_fabric_output_widths(fabric, W):
    """456 roots of 1 and 3 next-hop words; Wout 3, 4 (16-B stores) and 5."""
    assert fabric.eng.V == 456 and fabric.sw.max_nh_words == 3
    got = by_node(fabric.sw, fabric.sw.select_policy(*fabric.args(), W))
    PR.assert_equal(got, fabric.want(W))


@pytest.mark.parametrize("without", PR.KEYS)
def test_policy_each_output_null_in_turn(fabric, without):
    keys = [k for k in PR.KEYS if k != without]
    got = by_node(fabric.sw, fabric.sw.select_policy(*fabric.args(), 3, keys))
    assert sorted(got) == sorted(keys)
    PR.assert_equal(got, fabric.want(3), keys)


def poisoned(n, P, W):
    """{key: (tensor with GUARD poisoned words either side, words)}"""
    out = {}
    for k in PR.KEYS:
        words = n * P * (W if k == "nh" else 1)
        out[k] = (torch.full((words + 2 * GUARD,), -1, dtype=torch.int32, device="cuda"), words)
    return out

def ptrs(bufs, keys=PR.KEYS):
    return {f"d_{k}": bufs[k][0].data_ptr() + 4 * GUARD for k in keys}


def test_policy_dev_on_a_stream_writes_every_word_and_no_other(fabric):
    sw = fabric.sw
    n, P, W = sw.n_roots, len(fabric.table), 4
    bufs = poisoned(n, P, W)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    sw.select_policy_dev(*fabric.args(), W, stream=stream.cuda_stream, **ptrs(bufs))
    stream.synchronize()
    want = fabric.want(W)
    for k, (t, words) in bufs.items():
        h = t.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == FF).all() and (h[GUARD + words:] == FF).all(), k
        body = h[GUARD:GUARD + words].reshape((n, P, W) if k == "nh" else (n, P))
        full = np.zeros_like(want[k])
        full[sw.roots] = body
        assert np.array_equal(full, want[k]), k
    # 0xFFFFFFFF is a value only of metric and best (no announcer reached)
    for k in ("count", "nh", "links", "need"):
        assert not (bufs[k][0].cpu().numpy().view(np.uint32)[GUARD:GUARD + bufs[k][1]] == FF).any()


def test_msweep_policy_equals_single_sweep(fabric):
    m = Multi([0, 0])
    try:
        m.load(fabric.csr)
        ms = MultiSweep(m, mode="derive")
        ms.run()
        a, b = ms.part_roots(0), ms.part_roots(1)
        assert a.size and b.size and a.size + b.size == m.V
        got = ms.select_policy(*fabric.args())
        assert got["nh"].shape == (m.V, len(fabric.table), 3)
        PR.assert_equal(got, fabric.want(3))
        ms.close()
    finally:
        m.close()


# ---------------------------------------------------------------- contract
def test_policy_contract_errors_write_nothing():
    """Every OSPF_E_INVAL (-1) and an injected OSPF_E_DEVICE (-3) leave the
    poisoned outputs untouched; the sweep still answers a good table after."""
    f = Fabric()
    try:
        sw, eng = f.sw, f.eng
        good = [[5, 9, 200], [], [455]]
        gpref, gmnh = [[1, 0, 1], [], [0]], [[2, 0, 1], [], [0]]
        off, nodes = R.csr_table(good)
        want, _ = PR.expect(f.spf, f.names, f.csr, good, gpref, gmnh, 3)
        n = sw.n_roots
        bufs = poisoned(n, 3, 3)

        def untouched():
            torch.cuda.synchronize()
            for k, (t, _) in bufs.items():
                assert (t.cpu().numpy().view(np.uint32) == FF).all(), k

        def still_good():
            PR.assert_equal(select(sw, good, gpref, gmnh), want)

        still_good()
        bad = [
            ([0, 3], [9, 5, 200], [0, 0, 0], None, 3),           # descending
            ([0, 2], [7, 7], [0, 0], None, 3),                   # not strictly ascending
            ([0, 1], [eng.V], [0], None, 3),                     # id >= V
            ([0, 2, 1, 3], [1, 2, 3], [0, 0, 0], None, 3),       # offsets not monotone
            ([0, 3], [5, 9, 200], [0, 2 ** 31, 0], None, 3),     # a pref >= 2^31
            ([0, 3], [5, 9, 200], None, None, 3),                # no pref
            (off, nodes, PR.flat(gpref), PR.flat(gmnh), 2),      # nh_words too small
        ]
        for boff, bnodes, bpref, bmnh, W in bad:
            with pytest.raises(EngineError) as ei:
                sw.select_policy_dev(boff, bnodes, bpref, bmnh, W, **ptrs(bufs))
            assert ei.value.code == -1, (boff, bnodes, ei.value)
            untouched()
            with pytest.raises(EngineError) as ei:
                sw.select_policy(boff, bnodes, bpref, bmnh, W)
            assert ei.value.code == -1
            still_good()
        for call in (lambda: sw.select_policy_dev(off, nodes, PR.flat(gpref), PR.flat(gmnh), 3,
                                                  **ptrs(bufs)),
                     lambda: sw.select_policy(off, nodes, PR.flat(gpref), PR.flat(gmnh))):
            eng._L.ospf_inject_error(eng._h, 1)
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == -3
            untouched()
            still_good()
        r = sw.select_policy([0], [], [], [])  # no prefix: OSPF_OK, nothing written
        assert r["metric"].shape == (n, 0)
        # a sweep of an older graph version is stale: the kernel reads the live graph
        drained = int(np.nonzero(np.asarray(f.csr["no_transit"]))[0][0])
        eng.update_nodes([drained], [0], version=2)
        with pytest.raises(EngineError) as ei:
            sw.select_policy_dev(off, nodes, PR.flat(gpref), PR.flat(gmnh), 3, **ptrs(bufs))
        assert ei.value.code == -1
        untouched()
    finally:
        f.close()


# ---------------------------------------------------------------- LinkState
def fabric_prefixes(f):
    attrs = [(1000, 200, 1), (1000, 200, 4), (900, 300, 0)]  # by class rank
    return {f"p{p}": [(f.names[a],) + attrs[c] + (m or None,)
                      for a, c, m in zip(ann, f.pref[p], f.mnh[p])]
            for p, ann in enumerate(f.table)}


def test_linkstate_policy_on_the_device(fabric):
    ls = LinkState()
    ls.apply(R.graph("fabric", 3)[0])
    got = ls.all_sources_select_policy(fabric_prefixes(fabric))
    assert ls.sweep_stats()["sweeps"] == 1 and ls.sweep_stats()["rows_copied"] == 0
    PR.assert_equal(got, fabric.want(3))
    assert np.array_equal(got["installed"], fabric.want(3)["installed"])
    assert ls.counters()["engine_errors"] == 0


def test_linkstate_policy_multi_device(fabric):
    ls = LinkState(devices=[0, 0])
    ls.apply(R.graph("fabric", 3)[0])
    got = ls.all_sources_select_policy(fabric_prefixes(fabric))
    assert ls.sweep_stats()["devices"] == 2
    PR.assert_equal(got, fabric.want(3))


@pytest.mark.parametrize("after", [1, 4])
def test_linkstate_policy_degrades_to_host_path(fabric, after):
    """An injected device error (the load, or the select itself) with degrade
    on: the same arrays from the host path, engine_errors rises."""
    ls = LinkState()
    ls.set_degrade(True)
    ls.apply(R.graph("fabric", 3)[0])
    before = ls.counters()["engine_errors"]
    ls.inject_engine_error(after)
    got = ls.all_sources_select_policy(fabric_prefixes(fabric))
    PR.assert_equal(got, fabric.want(3))
    c = ls.counters()
    assert c["engine_errors"] == before + 1 and c["engine_degraded"] == 1
