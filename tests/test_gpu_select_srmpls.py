"""Device-side SR_MPLS route selection (ospf_sweep_select_srmpls*,
Sweep.select_srmpls, LinkState.all_sources_select_srmpls): per destination
next hops for every root and every prefix.

Expected values come from srmpls_ref.expect: selectBestPathsSpf with
perDestination restated in Python over the CPU oracle's SPF results and the
CSR columns, never the engine's rows or its packed key. Every device output is
written into a buffer with 16 poisoned words either side."""
import numpy as np
import pytest
import torch

import select_ref as R
import selpolicy_ref as PR
import srmpls_ref as SR
from graphs import metric_graph
from openr_amd.adjdb import AdjDbStream
from openr_amd.engine import Engine, EngineError, Sweep
from openr_amd.linkstate import LinkState
from oracle import Oracle, parse_spf_text
from test_gpu_select_policy import hub_stream

pytestmark = pytest.mark.gpu

FF = 0xFFFFFFFF
GUARD = 16  # poisoned words kept before and after every device output
CLASS_ATTRS = [(1000, 200, 1), (1000, 200, 4), (900, 300, 0)]


def load(stream):
    ls = LinkState()
    ls.apply(stream)
    names, csr = ls.node_names(), ls.csr()
    eng = Engine()
    eng.load(csr)
    return names, csr, eng


def oracle_of(stream, names, use_link_metric=True):
    orc = Oracle(stream)
    return {r: parse_spf_text(orc.spf_text(r, use_link_metric)) for r in names}


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


def shapes(n, P, A, W):
    return {k: (n, A) if k == "dst_links" else (n, A, W) if k == "dst_nh" else (n, P)
            for k in SR.KEYS}


def poisoned(n, P, A, W, skew=0):
    """{key: (tensor with GUARD (+ skew for dst_nh) poisoned words in front and
    GUARD behind, first word, shape)}"""
    out = {}
    for k, shp in shapes(n, P, A, W).items():
        first = GUARD + (skew if k == "dst_nh" else 0)
        t = torch.full((first + int(np.prod(shp)) + GUARD,), -1, dtype=torch.int32, device="cuda")
        out[k] = (t, first, shp)
    return out


def ptrs(bufs, keys):
    return {f"d_{k}": bufs[k][0].data_ptr() + 4 * bufs[k][1] for k in keys}


def untouched(bufs, keys=SR.KEYS):
    torch.cuda.synchronize()
    for k in keys:
        assert (bufs[k][0].cpu().numpy().view(np.uint32) == FF).all(), k


def select_dev(sw, table, pref, mnh, flags, W, keys=SR.KEYS, skew=0):
    """select_srmpls_dev into poisoned buffers -> the wanted outputs by node
    id; the guards and the buffers of unwanted outputs must be untouched"""
    off, nodes = R.csr_table(table)
    n, P, A = sw.n_roots, len(table), int(off[-1])
    bufs = poisoned(n, P, A, W, skew)
    torch.cuda.synchronize()
    sw.select_srmpls_dev(off, nodes, PR.flat(pref), PR.flat(mnh),
                         None if flags is None else SR.flat(flags), W, **ptrs(bufs, keys))
    torch.cuda.synchronize()
    untouched(bufs, [k for k in SR.KEYS if k not in keys])
    out = {}
    for k in keys:
        t, first, shp = bufs[k]
        h = t.cpu().numpy().view(np.uint32)
        words = int(np.prod(shp))
        assert (h[:first] == FF).all() and (h[first + words:] == FF).all(), k
        full = np.zeros((sw.engine.V,) + shp[1:], np.uint32)
        full[sw.roots] = h[first:first + words].reshape(shp)
        out[k] = full
    return out


# ---------------------------------------------------------------- every mode
@pytest.mark.parametrize("hop", [False, True])
@pytest.mark.parametrize("kind,seed", [("unit", 0), ("weighted", 1), ("sparse-weighted", 1)])
def test_srmpls_every_sweep_mode(kind, seed, hop):
    names, csr, eng = load(R.graph(kind, seed, 70)[0])
    try:
        assert np.asarray(csr["no_transit"]).any(), "this seed must have drained nodes"
        spf = R.oracle_spf(kind, seed, 70, tuple(names), not hop)
        rng = np.random.default_rng(300 + seed)
        table = R.random_table(70, rng)
        pref, mnh = PR.random_policy(table, rng, classes=2, max_need=4)
        flags = SR.random_flags(table, rng)
        wants, ran = {}, []
        for mode, sw in sweeps(eng, modes_for(kind, hop), hop):
            W = sw.max_nh_words
            if W not in wants:
                wants[W] = SR.expect(spf, names, csr, table, pref, mnh, flags, W, hop)
            want, facts = wants[W]
            assert facts["rule1208_fired"] == 0, facts
            for k in SR.FACTS:
                # a longer parallel link is dropped only where metrics differ and count
                if k != "parallel_dropped" or (kind.endswith("weighted") and not hop):
                    assert facts[k] > 0, (k, facts)
            SR.assert_equal(select_dev(sw, table, pref, mnh, flags, W), want, ctx=(mode, hop))
            ran.append(mode)
        assert "batch" in ran
        # the host-output call: the same arrays in roots order
        sw = Sweep(eng, mode="batch", hop_count=hop)
        try:
            sw.run()
            eng.sync()
            off, nodes = R.csr_table(table)
            got = sw.select_srmpls(off, nodes, PR.flat(pref), PR.flat(mnh), SR.flat(flags))
            want = wants[sw.max_nh_words][0]
            for k in SR.KEYS:
                assert np.array_equal(got[k], want[k][sw.roots]), k
        finally:
            sw.close()
    finally:
        eng.close()


# ---------------------------------------------------------------- kernel paths
class Paths:
    """The 70-node weighted graph, its batch sweep and a pool of 130 prefixes:
    8, 9 and 65 announcers first (kSelShort, kSelShort + 1, more than a wave),
    then select_ref's table and short random ones."""

    def __init__(self):
        self.names, self.csr, self.eng = load(R.graph("weighted", 1, 70)[0])
        self.spf = R.oracle_spf("weighted", 1, 70, tuple(self.names), True)
        rng = np.random.default_rng(17)
        pick = lambda k: sorted(rng.choice(70, size=k, replace=False).tolist())  # noqa: E731
        self.table = [pick(8), pick(9), pick(65)] + R.random_table(70, rng) + \
            [pick(int(k)) for k in rng.integers(1, 13, size=48)]
        assert len(self.table) == 130
        self.pref, self.mnh = PR.random_policy(self.table, rng, classes=2, max_need=3)
        self.flags = SR.random_flags(self.table, rng)
        self.sw = Sweep(self.eng, mode="batch")
        self.sw.run()
        self.eng.sync()
        self._want = {}

    def want(self, P, W):
        if (P, W) not in self._want:
            self._want[P, W] = SR.expect(self.spf, self.names, self.csr, self.table[:P],
                                         self.pref[:P], self.mnh[:P], self.flags[:P], W)[0]
        return self._want[P, W]

    def cols(self, P):
        return self.table[:P], self.pref[:P], self.mnh[:P], self.flags[:P]

    def close(self):
        self.sw.close()
        self.eng.close()


@pytest.fixture(scope="module")
def paths():
    f = Paths()
    yield f
    f.close()


@pytest.mark.parametrize("P", [1, 2, 3, 64, 65, 130])
def test_srmpls_prefix_counts_and_lengths(paths, P):
    """P = 1 / 2 / 3: a prefix of kSelShort, of kSelShort + 1 and of more than
    64 entries alone in their chunk; P = 64, 65, 130: a full chunk, one prefix
    more, several waves."""
    W = paths.sw.max_nh_words
    SR.assert_equal(select_dev(paths.sw, *paths.cols(P), W), paths.want(P, W), ctx=P)


@pytest.mark.parametrize("W,skew", [(1, 0), (3, 0), (4, 0), (4, 1), (5, 0)])
def test_srmpls_output_widths_padding_and_alignment(paths, W, skew):
    """nh_words above the root's words (zero padding), the 16-B store path
    (W = 4) and the same width through a dst_nh pointer one word off 16 B."""
    assert paths.sw.max_nh_words == 1
    SR.assert_equal(select_dev(paths.sw, *paths.cols(65), W, skew=skew), paths.want(65, W),
                    ctx=(W, skew))


def test_srmpls_wide_root():
    """A hub of 150 distinct neighbours (5 words: the lane-per-word path)
    beside spokes of one word; prefixes of 1, 9, 65 and 130 entries and every
    spoke at once."""
    st = hub_stream()
    names, csr, eng = load(st)
    try:
        hub = names.index("hub")
        assert eng.nh_words(hub) == 5  # > kSelLaneW
        V = eng.V
        spf = oracle_of(st, names)
        rng = np.random.default_rng(3)
        table = [[], [hub], [3]] + [sorted(rng.choice(V, size=k, replace=False).tolist())
                                    for k in (9, 65, 130)] + [list(range(1, V)), list(range(V))]
        pref, mnh = PR.random_policy(table, rng, classes=2, max_need=4)
        pref[-2], mnh[-2] = [0] * (V - 1), [0] * (V - 2) + [200]
        flags = SR.random_flags(table, rng)
        flags[-1][hub] = 1  # the hub announces with a prepend label: it routes to the spokes
        ran = 0
        for mode, sw in sweeps(eng, ("batch", "wderive")):
            for W in (5, 8):
                want, facts = SR.expect(spf, names, csr, table, pref, mnh, flags, W)
                assert facts["rule1208_fired"] == 0
                assert want["dst_nh"][hub, :, 4].any(), "the hub's fifth word must be in use"
                SR.assert_equal(select_dev(sw, table, pref, mnh, flags, W), want, ctx=(mode, W))
            ran += 1
        assert ran
    finally:
        eng.close()


# ---------------------------------------------------------------- links
@pytest.mark.parametrize("hop", [False, True])
def test_srmpls_parallel_links_of_unequal_metric(hop):
    dbs = metric_graph([("r", "x", 1, 1), ("r", "x", 1, 1),          # two equal links: 2
                        ("r", "y", 1, 1), ("r", "y", 3, 1),          # unequal: 1, 2 under hop count
                        ("r", "z", 1, 1), ("r", "z", 1, 1, "down"),  # a down link never counts
                        ("x", "t", 1, 1), ("y", "t", 1, 1)])
    st = AdjDbStream.from_dbs(dbs)
    names, csr, eng = load(st)
    try:
        r, t, x, y, z = (names.index(n) for n in "rtxyz")
        spf = oracle_of(st, names, not hop)
        table = [[x], [y], [z], [t], sorted([x, y, z])]
        pref, mnh = PR.uniform_policy(table)
        flags = [[0] * len(a) for a in table]
        want, _ = SR.expect(spf, names, csr, table, pref, mnh, flags, 1, hop)
        off = np.cumsum([0] + [len(a) for a in table])
        assert want["dst_links"][r, off[1]] == (2 if hop else 1)  # y: below its 2 up links
        assert want["links"][r].tolist() == [2, 2 if hop else 1, 1, 4 if hop else 3, 5 if hop else 4]
        ran = 0
        for mode, sw in sweeps(eng, ("wderive", "batch", "derive"), hop):
            SR.assert_equal(select_dev(sw, table, pref, mnh, flags, 1), want, ctx=mode)
            ran += 1
        assert ran
    finally:
        eng.close()


# ---------------------------------------------------------------- want
@pytest.mark.parametrize("keys", [("dst_links",), tuple(k for k in SR.KEYS if k != "dst_nh"),
                                  ("dst_nh",), ("metric", "best")])
def test_srmpls_want_subsets(paths, keys):
    got = select_dev(paths.sw, *paths.cols(65), 1, keys=keys)
    assert sorted(got) == sorted(keys)
    SR.assert_equal(got, paths.want(65, 1), keys)
    off, nodes = R.csr_table(paths.table[:65])
    host = paths.sw.select_srmpls(off, nodes, PR.flat(paths.pref[:65]), PR.flat(paths.mnh[:65]),
                                  SR.flat(paths.flags[:65]), want=keys)
    assert sorted(host) == sorted(keys)
    for k in keys:
        assert np.array_equal(host[k], paths.want(65, 1)[k][paths.sw.roots]), k


def test_srmpls_no_flag_equals_select_policy(paths):
    """All flags 0 (and NULL flags): metric / count / need / best are
    Sweep.select_policy's on the same sweep, the OR of a prefix's dst_nh its
    nh, and links at least its links."""
    table, pref, mnh, _ = paths.cols(130)
    off, nodes = R.csr_table(table)
    pol = paths.sw.select_policy(off, nodes, PR.flat(pref), PR.flat(mnh))
    zero = [[0] * len(a) for a in table]
    for flags in (zero, None):
        got = select_dev(paths.sw, table, pref, mnh, flags, 1)
        for k in ("metric", "count", "need", "best"):
            assert np.array_equal(got[k][paths.sw.roots], pol[k]), k
        assert np.array_equal(SR.or_of_prefixes(got["dst_nh"], table)[paths.sw.roots], pol["nh"])
        assert (got["links"][paths.sw.roots] >= pol["links"]).all()
        assert (got["links"][paths.sw.roots] > pol["links"]).any()


# ---------------------------------------------------------------- contract
def test_srmpls_contract_errors_write_nothing():
    """Every OSPF_E_INVAL (-1) and an injected OSPF_E_DEVICE (-3) leave the
    poisoned outputs untouched; the sweep still answers a good table after."""
    names, csr, eng = load(R.graph("weighted", 1, 70)[0])
    try:
        spf = R.oracle_spf("weighted", 1, 70, tuple(names), True)
        good = [[5, 9, 60], [], [69]]
        gpref, gmnh, gflags = [[1, 0, 1], [], [0]], [[2, 0, 1], [], [0]], [[1, 0, 1], [], [1]]
        off, nodes = R.csr_table(good)
        want, _ = SR.expect(spf, names, csr, good, gpref, gmnh, gflags, 2)
        cols = (off, nodes, PR.flat(gpref), PR.flat(gmnh), SR.flat(gflags))
        sw = Sweep(eng, mode="batch", defer=True)  # no eager run at create
        bufs = poisoned(eng.V, 3, 4, 2)
        # before the first run
        with pytest.raises(EngineError) as ei:
            sw.select_srmpls_dev(*cols, 2, **ptrs(bufs, SR.KEYS))
        assert ei.value.code == -1
        untouched(bufs)
        sw.run()
        eng.sync()

        def still_good():
            SR.assert_equal(select_dev(sw, good, gpref, gmnh, gflags, 2), want)

        still_good()
        bad = [
            (off, nodes, cols[2], cols[3], [1, 2, 0, 1], 2),          # a flag with bit 1 set
            (off, nodes, cols[2], cols[3], [1, 0, 0x80000001, 1], 2),  # and with bit 31
            (off, nodes, cols[2], cols[3], cols[4], 0),               # nh_words too small
            ([0, 3], [9, 5, 60], [0, 0, 0], None, None, 2),           # descending
            ([0, 1], [eng.V], [0], None, [0], 2),                     # id >= V
            ([0, 3], [5, 9, 60], [0, 2 ** 31, 0], None, None, 2),     # a pref >= 2^31
            ([0, 3], [5, 9, 60], None, None, [0, 0, 0], 2),           # no pref
        ]
        for boff, bnodes, bpref, bmnh, bflags, W in bad:
            with pytest.raises(EngineError) as ei:
                sw.select_srmpls_dev(boff, bnodes, bpref, bmnh, bflags, W, **ptrs(bufs, SR.KEYS))
            assert ei.value.code == -1, (bflags, W, ei.value)
            untouched(bufs)
            if W:
                with pytest.raises(EngineError) as ei:
                    sw.select_srmpls(boff, bnodes, bpref, bmnh, bflags, W)
                assert ei.value.code == -1
            still_good()
        for call in (lambda: sw.select_srmpls_dev(*cols, 2, **ptrs(bufs, SR.KEYS)),
                     lambda: sw.select_srmpls(*cols)):
            eng._L.ospf_inject_error(eng._h, 1)
            with pytest.raises(EngineError) as ei:
                call()
            assert ei.value.code == -3
            untouched(bufs)
            still_good()
        r = sw.select_srmpls([0], [], [], [], [])  # no prefix: OSPF_OK, nothing written
        assert r["metric"].shape == (sw.n_roots, 0) and r["dst_nh"].shape[:2] == (sw.n_roots, 0)
        sw.select_srmpls_dev([0], [], [], [], [], 2, **ptrs(bufs, SR.KEYS))
        untouched(bufs)
        # a sweep of an older graph version is stale: the kernel reads the live graph
        drained = int(np.nonzero(np.asarray(csr["no_transit"]))[0][0])
        eng.update_nodes([drained], [0], version=2)
        with pytest.raises(EngineError) as ei:
            sw.select_srmpls_dev(*cols, 2, **ptrs(bufs, SR.KEYS))
        assert ei.value.code == -1
        untouched(bufs)
        sw.close()
    finally:
        eng.close()


# ---------------------------------------------------------------- LinkState
def as_prefixes(names, table, pref, mnh, flags):
    return {f"p{p}": [(names[a],) + CLASS_ATTRS[c] + (m or None, bool(f))
                      for a, c, m, f in zip(ann, pref[p], mnh[p], flags[p])]
            for p, ann in enumerate(table)}


@pytest.mark.parametrize("inject", [0, 1, 4])
def test_linkstate_srmpls_device_and_degraded(paths, inject):
    """On the device (one sweep, no row copied); with an injected device error
    (the load, or the select itself) and degrade on: the same arrays from the
    host path, engine_errors rises."""
    ls = LinkState()
    ls.set_degrade(True)
    ls.apply(R.graph("weighted", 1, 70)[0])
    before = ls.counters()["engine_errors"]
    if inject:
        ls.inject_engine_error(inject)
    got = ls.all_sources_select_srmpls(as_prefixes(paths.names, *paths.cols(65)))
    want = paths.want(65, 1)
    SR.assert_equal(got, want)
    assert np.array_equal(got["installed"], want["installed"])
    c = ls.counters()
    if inject:
        assert c["engine_errors"] == before + 1 and c["engine_degraded"] == 1
    else:
        assert c["engine_errors"] == 0
        assert ls.sweep_stats()["sweeps"] == 1 and ls.sweep_stats()["rows_copied"] == 0


def test_linkstate_srmpls_multi_device_takes_the_host_path(paths):
    ls = LinkState(devices=[0, 0])
    ls.apply(R.graph("weighted", 1, 70)[0])
    got = ls.all_sources_select_srmpls(as_prefixes(paths.names, *paths.cols(65)))
    SR.assert_equal(got, paths.want(65, 1))
    assert ls.counters()["engine_errors"] == 0
