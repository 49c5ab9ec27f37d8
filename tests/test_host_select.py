"""LinkState.all_sources_select on the host path (set_host_spf: no device):
metric, tie count and next-hop mask of every (node, prefix) equal the
reference loop of SpfSolver::getNextHopsWithMetric
(openr/decision/SpfSolver.cpp:1043-1089) applied to the CPU oracle's SPF
results; the mask decoder round-trips; unknown and duplicate announcer names
are dropped."""
import numpy as np
import pytest

import select_ref as R
from openr_amd.linkstate import LinkState, decode_next_hops, encode_next_hops


def host_ls(kind, seed):
    st, _ = R.graph(kind, seed)
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(st)
    return ls


def check(kind, seed, use_link_metric, table_of):
    ls = host_ls(kind, seed)
    names, csr = ls.node_names(), ls.csr()
    spf = R.oracle_spf(kind, seed, 70, tuple(names), use_link_metric)
    table = table_of(names, spf)
    prefixes = {f"p{i}": [names[a] for a in ann] for i, ann in enumerate(table)}
    metric, count, nh = ls.all_sources_select(prefixes, use_link_metric)
    W = nh.shape[2]
    assert W == max(1, max((len(R.root_neighbor_ids(csr, r)) + 31) // 32 for r in range(len(names))))
    em, ec, en = R.expect(spf, names, csr, table, W)
    assert np.array_equal(metric, em)
    assert np.array_equal(count, ec)
    assert np.array_equal(nh, en)
    assert ls.counters()["engine_errors"] == 0
    return ls, names, csr, (metric, count, nh)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("kind", ["unit", "weighted"])
def test_host_select_random_graphs(kind, seed):
    rng = np.random.default_rng(100 + seed)
    for use_link_metric in (True, False):
        check(kind, seed, use_link_metric, lambda names, spf: R.random_table(len(names), rng))


@pytest.mark.parametrize("kind,seed", [("sparse-unit", 0), ("sparse-weighted", 1)])
def test_host_select_unreached_announcers(kind, seed):
    """A prefix announced only by nodes some root does not reach: that root
    gets OSPF_DIST_INF, count 0 and an empty mask."""
    seen = {}

    def table_of(names, spf):
        miss = R.unreached(spf, names)
        assert miss, "this seed must have a root with unreached nodes"
        root = sorted(miss)[0]
        seen["root"] = names.index(root)
        only = [names.index(x) for x in miss[root]]
        return R.random_table(len(names), np.random.default_rng(7), extra=[only])

    _, _, _, (metric, count, nh) = check(kind, seed, True, table_of)
    r = seen["root"]
    assert metric[r, -1] == R.INF and count[r, -1] == 0 and not nh[r, -1].any()


def test_host_select_small_fabric():
    rng = np.random.default_rng(11)
    _, names, _, _ = check("fabric", 3, True, lambda names, spf: R.fabric_table(names, rng))
    assert len(names) == 456


def test_decoder_round_trips():
    ls = host_ls("fabric", 3)
    names, csr = ls.node_names(), ls.csr()
    rng = np.random.default_rng(5)
    for r in rng.choice(len(names), size=24, replace=False).tolist():
        nb = R.root_neighbor_ids(csr, r)
        W = (len(nb) + 31) // 32 + 1  # one zero word of padding
        pick = sorted(rng.choice(len(nb), size=min(len(nb), 5), replace=False).tolist())
        hops = [names[int(nb[k])] for k in pick]
        words = encode_next_hops(csr, names, r, hops, W)
        assert decode_next_hops(csr, names, r, words) == hops
        assert ls.next_hop_names(names[r], words, csr, names) == hops
        assert decode_next_hops(csr, names, r, np.zeros(W, np.uint32)) == []
    with pytest.raises(ValueError):  # a bit beyond the root's neighbours
        r = 0
        nb = R.root_neighbor_ids(csr, r)
        bad = np.zeros((len(nb) + 32) // 32 + 1, np.uint32)
        bad[len(nb) // 32] = np.uint32(1 << (len(nb) % 32))
        decode_next_hops(csr, names, r, bad)


def test_unknown_and_duplicate_names_are_dropped():
    ls = host_ls("unit", 0)
    names = ls.node_names()
    a, b, c = names[3], names[17], names[40]
    clean = {"x": [a, b], "y": [c], "z": []}
    noisy = {"x": [b, "no-such-node", a, b, a], "y": ["ghost", c, c], "z": ["ghost"]}
    want = ls.all_sources_select(clean)
    got = ls.all_sources_select(noisy)
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    # the all-unknown prefix is an empty one: nothing reached anywhere
    assert (got[0][:, 2] == R.INF).all() and not got[1][:, 2].any() and not got[2][:, 2].any()
    # a node announcing the prefix itself: metric 0, one announcer, no next hop
    r = names.index(c)
    assert got[0][r, 1] == 0 and got[1][r, 1] == 1 and not got[2][r, 1].any()
