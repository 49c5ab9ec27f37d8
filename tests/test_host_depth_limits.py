"""The deep ladders of depth_ref.py are what test_gpu_depth_limits.py says they
are (checked on the host against the oracle, so the GPU tests cannot be
vacuous): the engine's depth bound restated over the CSR equals the stated
one, the largest finite distance is the stated one, every ladder root leaves
some node unreached (0x7F level bytes next to deep ones), and the hub has
the stated number of next-hop words."""
import numpy as np
import pytest

import depth_ref as D
from graphs import deep_ladder, depth_bound
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState


@pytest.mark.parametrize("name", list(D.SHAPES))
def test_shape_is_what_it_claims(name):
    bound, max_dist, V, hub_words = D.STATED[name]
    g = D.shape(name)
    assert g.V == V
    assert depth_bound(g.csr) == bound
    S, seed = D.SHAPES[name]["S"], D.SHAPES[name]["seed_stage"]
    assert bound == 2 * max(seed, S - 1 - seed) + 2
    # the seed is the lowest-id transit node; ends and hub are non-transit
    assert g.names[int(np.flatnonzero(g.csr["no_transit"] == 0)[0])] == f"a{seed:03d}"
    for nm in ("e0", "e1") + (("h",) if hub_words else ()):
        assert g.csr["no_transit"][g.ids[nm]] == 1
    far = 0
    ladder = [nm for nm in g.names if nm[0] != "z"]
    for r in ladder:
        res = D.spf(name, r)
        assert len(res) < g.V and not any(nm[0] == "z" for nm in res), r
        assert len(res) == len(ladder), r  # the overloaded nodes are still destinations
        far = max(far, max(e[0] for e in res.values()))
    assert far == max_dist
    assert D.spf(name, "e0")["e1"][0] == S + 1 == max_dist
    # a stage of two twins is two ECMP next hops towards what lies beyond it
    assert len(D.spf(name, "e0")["e1"][1]) == 2
    assert len(D.spf(name, "z0a")) == D.SHAPES[name]["islands"][0]
    if hub_words:
        h = g.ids["h"]
        assert D.words_of(g.csr, h) == hub_words
        assert D.root_neighbor_ids(g.csr, h).size == 2 * D.SHAPES[name]["hub"]
        # the hub shortens nothing: stages 0 and 2 stay 2 apart through stage 1
        assert D.spf(name, "s000a")["s002a"][0] == 2
        assert D.spf(name, "h")["e1"][0] == S - D.SHAPES[name]["hub"] + 2


def test_shapes_cover_both_store_paths():
    assert D.STATED["D122"][2] % 4 != 0 and D.STATED["D122a"][2] % 4 == 0


def test_depth_bound_restatement_small_cases():
    """A path of n transit nodes seeded at its end: ecc = n - 1; seeded in the
    middle by the naming trick; an overloaded seed moves the seed on."""
    def bound(dbs):
        return depth_bound(LinkState(stream=AdjDbStream.from_dbs(dbs)).csr())

    assert bound(deep_ladder(7, 1)) == 2 * 6 + 2
    assert bound(deep_ladder(7, 1, seed_stage=3)) == 2 * 3 + 2
    assert bound(deep_ladder(7, 2, seed_stage=2, ends=True, hub=3, islands=(4,))) == 2 * 4 + 2
    dbs = deep_ladder(7, 2, seed_stage=3)
    next(d for d in dbs if d.name == "a003").overloaded = True
    assert bound(dbs) == 2 * 6 + 2  # s000a seeds now


def test_weighted_ladder_keeps_links_and_hop_counts():
    g, w = D.shape("D122"), D.shape("D122", 5)
    assert np.array_equal(g.csr["col"], w.csr["col"]) and w.csr["metric"].max() == 30
    assert 1 <= w.csr["metric"].min() and len(np.unique(w.csr["metric"])) == 30
    for r in ("e0", "h", "a060", "z0b"):
        hop, unit = D.spf("D122", r, False, 5), D.spf("D122", r)
        assert {k: v[0] for k, v in hop.items()} == {k: v[0] for k, v in unit.items()}, r
