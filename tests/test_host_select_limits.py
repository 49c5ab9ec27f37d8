"""The anycast selection at its chunk and word limits on the host path, and the
expectation test_gpu_select_limits.py uses, proved against the product's own
faces without a GPU: LinkState.all_sources_select (for S3 also
all_sources_select_policy and all_sources_select_srmpls) and track_select /
select_delta / select_tracked with set_host_spf(True). The fixtures and what
makes each a limit case are in select_limits.py; where a fixture names its
judged roots only those are compared. The four models of wrong kernels are
shown to disagree with the expectation on their fixtures."""
import numpy as np
import pytest

import policy_limits as L
import select_limits as S
import seldelta_ref as D
import selpolicy_ref as PR
import srmpls_ref as SR
from openr_amd.linkstate import LinkState

S3_NAMES = [f"S3-{P}" for P in S.S3_SIZES]
# the versions a resident state walks through, per fixture
WALKS = {"S1": (0, 1), "S2": (0, 1, 2, 1, 0), "S4": (0, 1, 2), "S5": (0, 1, 0), "S3-321": (0, 1)}


@pytest.fixture(scope="module")
def cases():
    """every fixture once for the module (select_limits.case keeps them)"""
    return {name: S.case(name) for name in S.CASES}


def host_ls(version):
    ls = LinkState()
    ls.set_host_spf(True)
    ls.apply(version.stream)
    assert ls.node_names() == version.names
    return ls


def rows_of(arrs, roots, keys):
    return {k: arrs[k][roots] for k in keys}


@pytest.mark.parametrize("name", list(S.CASES))
def test_preconditions_hold(cases, name):
    """each fixture is the limit case it claims to be, on the expectation alone"""
    S.preconditions(cases[name])


@pytest.mark.parametrize("name", list(S.CASES))
def test_expectation_is_the_host_path(cases, name):
    """select_ref over the oracle == the product's host selection, in every
    version, so the restatement is not its own witness"""
    c = cases[name]
    roots = c.judged
    for i, v in enumerate(c.versions):
        got = host_ls(v).all_sources_select(S.prefixes_by_name(c))
        W = got[2].shape[2]
        assert W == v.words
        for what, g, w in zip(("metric", "count", "nh"), got, c.exp(W, i)):
            bad = np.argwhere(g[roots] != w[roots])
            assert bad.size == 0, (name, i, what, bad[:5].tolist())


@pytest.mark.parametrize("name", S3_NAMES)
def test_policy_expectations_are_the_host_path(cases, name):
    """S3's policy faces: selpolicy_ref / srmpls_ref == the host selection"""
    c = cases[name]
    roots = c.judged
    keys = PR.KEYS + ("installed",)
    for i, v in enumerate(c.versions):
        got = host_ls(v).all_sources_select_policy(L.policy_prefixes(c))
        PR.assert_equal(rows_of(got, roots, keys), rows_of(c.pol(1, i), roots, keys), keys,
                        ctx=(name, i))
    got = host_ls(c.base).all_sources_select_srmpls(L.srmpls_prefixes(c))
    keys = SR.KEYS + ("installed",)
    SR.assert_equal(rows_of(got, roots, keys), rows_of(c.sr(1)[0], roots, keys), keys, ctx=name)


@pytest.mark.parametrize("name", list(WALKS))
def test_expected_delta_is_the_host_path(cases, name):
    """track_select, then one select_delta per step of the fixture's walk ==
    seldelta_ref.delta on the judged roots, rebased roots included; the
    baseline read back is the expectation after"""
    c = cases[name]
    keep = set(c.judged)
    walk = WALKS[name]
    ls = host_ls(c.versions[walk[0]])
    ls.track_select(S.prefixes_by_name(c))
    for before, after in zip(walk, walk[1:]):
        ls.apply(c.versions[after].stream)
        d = ls.select_delta()
        assert not d["full"]
        W = d["nh"].shape[1]
        assert W == c.versions[after].words
        changed, rebased, ea, _ = c.delta(W, before, after)
        assert changed, (name, before, after)
        assert sorted(set(d["rebased"].tolist()) & keep) == rebased
        got = {k: x for k, x in D.records(d["changes"], d["nh"]).items() if k[0] in keep}
        want = D.wanted(changed, ea)
        assert set(got) == set(want), (name, after, sorted(set(got) ^ set(want))[:8])
        assert got == want
        names = [c.base.names[r] for r in c.judged]
        for g, w in zip(ls.select_tracked(names), ea):
            assert np.array_equal(g, w[c.judged]), (name, after)
    assert ls.counters()["engine_errors"] == 0


# ---------------------------------------------------------------- the wrong kernels
def test_a_signed_minimum_is_told_apart(cases):
    """S1: the minimum over int32 views picks a far announcer wherever a near
    one decides, on both roots and at every prefix length and position; where
    every announcer is far it cannot differ (select_limits' note on S1)"""
    c = cases["S1"]
    em, ec, _ = c.exp(5)
    for r in (c.focus["a"], c.focus["a1"]):
        hit = []
        for p, (kind, n, q) in enumerate(c.plan):
            want = (int(em[r, p]), int(ec[r, p]))
            assert S.min_kernel(c, r, p) == want
            if S.min_kernel(c, r, p, signed=True) != want:
                hit.append(p)
        assert hit == [p for p, (kind, _, _) in enumerate(c.plan) if kind == "mixed"]
        assert {c.plan[p][1] for p in hit} == {8, 9, 65, 130}


def test_a_compare_without_the_last_word_is_told_apart(cases):
    """S2: the first update's record of each hub's own target is missing from
    a compare that stops at word W - 2, for W = 2, 3, 4 and 5"""
    c = cases["S2"]
    changed = c.delta(5, 0, 1)[0]
    blind = S.last_word_blind(c, 5, 0, 1)
    lost = changed - blind
    for hub in S.S2_HUBS:
        assert (c.ids[hub], S.S2_T[hub]) in lost, hub
    # the way back is the same change: it is lost again
    assert {(c.ids[h], S.S2_T[h]) for h in S.S2_HUBS} <= c.delta(5, 1, 0)[0] - S.last_word_blind(c, 5, 1, 0)
    # a change of word 0 is seen by both
    assert {(c.ids[h], S.S2_U[h]) for h in S.S2_HUBS} <= S.last_word_blind(c, 5, 1, 2)


def test_a_neighbour_compare_of_one_trip_is_told_apart(cases):
    """S5: a compare of the first 64 list entries does not rebase the hub"""
    c = cases["S5"]
    vb, va = c.versions
    rebased = c.delta(5)[1]
    short = S.first_64_rebased(vb, va, c.judged)
    assert c.focus["h5"] in rebased and c.focus["h5"] not in short
    assert set(rebased) - set(short) == {c.focus["h5"]}


@pytest.mark.parametrize("name", ["S3-257", "S3-321", "S4"])
def test_waves_of_one_trip_are_told_apart(cases, name):
    """S3 / S4: prefixes 256 and up keep the poison (one-shot) or the stored
    entry (state) when a wave stops after its first chunk"""
    c = cases[name]
    em, ec, _ = c.exp(1)
    assert (S.one_trip(em, S.INF) != em).any() and (S.one_trip(ec, S.INF) != ec).any()
    _, _, ea, eb = c.delta(1)
    stale = S.one_trip(ea[0], eb[0])
    assert (stale != ea[0]).any() and (stale[:, :S.TRIP] == ea[0][:, :S.TRIP]).all()
