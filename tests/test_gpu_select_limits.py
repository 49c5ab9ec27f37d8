"""The anycast selection kernels at their chunk and word limits (select_kernel,
seldelta_kernel and the device functions of spf_select_dev.h; for the launch
shape also policy_kernel, seldelta_policy_kernel and srmpls_kernel): distances
with bit 31 set in the minimum, roots of exactly 2, 3, 4 and 5 next-hop words
with changes in the last word alone, tables that send a wave on a second trip,
the change list's compaction at its edges and under a short capacity, and a
rebase decided at position 128 of a neighbour list.

The fixtures, and the asserts on the expectation that make each a limit case,
are in select_limits.py (select_limits.case runs them before anything is asked
of the engine). Expected values come from select_ref.expect / seldelta_ref.delta
(S3's policy faces: selpolicy_ref, policy_delta_ref, srmpls_ref) over the CPU
oracle's SPF -- never the engine's rows; test_host_select_limits.py proves the
same expectation against the product's host path without a GPU. Every
comparison is exact. Per fixture and admitted sweep mode the one-shot call
writes into poisoned device buffers with guards, then the resident state is
primed, read back, updated and read back again. One engine is alive at a time."""
import numpy as np
import pytest
import torch

import policy_delta_ref as PD
import select_limits as S
import select_ref as R
import seldelta_ref as D
import selpolicy_ref as PR
import srmpls_ref as SR
from openr_amd.engine import EngineError, SelState, SelStateOverflow
from test_gpu_policy_limits import policy_dev
from test_gpu_select_delta import Rig, assert_state, assert_update
from test_gpu_select_srmpls import FF, GUARD, select_dev as srmpls_dev

pytestmark = pytest.mark.gpu

MODES = ("batch", "wderive")
NAMES = ("metric", "count", "nh")


def select_dev(sw, table, W, skew=0):
    """Sweep.select_dev into poisoned buffers (nh `skew` words off 16 B) ->
    (metric, count, nh) by node id; the guards either side must be untouched"""
    off, nodes = R.csr_table(table)
    n, P = sw.n_roots, len(table)
    bufs = {}
    for k in NAMES:
        first = GUARD + (skew if k == "nh" else 0)
        shp = (n, P, W) if k == "nh" else (n, P)
        t = torch.full((first + int(np.prod(shp)) + GUARD,), -1, dtype=torch.int32, device="cuda")
        bufs[k] = (t, first, shp)
    assert (bufs["nh"][0].data_ptr() + 4 * bufs["nh"][1]) % 16 == 4 * skew
    torch.cuda.synchronize()
    sw.select_dev(off, nodes, W, **{f"d_{k}": t.data_ptr() + 4 * first
                                    for k, (t, first, _) in bufs.items()})
    torch.cuda.synchronize()
    out = []
    for k in NAMES:
        t, first, shp = bufs[k]
        h = t.cpu().numpy().view(np.uint32)
        words = int(np.prod(shp))
        assert (h[:first] == FF).all() and (h[first + words:] == FF).all(), (k, W, skew)
        full = np.zeros((sw.engine.V,) + shp[1:], np.uint32)
        full[sw.roots] = h[first:first + words].reshape(shp)
        out.append(full)
    return out


def one_shot(c, sw, W, skew=0, ctx=""):
    """select_kernel at output width W == the expectation on the judged roots"""
    roots = c.judged
    for what, g, w in zip(NAMES, select_dev(sw, c.table, W, skew), c.exp(W)):
        bad = np.argwhere(g[roots] != w[roots])
        assert bad.size == 0, (c.name, ctx, W, skew, what, bad[:5].tolist())


def host_call(c, sw):
    """Sweep.select (host outputs, the sweep's own width)"""
    off, nodes = R.csr_table(c.table)
    W = max(1, sw.max_nh_words)
    got = sw.select(off, nodes)
    for what, g, w in zip(NAMES, got, c.exp(W)):
        assert np.array_equal(g, w[sw.roots]), (c.name, what)


def run_fixture(c, widths, steps, modes=MODES, extra=None):
    """Per admitted sweep mode: select_dev at every (width, skew), then the
    resident state primed, read back and walked through `steps` (before,
    after, nh_words of the read), each update against seldelta_ref.delta with
    its records' words and the state read back. extra(sw) runs on the first
    sweep. EngineError -4 at sweep creation skips the mode; batch must run."""
    S.preconditions(c)
    off, nodes = R.csr_table(c.table)
    W0 = c.base.words
    # sampled roots: the other roots' records are counted too, and not judged
    cap = None if c.roots is None else c.base.V * len(c.table)
    ran = []
    for mode in modes:
        rig, st = Rig(mode), None
        try:
            sw = rig.sweep(c.base)
            if sw is None:
                continue
            assert max(1, sw.max_nh_words) == W0
            for W, skew in widths:
                one_shot(c, sw, W, skew, ctx=mode)
            if extra:
                extra(sw)
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            assert_state(st, c.exp(W0), W0, c.roots, what=(c.name, mode, "prime"))
            for before, after, W in steps:
                sw = rig.sweep(c.versions[after])
                assert sw is not None, (mode, after)
                changed, _ = assert_update(st, sw, c.versions[before], c.versions[after], c.table,
                                           W, False, roots=c.roots, cap=cap,
                                           what=(c.name, mode, after))
                assert changed == c.delta(W, before, after)[0] and changed
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    print(f"{c.name}: sweep modes {ran}")
    assert "batch" in ran, ran
    return ran


# ---------------------------------------------------------------- S1
def test_distances_with_bit_31_in_the_anycast_minimum():
    """prefix_min / wave_min, the `d < m` walk and the `dist[id] == m` count
    with distances of 0x80000005 and above, on the lane-per-word path (root a,
    131 neighbours) and the lane paths (a1), at prefixes of 8, 9, 65 and 130
    announcers with the deciding one at position 0, 63, 64 and beyond, a tie
    on both trips, an unreached announcer in the lanes. Catches: `min` on the
    shuffled int in wave_min, a signed `d < m` or `min(m, dist)` (the mixed
    prefixes: a far announcer wins over the near one), a distance with bit 31
    taken for unreached (the far prefixes and the tie's count). The update
    moves every far distance from one value of at least 2^31 to the next."""
    c = S.case("S1")
    ran = run_fixture(c, widths=((5, 0), (8, 0)), steps=((0, 1, 5), (1, 0, 8)))
    assert ran, "no sweep mode admits the 0x7FFFFFFF metric"


# ---------------------------------------------------------------- S2
def test_roots_of_2_3_4_and_5_words_and_changes_in_one_word():
    """Hubs of 64, 96, 128 and 129 neighbours: the largest of W = 2, 3, 4 and
    the smallest of 5. Catches: a word dropped by the cooperative [n][W] store
    (4 trips at W = 4) or by select_kernel's scalar (Wout = 5, 6, skewed 8)
    and 16-B (Wout = 8) stores, `w < W - 1` in the lane's `ow[w] != acc[w]`
    or in the lane-per-word compare (the first update takes the top bit of
    each hub's word W - 1 off its target's entry and leaves metric, count and
    the other words alone: nothing else reports it), a compare that starts at
    word 1 (the second update changes word 0 alone), a chg_nh record short of
    a word at nh_words 5 and 8 -- and a five-word root on the four-word path.
    The targets' prefixes sit in lanes 0 and 63 of the first chunk and lane 0
    of the second."""
    c = S.case("S2")

    def extra(sw):
        for hub, n in S.S2_HUBS.items():
            assert sw.engine.nh_words(c.ids[hub]) == int(hub[1])

    run_fixture(c, widths=((5, 0), (6, 0), (8, 0), (8, 1)),
                steps=((0, 1, 5), (1, 2, 8), (2, 1, 5), (1, 0, 8)), extra=extra)


# ---------------------------------------------------------------- S3
@pytest.mark.parametrize("P", S.S3_SIZES)
def test_tables_across_the_waves_trips(P):
    """P = 64, 65, 256, 257, 321: one wave, a second wave of one prefix, four
    full waves, wave 0's second trip of one prefix, wave 1's. Catches: `base
    += 64` or a stride of the launch's wave count taken wrong in select_kernel
    / seldelta_kernel (prefixes 256 and up keep the poison, or the stored
    entry), `n = min(64, P - base)` wrong on a partial second trip, a change
    list without the second trip's entries."""
    c = S.case(f"S3-{P}")
    widths = ((1, 0), (4, 0), (3, 1)) if P == 321 else ((1, 0),)
    run_fixture(c, widths=widths, steps=((0, 1, 1),), extra=lambda sw: host_call(c, sw))


def policy_update(st, sw, c, before, after, ctx):
    """one update_policy == the expected policy delta (all roots judged)"""
    changed, rebased, ea, _ = c.pdelta(1, before, after)
    rec, nh, reb = st.update_policy(sw, cap=len(changed), cap_rebased=4, nh_words=1)
    assert sorted(reb.tolist()) == rebased == [], ctx
    got, want = PD.records(rec, nh), PD.wanted(changed, ea)
    assert set(got) == set(want), (ctx, sorted(set(got) ^ set(want))[:8])
    assert got == want, ctx
    PD.assert_state(st, ea, 1, what=ctx)


@pytest.mark.parametrize("P", S.S3_SIZES)
def test_tables_across_the_waves_trips_policy_faces(P):
    """The same tables through the kernels that copy the launch shape:
    policy_kernel under a random two-class policy, srmpls_kernel with random
    prepend flags (on a second trip the entries of one wave's chunks are no
    longer one contiguous range of dst_links / dst_nh), and a policy state
    primed and updated (seldelta_policy_kernel)."""
    c = S.case(f"S3-{P}")
    off, nodes = R.csr_table(c.table)
    ran = []
    for mode in MODES:
        rig, st = Rig(mode), None
        try:
            sw = rig.sweep(c.base)
            if sw is None:
                continue
            PR.assert_equal(policy_dev(sw, c, 1), c.pol(1), ctx=(c.name, mode))
            got = srmpls_dev(sw, c.table, c.pref, c.mnh, c.flags, 1)
            SR.assert_equal(got, c.sr(1)[0], ctx=(c.name, mode))
            st = SelState(rig.eng, off, nodes, PR.flat(c.pref), PR.flat(c.mnh))
            st.prime(sw)
            PD.assert_state(st, c.pol(1), 1, what=(c.name, mode, "prime"))
            sw = rig.sweep(c.versions[1])
            assert sw is not None
            policy_update(st, sw, c, 0, 1, (c.name, mode))
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    assert "batch" in ran, ran


# ---------------------------------------------------------------- S4
def overflow_then_exact(st, sw, c, W, before, after, cap_short, ctx):
    """The update with a capacity below the count raises SelStateOverflow,
    reports the whole count and leaves the state as it was; with the exact
    capacity it then succeeds, its record set and the state exact."""
    changed, rebased, ea, eb = c.delta(W, before, after)
    assert c.roots is None and 0 <= cap_short < len(changed) and not rebased
    with pytest.raises(EngineError) as ei:
        st.update(sw, cap=cap_short, cap_rebased=0, nh_words=W)
    assert isinstance(ei.value, SelStateOverflow) and ei.value.code == -4, ctx
    assert ei.value.n_changes == len(changed) and ei.value.n_rebased == 0, ctx
    assert_state(st, eb, W, what=(ctx, "after the overflow"))
    rec, nh, reb = st.update(sw, cap=len(changed), cap_rebased=0, nh_words=W)
    assert len(rec) == len(changed) and len(reb) == 0, ctx
    got, want = D.records(rec, nh), D.wanted(changed, ea)
    assert set(got) == set(want), (ctx, sorted(set(got) ^ set(want))[:8])
    assert got == want, ctx
    assert_state(st, ea, W, what=ctx)


def test_compaction_edges_and_capacity_one_short():
    """The ballot / popcount prefix of the change list at P = 321. First every
    prefix of root r changes: five chunks whose 64 lanes all changed (the mask
    all ones, lane 63's prefix mask (1 << 63) - 1) and one of a single lane.
    Then, for every root but the leaves, exactly the prefixes at 0, 63, 64,
    255, 256 and 320: a lone change in lane 0 or lane 63, on both trips.
    Catches: `1ull << lane` as a 32-bit shift, a prefix mask that includes the
    lane itself, the leader's base not broadcast, a record at `idx == cap`
    written or one below it dropped, a count that stops at the capacity, a
    state committed in spite of the overflow."""
    c = S.case("S4")
    off, nodes = R.csr_table(c.table)
    ran = []
    for mode in MODES:
        rig, st = Rig(mode), None
        try:
            sw = rig.sweep(c.base)
            if sw is None:
                continue
            one_shot(c, sw, 1, ctx=mode)
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            assert_state(st, c.exp(1), 1, what=(mode, "prime"))
            for before, after in ((0, 1), (1, 2)):
                sw = rig.sweep(c.versions[after])
                assert sw is not None
                n = len(c.delta(1, before, after)[0])
                overflow_then_exact(st, sw, c, 1, before, after, n - 1, (mode, after))
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    assert "batch" in ran, ran


@pytest.mark.parametrize("nh_words", [5, 8])
def test_capacity_among_a_wide_roots_records(nh_words):
    """S2's first update with the words wanted and a capacity that falls among
    the records of the 129-neighbour hub (the entries of every other root plus
    one): the by-wave record writer's `ij >= cap` skip. Catches: the skip
    tested on the wave's first index only, words written past the list's end,
    a count or a state that depends on what fitted."""
    c = S.case("S2")
    off, nodes = R.csr_table(c.table)
    changed = c.delta(nh_words, 0, 1)[0]
    mine = S.changed_of(changed, c.ids["h5"])
    assert len(mine) >= 3
    rig, st = Rig("batch"), None
    try:
        sw = rig.sweep(c.base)
        assert sw is not None
        st = SelState(rig.eng, off, nodes)
        st.prime(sw)
        sw = rig.sweep(c.versions[1])
        overflow_then_exact(st, sw, c, nh_words, 0, 1, len(changed) - len(mine) + 1, nh_words)
    finally:
        if st is not None:
            st.close()
        rig.close()


# ---------------------------------------------------------------- S5
def test_rebase_decided_on_the_second_trip_of_the_list_compare():
    """The 129-neighbour hub swaps its last neighbour for a node of a higher
    id: count and width stay, the lists differ at position 128 alone. Catches:
    `k < 64` or a missing `k += 64` in the neighbour compare, a verdict taken
    from lane 0 instead of the ballot -- the hub would not be rebased and its
    entries, whose bit 128 now means another neighbour, would be compared (or
    not reported at all). The rebased list is cut one short, then exact."""
    c = S.case("S5")
    off, nodes = R.csr_table(c.table)
    h5 = c.focus["h5"]
    changed, rebased, ea, eb = c.delta(5)
    V, P = c.base.V, len(c.table)
    ran = []
    for mode in MODES:
        rig, st = Rig(mode), None
        try:
            sw = rig.sweep(c.base)
            if sw is None:
                continue
            one_shot(c, sw, 5, ctx=mode)
            st = SelState(rig.eng, off, nodes)
            st.prime(sw)
            assert_state(st, eb, 5, c.roots, what=(mode, "prime"))
            sw = rig.sweep(c.versions[1])
            assert sw is not None and sw.engine.nh_words(h5) == 5
            with pytest.raises(EngineError) as ei:
                st.update(sw, cap=V * P, cap_rebased=len(rebased) - 1, nh_words=5)
            assert isinstance(ei.value, SelStateOverflow) and ei.value.code == -4
            assert ei.value.n_rebased == len(rebased) == 3
            assert_state(st, eb, 5, c.roots, what=(mode, "after the overflow"))
            rec, nh, reb = st.update(sw, cap=V * P, cap_rebased=len(rebased), nh_words=5)
            assert sorted(reb.tolist()) == rebased and h5 in rebased
            assert not np.isin(rec["root"], rebased).any()  # no record names a rebased root
            keep = np.isin(rec["root"], c.judged)
            assert D.records(rec[keep], nh[keep]) == D.wanted(changed, ea)
            assert_state(st, ea, 5, c.roots, what=(mode, "update"))
            # and back: the same three roots again
            sw = rig.sweep(c.base)
            assert sw is not None
            assert_update(st, sw, c.versions[1], c.base, c.table, 5, False, roots=c.roots,
                          cap=V * P, what=(mode, "back"))
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    assert "batch" in ran, ran
