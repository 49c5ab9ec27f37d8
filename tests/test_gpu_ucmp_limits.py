"""The UCMP kernels (spf_ucmp.hip) at their weight and width limits: the device
against ucmp_ref's / ucmp_policy_ref's recursion in Python integers, which
test_host_ucmp_limits.py proves against the CPU oracle wherever no value
leaves i63 (beyond that the oracle is undefined and the recursion alone is
the expectation).

Every case primes a SelState, resolves both algorithms and compares all four
outputs of ucmp_copy (advertised, status, off, wt) exactly, and the round
count with the recursion's depth. The fixtures (test_host_ucmp_limits.py) are
explicit graphs; each asserts on the recursion what it exists for: I63 = 2^63
- 1 inclusive, products whose high word alone shows the overflow, a sum that
overflows and then takes more, VOID before OVERFLOW in both slot orders, the
link weight sums of 'adj', the gcd at large operands, and the root widths of
4, 5 and 66 next-hop words."""
import numpy as np
import pytest

import select_ref as R
import ucmp_policy_ref as UP
import ucmp_ref as U
from openr_amd.adjdb import AdjDbStream
from openr_amd.engine import SelState
from test_gpu_select_delta import Rig
from test_gpu_select_policy import hub_stream
from test_gpu_ucmp_all import assert_view, flat
from test_gpu_ucmp_policy import device_case as policy_device_case
from test_host_ucmp_all import assert_linkstate, tracked
from test_host_ucmp_limits import (A62, I63, SUMS, Fixture, L, assert_exact, assert_hub, assert_mixed,
                                   assert_policy, assert_product, assert_star, assert_sums,
                                   exact_fixture, hub_fixture, hub_roots, mixed_fixture,
                                   policy_fixture, product_fixture, star_fixture, star_roots)
from test_host_ucmp_policy import PolicyCase

pytestmark = pytest.mark.gpu


def run_case(fx, hop=False, look=None, need=None, sums=(None,), modes=("batch",)):
    """prime + both algorithms in every mode; `look`: the roots copied and
    compared (None: all), `need`: the roots the recursion is restricted to,
    `sums`: S overrides, each resolved over the one primed state.
    -> [(consts, selection, {algo: recursion})] per override"""
    exps = [fx.expectation(hop, need, s) for s in sums]
    off, nodes = R.csr_table(fx.table)
    roots = list(range(fx.version.V)) if look is None else list(look)
    for mode in modes:
        rig = Rig(mode, hop)
        st = None
        try:
            if rig.sweep(fx.version) is None:  # a mode that does not take the graph
                assert mode != "batch"
                continue
            st = SelState(rig.eng, off, nodes)
            st.prime(rig.sw)
            for consts, sel, exp in exps:
                assert st.ucmp_slots == len(consts.dn)
                for algo in U.ALGOS:
                    rounds = st.ucmp(algo, flat(fx.leaf_w), consts.S)
                    assert rounds == exp[algo][2], (mode, algo)
                    assert_view(st, sel, consts, exp[algo], roots, (mode, algo))
        finally:
            if st is not None:
                st.close()
            rig.close()
    return exps


# ---------------------------------------------------------------- the lane path
def test_exact_leaf_exact_sum_and_gcd():
    """I63 as a leaf and as a sum stays OK and is copied word for word; the
    view divides I63 by itself, (2^62, 2^61) by 2^61, and leaves two large
    coprime weights as they are; one more than I63 is OVERFLOW and reads 0."""
    fx = exact_fixture()
    (consts, sel, exp), = run_case(fx, modes=("batch", "wderive"))
    assert_exact(fx, consts, sel, exp)


def test_link_weight_sums_at_the_limit():
    """'adj' over S given to the call: 2^62 + 2^62 is OVERFLOW, 2^62 - 1 +
    2^62 and a single slot of I63 are OK with I63, I63 + 1 is OVERFLOW."""
    fx = exact_fixture()
    exps = run_case(fx, sums=[s for s, _ in SUMS])
    for (_, _, exp), (_, want) in zip(exps, SUMS):
        assert_sums(fx, exp, want)


@pytest.mark.parametrize("hop", [False, True])
def test_products_that_leave_i63(hop):
    """c * W with c = 2, 3, 4 tight links: 2 * I63 (the low word shows it),
    3 * I63 (only the high word does: the low word is 2^63 - 3) and 4 * 2^62
    (the low word is 0). A dearer parallel link counts under hop count only."""
    fx = product_fixture()
    (consts, sel, exp), = run_case(fx, hop)
    assert_product(fx, consts, exp, hop)


def test_overflow_then_more_and_void_over_overflow():
    fx = mixed_fixture()
    (consts, sel, exp), = run_case(fx)
    assert_mixed(fx, consts, sel, exp)


# ---------------------------------------------------------------- 4 and 5 words
@pytest.mark.parametrize("N", [127, 128, 129])
def test_hub_at_the_lane_and_wave_widths(N):
    """The hub's 4 words (N = 127, the lane path's last width) and 5 words (the
    wave path: a lane per word). The exact sum over every word is OK, one more
    is OVERFLOW; two lanes' 2^62 overflow where no other lane sees it; a zero
    weight in one word and an overflow in others is VOID."""
    fx = hub_fixture(N)
    (consts, sel, exp), = run_case(fx, look=hub_roots(fx, N))
    assert_hub(fx, consts, sel, exp, N)


# ---------------------------------------------------------------- more than 64 words
def test_star_of_66_words():
    """a lane of the wave path takes two words (x += 64): next hops in words 0,
    63, 64 and 65"""
    fx = star_fixture()
    look, need = star_roots(fx)
    (consts, sel, exp), = run_case(fx, look=look, need=need)
    assert_star(fx, consts, sel, exp)


# ---------------------------------------------------------------- policy states
def test_policy_drained_leaves_at_the_limit():
    case, ids = policy_fixture()
    sel, consts, exp = policy_device_case(case)
    assert_policy(case, ids, sel, consts, exp)


def policy_hub_case():
    """hub_stream()'s hub of 5 words with the drained spokes s007 and s090 as
    announcers; the hub reaches each directly and through its ring neighbour
    (s006, s089), so their weights meet in words 0 and 2 of the hub's mask."""
    dbs = hub_stream().to_dbs()
    names = sorted(d.name for d in dbs)
    d0, d1 = names.index("s007"), names.index("s090")
    table = [[d0], [d0], [d0, d1], [d1], [d0, 20, 60, d1], [d0, d1]]
    leaf_w = [[A62], [A62 - 1], [A62, 0], [I63], [A62, 3, 4, A62], [(1 << 61) - 1, (1 << 61) - 1]]
    case = PolicyCase(dbs, table, [[0] * len(a) for a in table], leaf_w)
    assert case.names == names and case.W == 5 and case.drained[d0] and case.drained[d1]
    return case


def test_policy_hub_with_drained_spokes_at_the_limit():
    case = policy_hub_case()
    hub, d0, d1 = (case.names.index(n) for n in ("hub", "s007", "s090"))
    sel, consts, exp = policy_device_case(case)
    res = exp["prefix"]
    lo = int(consts.dn_off[hub])
    hops = [int(consts.dn[lo + b]) for b in U.bits(sel["nh"][hub, 5])]
    assert hops == [d0 - 1, d0, d1 - 1, d1]  # the drained spokes and their ring neighbours
    assert {b // 32 for b in U.bits(sel["nh"][hub, 5])} == {0, 2}
    at = lambda p: (int(res[1][hub, p]), int(res[0][hub, p]))  # noqa: E731
    assert at(0) == (U.OVERFLOW, 0)  # 2^62 from the drained leaf and 2^62 through s006
    assert at(1) == (U.OK, I63 - 1)
    assert at(2) == (U.VOID, 0) and at(3) == (U.OVERFLOW, 0)
    assert at(4)[0] == U.OK and at(4)[1] < 100  # the drained announcers lose to the others
    assert at(5) == (U.OK, I63 - 3)  # four times 2^61 - 1 across two lanes
    mine = UP.links(sel, consts, res, hub, 1, case.table, case.leaf_w, case.drained)
    assert mine == [(d0 - 1, 1, 1), (d0, 1, 1)]


# ---------------------------------------------------------------- LinkState
def test_linkstate_exact_limits_by_name():
    """all_sources_ucmp / ucmp_tracked by node names on the device: the
    recursion's result, and the host loop's for the same nodes (no entry of
    this table leaves i63, under either algorithm)."""
    fx = exact_fixture(overflow=False)
    case = fx.case()
    ls = tracked(case, True, host=False)
    for algo in U.ALGOS:
        res = assert_linkstate(ls, case, True, algo)
        assert ls.ucmp_info["device"] and ls.ucmp_info["rounds"] == res[2] == 3
        assert (res[1] == U.OK).all() and int(res[0][fx.ids["s"], 1]) == I63
        for g, w in zip(ls.ucmp_host_loop(case.leaf_w, algo, case.names), ls.ucmp_tracked(case.names)):
            assert np.array_equal(g, w), algo
    c = ls.counters()
    assert c["engine_errors"] == 0 and c["engine_degraded"] == 0


def pair_fixture(w):
    """t - h = g - w0 with two tight parallel links h = g, each of weight `w`
    from g; t - c - d beside them. t announces."""
    links = L("t", "h") + L("g", "h", 2, wa=w) + L("g", "w0") + L("t", "c") + L("c", "d")
    return Fixture(links, [{"t": 6}, {"d": 4, "h": 9}])


def test_linkstate_link_weights_beyond_the_engine_contract():
    """Two tight parallel links of weight 2^62 from g to h: S(g, h) = 2^63 is
    no i64. That call is the host loop's (which adds as the reference does: g
    and w0, whose walks use the pair, are not asserted); it is no engine error
    and degrades nothing. With the weights lowered the same LinkState runs on
    the device again. A negative link weight is treated alike."""
    fx = pair_fixture(A62)
    case = fx.case()
    ls = tracked(case, True, host=False)
    consts, sel, exp = fx.expectation()
    assert consts.S[consts.slot(fx.ids["g"], fx.ids["h"])] == 1 << 63
    res = exp["adj"]
    assert fx.at(res, "g", 0)[0] == U.OVERFLOW and fx.at(res, "w0", 0)[0] == U.OVERFLOW
    clear = [fx.ids[nm] for nm in ("t", "h", "c", "d")]
    assert (res[1][clear] == U.OK).all()

    def clean():
        c = ls.counters()
        assert c["engine_errors"] == 0 and c["engine_degraded"] == 0

    weight, status = ls.all_sources_ucmp(case.leaf_w, "adj")
    assert not ls.ucmp_info["device"]
    clean()
    assert np.array_equal(status[clear], res[1][clear]) and np.array_equal(weight[clear], res[0][clear])
    want = U.copy_expect(sel, consts, res, clear)
    for g, w in zip(ls.ucmp_tracked([case.names[i] for i in clear]), want):
        assert np.array_equal(g, w)
    for w in (-1, 3):  # a negative weight: the host loop again; 3: the device
        low = pair_fixture(w)
        ls.apply(AdjDbStream.from_dbs(low.version.dbs))
        ls.select_delta()
        if w < 0:
            ls.all_sources_ucmp(case.leaf_w, "adj")
            assert not ls.ucmp_info["device"]
            clean()
    moved = low.case()
    for algo in U.ALGOS:
        assert_linkstate(ls, moved, True, algo)
        assert ls.ucmp_info["device"]
    clean()
