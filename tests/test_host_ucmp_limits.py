"""The UCMP recursion (ucmp_ref, ucmp_policy_ref) at the weight limits, proved
against the CPU oracle's resolveUcmpWeights root by root -- no device, no
engine code. The fixtures here are shared with test_gpu_ucmp_limits.py, which
runs the device against the same recursion.

I63 = 2^63 - 1 is the largest weight an entry holds: a leaf, a sum or a product
equal to it stays OK and is carried word for word; one more is OVERFLOW. The
oracle (like the reference it restates) adds into a signed 64-bit integer, so
beyond i63 it is undefined: for the entries the recursion marks OVERFLOW
nothing is compared with the oracle, here or anywhere. Every other entry of
every fixture is compared, under both algorithms: the advertised weight and the
normalised per-link weights. The oracle's text protocol carries I63 as it is
(decimal in, decimal out), so no smaller stand-in is needed.

Every graph is built from explicit links of metric 1 (one dearer parallel
link excepted, which is the point of that fixture): equidistance is a property
of the fixture, not of a seed. Each test asserts the literal statuses and
values its fixture exists for."""
import numpy as np
import pytest

import seldelta_ref as D
import ucmp_policy_ref as UP
import ucmp_ref as U
from openr_amd.adjdb import AdjDb, create_adjacency
from openr_amd.linkstate import LinkState
from test_host_ucmp_all import Case
from test_host_ucmp_policy import PolicyCase

I63 = U.I63
A62 = 1 << 62
POOL = (2, 3, 4, 6, 9, 10)


def named_dbs(links, over=()):
    """links: (a, b, metric a->b, metric b->a, weight a, weight b)"""
    names = sorted({x for l in links for x in l[:2]})
    adjs = {nm: [] for nm in names}
    for i, (a, b, ma, mb, wa, wb) in enumerate(links):
        adjs[a].append(create_adjacency(b, f"{a}-{b}-{i}", f"{b}-{a}-{i}", ma, weight=wa))
        adjs[b].append(create_adjacency(a, f"{b}-{a}-{i}", f"{a}-{b}-{i}", mb, weight=wb))
    return [AdjDb(nm, adjs[nm], i + 1, overloaded=nm in over) for i, nm in enumerate(names)]


def L(a, b, n=1, m=1, wa=1, wb=1):
    """n parallel links a - b of metric m"""
    return [(a, b, m, m, wa, wb)] * n


class Fixture:
    """An explicit graph and a weighted prefix table given by node names:
    prefixes = [{announcer name: leaf weight}]."""

    def __init__(self, links, prefixes, over=()):
        self.version = v = D.Version(named_dbs(links, over))
        self.ids = {nm: i for i, nm in enumerate(v.names)}
        self.table, self.leaf_w = [], []
        for pf in prefixes:
            ann = sorted((self.ids[nm], w) for nm, w in pf.items())
            self.table.append([a for a, _ in ann])
            self.leaf_w.append([w for _, w in ann])
        ls = LinkState()
        ls.set_host_spf(True)
        ls.apply(v.stream)
        self.keys = ls.link_keys()

    def expectation(self, hop=False, roots=None, sums=None):
        """-> consts, selection, {algo: recursion}. sums = {(node name,
        neighbour name): S} overrides the link weight sums ('adj')."""
        v = self.version
        consts = U.Consts(v.csr, v.names, v.dbs, self.keys, not hop)
        if sums:
            consts = consts.with_S({(self.ids[a], self.ids[b]): s for (a, b), s in sums.items()})
        sel = v.expect(self.table, v.words, not hop, roots)
        return consts, sel, {algo: U.resolve(sel, consts, self.table, self.leaf_w, algo)
                             for algo in U.ALGOS}

    def at(self, res, name, p):
        """(status, advertised weight) of node `name` for prefix p"""
        return int(res[1][self.ids[name], p]), int(res[0][self.ids[name], p])

    def view(self, consts, sel, res, name, p):
        """[(next hop name, normalised weight)] of node `name`, in slot order"""
        return [(self.version.names[k], w) for k, _, w in U.links(sel, consts, res, self.ids[name], p)]

    def case(self):
        """test_host_ucmp_all.Case over this fixture (assert_linkstate, tracked)"""
        v = self.version
        c = Case.__new__(Case)
        c.dbs, c.stream, c.names, c.csr, c.keys, c.V = v.dbs, v.stream, v.names, v.csr, self.keys, v.V
        c.table, c.leaf_w, c.W = self.table, self.leaf_w, v.words
        from oracle import Oracle
        c.orc = Oracle(v.stream)
        return c


# ---------------------------------------------------------------- the fixtures
def exact_fixture(overflow=True):
    """t - a - s - r by single links, t1 and t2 next to s.
    p0 the exact leaf, p1 the exact sum of two coprime weights, p2 the pair
    (2^62, 2^61), p3 another exact sum; with `overflow` p4 / p5, one more than
    I63. The link weights reach the same limits under 'adj': a's link to t
    carries I63, s's links to t1 and t2 carry 2^62 and 2^62 - 1."""
    links = L("t", "a", wb=I63) + L("a", "s") + L("t1", "s", wb=A62) + L("t2", "s", wb=A62 - 1)
    links += L("s", "r")
    over = [{"t1": A62, "t2": A62}, {"t1": I63, "t2": 1}] if overflow else []
    return Fixture(links, [{"t": I63}, {"t1": A62, "t2": A62 - 1}, {"t1": A62, "t2": 1 << 61},
                           {"t1": I63 - 1, "t2": 1}] + over)


def assert_exact(fx, consts, sel, exp):
    P = len(fx.table)
    for algo in U.ALGOS:
        res = exp[algo]
        assert fx.at(res, "t", 0) == (U.OK, I63) and fx.at(res, "a", 0) == (U.OK, I63), algo
        assert fx.view(consts, sel, res, "a", 0) == [("t", 1)]  # I63 / gcd = 1
    res = exp["prefix"]
    assert [fx.at(res, nm, 0) for nm in ("s", "r", "t1", "t2")] == [(U.OK, I63)] * 4
    assert fx.view(consts, sel, res, "r", 0) == [("s", 1)]
    for p in (1, 3):
        assert [fx.at(res, nm, p) for nm in ("s", "r", "a", "t")] == [(U.OK, I63)] * 4
    assert fx.view(consts, sel, res, "s", 1) == [("t1", A62), ("t2", A62 - 1)]  # coprime: as they are
    assert fx.at(res, "s", 2) == (U.OK, 3 << 61)
    assert fx.view(consts, sel, res, "s", 2) == [("t1", 2), ("t2", 1)]
    for p in range(4, P):
        assert [fx.at(res, nm, p) for nm in ("s", "r", "a", "t")] == [(U.OVERFLOW, 0)] * 4
        assert fx.at(res, "t1", p)[0] == U.OK and fx.at(res, "t2", p)[0] == U.OK
    res = exp["adj"]  # the link weight sums: S(s, t1) + S(s, t2) = I63, S(a, t) = I63
    assert [fx.at(res, nm, 0) for nm in ("s", "r", "t1", "t2")] == [(U.OK, 1)] * 4
    for p in (1, 2, 3):
        assert fx.at(res, "s", p) == (U.OK, I63) and fx.at(res, "r", p) == (U.OK, 1)
    assert (res[1] == U.OK).all()
    assert exp["prefix"][2] == 3 and exp["adj"][2] == 3


def product_fixture():
    """s announces; q1 / q2 / q4 behind it by two / three / four tight parallel
    links, a node behind each; e behind s by one link of metric 1 and one of
    metric 2 (c = 1 under link metrics, 2 under hop count), f behind e."""
    links = L("s", "q1", 2) + L("s", "q2", 3) + L("s", "q4", 4)
    links += L("q1", "b1") + L("q2", "b2") + L("q4", "b4")
    links += L("s", "e") + L("s", "e", m=2) + L("e", "f")
    return Fixture(links, [{"s": I63}, {"s": A62}, {"s": 5}])


def assert_product(fx, consts, exp, hop):
    res = exp["prefix"]
    ovf = (U.OVERFLOW, 0)
    for p in (0, 1):  # 2 * I63: high word 0; 3 * I63: high word 1, low word <= I63; 4 * 2^62: low word 0
        for nm in ("q1", "q2", "q4", "b1", "b2", "b4"):
            assert fx.at(res, nm, p) == ovf, (nm, p)
    assert [fx.at(res, nm, 2)[1] for nm in ("q1", "q2", "q4", "b4")] == [10, 15, 20, 20]
    assert int(consts.c[consts.slot(fx.ids["e"], fx.ids["s"])]) == (2 if hop else 1)
    want = [ovf, ovf, (U.OK, 10)] if hop else [(U.OK, I63), (U.OK, A62), (U.OK, 5)]
    assert [fx.at(res, "e", p) for p in range(3)] == want  # the dearer link counts under hop count only
    assert [fx.at(res, "f", p) for p in range(3)] == want
    assert (exp["adj"][1] == U.OK).all()


def mixed_fixture():
    """n with the next hops x1, x2, x3 in that slot order (m behind n): sums
    that overflow and then take more, in every order, and one exact sum.
    v1 with an OVERFLOW next hop (h1, two links to u1) in the slot before a
    VOID one (k1, before the zero-weight leaf z1); v2 the mirror image: the
    VOID next hop h2 first, the OVERFLOW next hop k2 second. w1 behind v1."""
    links = L("n", "x1") + L("n", "x2") + L("n", "x3") + L("m", "n")
    links += L("v1", "h1") + L("h1", "u1", 2) + L("v1", "k1") + L("k1", "z1") + L("w1", "v1")
    links += L("v2", "h2") + L("h2", "z2") + L("v2", "k2") + L("k2", "u2", 2)
    return Fixture(links, [{"x1": A62, "x2": A62, "x3": 5}, {"x1": 5, "x2": A62, "x3": A62},
                           {"x1": A62, "x2": 5, "x3": A62}, {"x1": A62, "x2": A62 - 6, "x3": 5},
                           {"u1": I63, "z1": 0, "u2": I63, "z2": 0}])


def assert_mixed(fx, consts, sel, exp):
    res = exp["prefix"]
    ids = fx.ids
    n = ids["n"]
    hops = [int(consts.dn[int(consts.dn_off[n]) + b]) for b in U.bits(sel[2][n, 0])]
    assert hops == [ids["x1"], ids["x2"], ids["x3"]]  # the slot order the case is about
    for p in (0, 1, 2):
        assert fx.at(res, "n", p) == (U.OVERFLOW, 0) and fx.at(res, "m", p) == (U.OVERFLOW, 0)
    assert fx.at(res, "n", 3) == (U.OK, I63) and fx.at(res, "m", 3) == (U.OK, I63)
    for v, first, second in (("v1", "h1", "k1"), ("v2", "h2", "k2")):
        lo = int(consts.dn_off[ids[v]])
        assert [int(consts.dn[lo + b]) for b in U.bits(sel[2][ids[v], 4])] == [ids[first], ids[second]]
    assert fx.at(res, "h1", 4)[0] == U.OVERFLOW and fx.at(res, "k1", 4)[0] == U.VOID
    assert fx.at(res, "h2", 4)[0] == U.VOID and fx.at(res, "k2", 4)[0] == U.OVERFLOW
    for nm in ("v1", "v2", "w1"):
        assert fx.at(res, nm, 4) == (U.VOID, 0), nm


def spoke(i):
    return f"s{i:04d}"


def hub_fixture(N):
    """A hub with N spokes by one link each (no ring) and zq behind the hub by
    two parallel links; zq's id is the largest, so spoke i is bit i of the
    hub's mask and the hub has N + 1 neighbours: 4 words for N = 127 (the
    last width of the lane path), 5 for N = 128 (the fifth word holds zq only)
    and for N = 129 (spoke 128 in the fifth word).
    Prefixes: A every spoke, the sum exactly I63; E spokes 0 and 64 with 2^62
    each (words 0 and 2: the overflow of two lanes that no third lane sees);
    B as A, the last spoke's weight one more; C spoke 0 of weight zero and
    2^62 in three other words; D every spoke from the small pool; E2 spokes 0
    and N - 1 with 2^62 each."""
    links = [l for i in range(N) for l in L("hub", spoke(i))] + L("hub", "zq", 2)
    a = {spoke(i): I63 // N + (i < I63 % N) for i in range(N)}
    b = dict(a)
    b[spoke(N - 1)] += 1
    rng = np.random.default_rng(N)
    d = {spoke(i): int(w) for i, w in enumerate(rng.choice(POOL, size=N))}
    return Fixture(links, [a, {spoke(0): A62, spoke(64): A62}, b,
                           {spoke(0): 0, spoke(40): A62, spoke(70): A62, spoke(N - 1): A62}, d,
                           {spoke(0): A62, spoke(N - 1): A62}])


def hub_roots(fx, N):
    return [fx.ids[nm] for nm in ("hub", "zq", spoke(0), spoke(64), spoke(N - 1))]


def assert_hub(fx, consts, sel, exp, N):
    v, ids = fx.version, fx.ids
    hub = ids["hub"]
    words = (N + 1 + 31) // 32
    assert v.words == words == {127: 4, 128: 5, 129: 5}[N]
    assert v.nbrs(hub) == [ids[spoke(i)] for i in range(N)] + [ids["zq"]]
    mask = sel[2][hub]
    assert (mask[0, :(N + 31) // 32] != 0).all() and (mask[2, :(N + 31) // 32] != 0).all()
    if N == 129:
        assert mask[0, 4] == 1 and mask[2, 4] == 1  # the fifth word: spoke 128
    res = exp["prefix"]
    by_bit = lambda p: dict(zip(U.bits(mask[p]), fx.leaf_w[p]))  # noqa: E731  (every announcer a next hop)
    for p in (0, 1, 2):  # no word's weights overflow on their own: across words (lanes) only
        w = by_bit(p)
        assert len(w) == len(fx.leaf_w[p])
        assert max(sum(x for b, x in w.items() if b // 32 == k) for k in range(words)) <= I63 // 2 + 1
    assert sum(fx.leaf_w[0]) == I63 and sum(fx.leaf_w[2]) == I63 + 1
    assert fx.at(res, "hub", 0) == (U.OK, I63) and fx.at(res, "zq", 0) == (U.OVERFLOW, 0)
    assert fx.at(res, "hub", 1) == (U.OVERFLOW, 0) and fx.at(res, "hub", 5) == (U.OVERFLOW, 0)
    assert fx.at(res, "hub", 2) == (U.OVERFLOW, 0) and fx.at(res, spoke(0), 2)[0] == U.OK
    assert fx.at(res, "hub", 3) == (U.VOID, 0) and fx.at(res, "zq", 3) == (U.VOID, 0)
    assert U.bits(mask[3]) == [0, 40, 70, N - 1]  # the zero weight and the large ones in different words
    assert fx.at(res, "hub", 4) == (U.OK, sum(fx.leaf_w[4]))
    assert fx.at(res, "zq", 4) == (U.OK, 2 * sum(fx.leaf_w[4]))
    assert exp["prefix"][2] == 2 and exp["adj"][2] == 2


STAR = 2100


def star_fixture():
    """A hub with 2,100 spokes and zq (two parallel links): 2,101 neighbours,
    66 words, so a lane of the wave path takes two words. p0's announcers sit
    in words 0, 63, 64 and 65 of the hub's mask; p3 is zq (word 65, c = 2)."""
    links = [l for i in range(STAR) for l in L("hub", spoke(i))] + L("hub", "zq", 2)
    return Fixture(links, [{spoke(5): 4, spoke(63 * 32 + 1): 6, spoke(64 * 32 + 2): 9, spoke(65 * 32 + 3): 10},
                           {spoke(40): 3}, {spoke(10): 9, spoke(STAR - 1): 6}, {"zq": 10}])


def star_roots(fx):
    """-> the four roots compared, the roots the recursion needs (them and
    every announcer: the oracle's SPF of 2,102 roots would take minutes)"""
    look = [fx.ids[nm] for nm in ("hub", "zq", spoke(5), spoke(1000))]
    return look, sorted(set(look) | {a for ann in fx.table for a in ann})


def assert_star(fx, consts, sel, exp):
    hub = fx.ids["hub"]
    assert fx.version.words == 66
    mask = sel[2][hub]
    assert [b // 32 for b in U.bits(mask[0])] == [0, 63, 64, 65]
    assert U.bits(mask[3]) == [STAR]  # zq: the last bit in use, word 65
    res = exp["prefix"]
    assert [fx.at(res, "hub", p) for p in range(4)] == [(U.OK, 29), (U.OK, 3), (U.OK, 15), (U.OK, 20)]
    assert fx.at(res, spoke(1000), 0) == (U.OK, 29) and fx.at(res, "zq", 0) == (U.OK, 58)
    assert fx.view(consts, sel, res, "hub", 2) == [(spoke(10), 3), (spoke(STAR - 1), 2)]
    assert exp["prefix"][2] == 2


def policy_fixture():
    """Policy states (the drained-leaf rule; every announcer in one class).
    x - k - u, and u2 - k by two parallel links, k drained with leaf weight
    I63: u takes I63 over its one link, u2 twice that (k's own entry selects x).
    k0 and t drained announcers, k0 of weight zero: v reaches k0 directly over
    a link of metric 2 and t (I63) through o, which multiplies it by two links:
    a zero-weight drained leaf in the slot before an OVERFLOW next hop. v2 is
    the mirror image: the OVERFLOW next hop o2 before the drained leaf y2."""
    links = L("x", "k") + L("k", "u") + L("k", "u2", 2)
    links += L("v", "k0", m=2) + L("v", "o") + L("o", "t", 2)
    links += L("v2", "y2", m=2) + L("v2", "o2") + L("o2", "t2", 2)
    dbs = named_dbs(links, over=("k", "k0", "t", "y2", "t2"))
    ids = {nm: i for i, nm in enumerate(sorted(d.name for d in dbs))}
    pf = [{"k": I63, "x": 7}, {"k0": 0, "t": I63, "y2": 0, "t2": I63}]
    table = [sorted(ids[nm] for nm in p) for p in pf]
    leaf_w = [[w for _, w in sorted((ids[nm], w) for nm, w in p.items())] for p in pf]
    case = PolicyCase(dbs, table, [[0] * len(a) for a in table], leaf_w)
    assert case.names == sorted(ids, key=ids.get)
    return case, ids


def assert_policy(case, ids, sel, consts, exp):
    res = exp["prefix"]
    at = lambda nm, p: (int(res[1][ids[nm], p]), int(res[0][ids[nm], p]))  # noqa: E731
    assert at("u", 0) == (U.OK, I63) and at("u2", 0) == (U.OVERFLOW, 0)
    assert at("k", 0) == (U.OK, 7) and sel["metric"][ids["k"], 0] == 1  # k's own entry selects x
    mine = UP.links(sel, consts, res, ids["u"], 0, case.table, case.leaf_w, case.drained)
    assert mine == [(ids["k"], 1, 1)]  # I63 / gcd = 1
    assert at("o", 1) == (U.OVERFLOW, 0) and at("o2", 1) == (U.OVERFLOW, 0)
    for v, first, second in (("v", "k0", "o"), ("v2", "o2", "y2")):
        lo = int(consts.dn_off[ids[v]])
        assert [int(consts.dn[lo + b]) for b in U.bits(sel["nh"][ids[v], 1])] == [ids[first], ids[second]]
        assert at(v, 1) == (U.VOID, 0)
    without = case.resolve(sel, consts, "prefix", leaf_rule=False)
    assert int(without[0][ids["u"], 0]) == 7  # the rule is what gives u the leaf weight


# ---------------------------------------------------------------- against the oracle
def oracle_check(fx, consts, sel, exp, hop=False):
    """every entry the recursion does not mark OVERFLOW against the oracle's
    walk of its root -> (entries compared, entries left out as OVERFLOW)"""
    from oracle import Oracle
    v = fx.version
    orc = Oracle(v.stream)
    spf = v.spf(not hop)
    done = skipped = 0
    for algo in U.ALGOS:
        Wv, st, _ = exp[algo]
        for r in range(v.V):
            for p, ann in enumerate(fx.table):
                best = U.min_cost(spf[v.names[r]], v.names, ann)
                lw = dict(zip(ann, fx.leaf_w[p]))
                if not best or any(lw[a] == 0 for a in best):
                    assert st[r, p] == (U.VOID if best else U.NONE)
                    continue
                if st[r, p] == U.OVERFLOW:
                    skipped += 1
                    continue
                got = orc.ucmp(v.names[r], {v.names[a]: lw[a] for a in best}, algo, not hop)
                w, hops = got[v.names[r]]
                mine = U.links(sel, consts, exp[algo], r, p)
                assert st[r, p] == U.OK and int(Wv[r, p]) == w, (algo, v.names[r], p)
                assert sorted((v.names[k], wt) for k, c, wt in mine for _ in range(c)) == \
                    sorted((nh, hw) for nh, hw in hops.values()), (algo, v.names[r], p)
                done += 1
    return done, skipped


def test_exact_leaf_exact_sum_and_gcd_equal_the_oracle():
    fx = exact_fixture()
    consts, sel, exp = fx.expectation()
    assert_exact(fx, consts, sel, exp)
    done, skipped = oracle_check(fx, consts, sel, exp)
    assert skipped == 2 * 4 and done == 2 * 6 * 6 - skipped  # 'adj': the link weight sums fit


SUMS = (  # S overrides of the exact fixture -> (status, weight) of s for p1 under 'adj'
    ({("s", "t1"): A62, ("s", "t2"): A62}, (U.OVERFLOW, 0)),
    ({("s", "t1"): A62 - 1, ("s", "t2"): A62}, (U.OK, I63)),
    ({("s", "t1"): I63, ("s", "t2"): 0, ("r", "s"): I63}, (U.OK, I63)),
    ({("s", "t1"): I63, ("s", "t2"): 1}, (U.OVERFLOW, 0)),
)


def assert_sums(fx, exp, want):
    res = exp["adj"]
    assert fx.at(res, "s", 1) == want
    assert fx.at(res, "r", 1)[0] == want[0] and fx.at(res, "a", 1)[0] == want[0]
    assert fx.at(res, "a", 0) == (U.OK, I63)  # a slot of exactly I63 is a weight like any other
    assert fx.at(exp["prefix"], "s", 1) == (U.OK, I63)  # S does not enter prefix-weight propagation


def test_exact_sums_through_the_link_weight_sums():
    """'adj' reaches the limit through S only: two slots of s at 2^62 each are
    OVERFLOW, 2^62 and 2^62 - 1 are OK with I63, a slot of exactly I63 is a
    weight like any other. (S is an input of the recursion and of the device;
    the fixture's own link weights, which the oracle reads, are the second
    case.)"""
    fx = exact_fixture()
    for sums, want in SUMS:
        _, _, exp = fx.expectation(sums=sums)
        assert_sums(fx, exp, want)
    _, _, exp = fx.expectation(sums=SUMS[2][0])
    assert fx.at(exp["adj"], "r", 1) == (U.OK, I63)


@pytest.mark.parametrize("hop", [False, True])
def test_products_equal_the_oracle_where_they_fit(hop):
    fx = product_fixture()
    consts, sel, exp = fx.expectation(hop)
    assert_product(fx, consts, exp, hop)
    done, skipped = oracle_check(fx, consts, sel, exp, hop)
    assert skipped == 2 * (6 + (2 if hop else 0)) and done > 3 * fx.version.V


def test_mixed_statuses_equal_the_oracle_where_they_fit():
    fx = mixed_fixture()
    consts, sel, exp = fx.expectation()
    assert_mixed(fx, consts, sel, exp)
    done, skipped = oracle_check(fx, consts, sel, exp)
    assert skipped == 3 * 2 + 2 and done > 2 * fx.version.V  # n and m three times; h1 and k2


def test_hub_of_129_equals_the_oracle_where_it_fits():
    fx = hub_fixture(129)
    consts, sel, exp = fx.expectation()
    assert_hub(fx, consts, sel, exp, 129)
    done, skipped = oracle_check(fx, consts, sel, exp)
    assert done > 5 * fx.version.V and skipped > 2 * 127  # E and E2: the hub, zq and the spokes that do not announce


@pytest.mark.parametrize("N", [127, 128])
def test_hub_fixtures_hold_what_they_exist_for(N):
    fx = hub_fixture(N)
    consts, sel, exp = fx.expectation()
    assert_hub(fx, consts, sel, exp, N)


def test_star_of_66_words_fixture():
    fx = star_fixture()
    look, need = star_roots(fx)
    consts, sel, exp = fx.expectation(roots=need)
    assert_star(fx, consts, sel, exp)


def test_policy_limits_equal_the_oracle_where_they_fit():
    """test_host_ucmp_policy.check restated with the OVERFLOW entries left out"""
    from test_host_ucmp_all import oracle_view
    case, ids = policy_fixture()
    spf, sel, consts = case.mode(True)
    exp = {algo: case.resolve(sel, consts, algo) for algo in U.ALGOS}
    assert_policy(case, ids, sel, consts, exp)
    done = skipped = 0
    for algo in U.ALGOS:
        Wv, st, _ = exp[algo]
        for r in range(case.V):
            for p, ann in enumerate(case.table):
                leaves = UP.policy_leaves(spf[case.names[r]], case.names, ann, case.pref[p], case.drained)
                lw = dict(zip(ann, case.leaf_w[p]))
                if not leaves or any(lw[a] == 0 for a in leaves):
                    assert st[r, p] == (U.VOID if leaves else U.NONE), (algo, r, p)
                    continue
                if st[r, p] == U.OVERFLOW:
                    skipped += 1
                    continue
                want_w, want_hops = oracle_view(case, r, {a: lw[a] for a in leaves}, algo, True)
                mine = UP.links(sel, consts, exp[algo], r, p, case.table, case.leaf_w, case.drained)
                assert st[r, p] == U.OK and int(Wv[r, p]) == want_w, (algo, r, p)
                assert {k: (c, w) for k, c, w in mine} == want_hops, (algo, r, p)
                done += 1
    assert skipped == 3 and done == 13  # u2, o and o2 under 'prefix' are left out
