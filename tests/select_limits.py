"""The anycast selection and its resident delta at their chunk and word limits:
explicit graphs, their tables and their oracle-derived expectation (shared by
test_host_select_limits.py and test_gpu_select_limits.py).

select_kernel and seldelta_kernel share the device functions of
spf_select_dev.h and one launch shape, and both have hard-coded constants:
kSelShort = 8 announcers walked by one lane, kSelLaneW = 4 words kept in a
lane, chunks of 64 prefixes, at most 4 waves a root (a fifth chunk is a wave's
second trip), the 64-entry stride of the neighbour-list compare, and distances
shuffled across the wave as `int`. policy_kernel, seldelta_policy_kernel and
srmpls_kernel copy the launch shape. Every fixture below sits on one of them:

  S1  distances with bit 31 set in the anycast minimum (walk, wave minimum,
      tie count), on the lane-per-word path (root a) and the lane paths (a1);
  S2  roots of exactly 2, 3, 4 and 5 next-hop words, and changes that show in
      a root's last word only (or in word 0 only);
  S3  tables of 64, 65, 256, 257 and 321 prefixes: a wave's second trip;
  S4  the change list's compaction: a chunk whose 64 lanes all changed, a
      lone change in lane 0 / lane 63, changes on the second trip, and the
      capacity one below the count (on S2's graph among a wide root's records);
  S5  a root rebased by a difference at position 128 of its neighbour list,
      its count and width unchanged.

The expectation is select_ref.expect / seldelta_ref.delta over the CPU oracle's
SPF and the CSR columns (for S3's policy faces selpolicy_ref, policy_delta_ref
and srmpls_ref) -- never the engine's rows -- and every case states, as asserts
on that expectation, the property that makes it a limit case (preconditions).
The only places where anything but the restatement appears are the four
models of WRONG kernels at the end of each section; the host test shows that
each disagrees with the expectation on its fixture.

A note on S1. An anycast minimum has no class to overrule the distance, so a
prefix whose expected metric has bit 31 set holds no reached announcer below
2^31, and on [2^31, 2^32) the signed order is the unsigned one: no minimum
over int32 views can differ there. The two properties therefore sit on paired
prefixes. The `far` and `tie` prefixes have every reached announcer (and the
metric) at 2^31 or above, the deciding one at position 0, 63, 64 or the last;
the `mixed` prefixes put the same far announcers beside near ones, where the
near one decides and the int32 minimum picks a far one instead. The cluster
has 141 far nodes, 112 of them behind the two nearest distances, so a far
prefix of 130 announcers has its deciding one at position 0 (c) or is the
tie; positions 63 and 64 of a far prefix are pinned at 65 announcers."""
import copy
import functools
from types import SimpleNamespace

import numpy as np

import policy_delta_ref as PD
import policy_limits as L
import seldelta_ref as D
import selpolicy_ref as PR
import srmpls_ref as SR
from graphs import metric_graph
from openr_amd.adjdb import AdjDb

INF = 0xFFFFFFFF
B31 = 0x80000000
CHUNK, WAVES = 64, 4          # prefixes a wave takes at a time; waves a root at most
TRIP = CHUNK * WAVES          # the first prefix of a wave's second trip


class Case(SimpleNamespace):
    """name; versions (seldelta_ref.Version); table (announcer ids per prefix,
    ascending); roots: the judged node ids (None: all); focus {role: node id};
    for S3 also pref / mnh / flags per entry"""

    @property
    def base(self):
        return self.versions[0]

    @property
    def judged(self):
        return list(range(self.base.V)) if self.roots is None else list(self.roots)

    def exp(self, W, version=0):
        """select_ref.expect's (metric, count, nh) at width W (kept)"""
        key = ("exp", W, version)
        if key not in self._kept:
            self._kept[key] = self.versions[version].expect(self.table, W, True, self.roots)
        return self._kept[key]

    def delta(self, W, before=0, after=1):
        """seldelta_ref.delta between two versions -> (changed, rebased, ea, eb),
        judged roots only (kept)"""
        key = ("delta", W, before, after)
        if key not in self._kept:
            self._kept[key] = D.delta(self.versions[before], self.versions[after], self.table, W,
                                      True, self.roots)
        return self._kept[key]

    def dists(self, root, p, version=0):
        """the oracle's distances of prefix p's announcers from `root`, kInf
        where unreached: what the kernel gathers"""
        v = self.versions[version]
        res = v.spf(True, [root])[v.names[root]]
        return np.array([res[v.names[x]][0] if v.names[x] in res else INF
                         for x in self.table[p]], np.uint32)

    # S3's policy faces
    def pol(self, W, version=0):
        key = ("pol", W, version)
        if key not in self._kept:
            self._kept[key] = PD.expect(self.versions[version], self.table, self.pref, self.mnh, W,
                                        roots=self.roots)[0]
        return self._kept[key]

    def sr(self, W):
        key = ("sr", W)
        if key not in self._kept:
            v = self.base
            self._kept[key] = SR.expect(v.spf(True, self.roots), v.names, v.csr, self.table,
                                        self.pref, self.mnh, self.flags, W, roots=self.roots)
        return self._kept[key]

    def pdelta(self, W, before=0, after=1):
        eb, ea = self.pol(W, before), self.pol(W, after)
        vb, va = self.versions[before], self.versions[after]
        rebased = [r for r in range(vb.V) if vb.nbrs(r) != va.nbrs(r)]
        keep = set(self.judged)
        return {c for c in PD.diff(eb, ea, rebased) if c[0] in keep}, rebased, ea, eb


def make(name, versions, rows, roots=None, focus=(), **more):
    """rows: per prefix the announcers' names, any order"""
    ids = {nm: i for i, nm in enumerate(versions[0].names)}
    assert all(v.names == versions[0].names for v in versions)
    table = [sorted(ids[nm] for nm in ents) for ents in rows]
    assert all(len(set(a)) == len(a) for a in table), "a node twice in a prefix"
    return Case(name=name, versions=versions, table=table,
                roots=None if roots is None else sorted(ids[r] for r in roots),
                focus={r: ids[r] for r in focus}, ids=ids, _kept={}, **more)


def raise_metric(dbs, a, b, by=1):
    """the metric a advertises towards b raised (one direction of one link)"""
    out = copy.deepcopy(dbs)
    hit = [adj for d in out if d.name == a for adj in d.adjs if adj.other == b]
    assert len(hit) == 1, (a, b, len(hit))
    hit[0].metric += by
    return out


def spread(pool, m):
    """m entries of `pool`, evenly spread over it, in order"""
    assert 0 <= m <= len(pool), (m, len(pool))
    return [pool[i * len(pool) // m] for i in range(m)]


def changed_of(changed, root):
    return sorted(p for r, p in changed if r == root)


# ---------------------------------------------------------------- S1
S1_ROOTS = ("a", "a1", "b", "c", "d000", "k000", "s100", "zz")
S1_LONE = "zz"  # the isolated node: an announcer no root but itself reaches


def s1_dbs(bump=False):
    """policy_limits.l1_dbs() (a: 131 neighbours, five words; a1: one word;
    c at 0x80000005 from a and the 140 cluster nodes k<i> at 0x80000006 + i % 5)
    and the isolated node zz. bump: b -> c costs 7 instead of 6, every far
    distance moves from one value of at least 2^31 to the next."""
    dbs = L.l1_dbs() + [AdjDb(S1_LONE, [], 999)]
    return raise_metric(dbs, "b", "c") if bump else dbs


def s1_rows():
    """-> (rows, plan): plan[p] = (kind, announcers, position of the deciding
    one or None for a tie). k<i> with i % 5 == 0 is the nearest cluster class;
    spokes <j> with j % 3 == 0 are at 1 from a, the others at 2 and 3."""
    k = lambda i: f"k{i:03d}"                                        # noqa: E731
    K0 = [k(i) for i in range(L.L1_CLUSTER) if i % 5 == 0]
    KX = [k(i) for i in range(L.L1_CLUSTER) if i % 5]
    NEAR = [L.spoke(j) for j in range(L.L1_SPOKES) if j % 3]
    rows, plan = [], []

    def place(kind, n, q, decider, pool, tail=()):
        """n announcers, `decider` at position q: q of the pool's names below
        it, the rest above, `tail` (sorting last) at the end"""
        pool = sorted(pool)
        before = spread([x for x in pool if x < decider], q)
        after = spread([x for x in pool if x > decider], n - 1 - q - len(tail))
        rows.append(before + [decider] + after + list(tail))
        assert len(rows[-1]) == n
        plan.append((kind, n, q))

    zz = [S1_LONE]
    # every reached announcer at 2^31 or above
    place("far", 8, 0, "c", KX, zz)
    place("far", 8, 6, "k010", KX, zz)
    place("far", 9, 0, "c", KX, zz)
    place("far", 9, 7, "k010", KX, zz)
    place("far", 65, 0, "c", KX, zz)
    place("far", 65, 63, "k080", KX, zz)
    place("far", 65, 64, "k080", KX)
    place("far", 130, 0, "c", KX + K0, zz)
    # ties of the nearest cluster class, on both trips of the 130
    for n in (9, 65, 130):
        rows.append([k(i) for i in range(n + 1) if i != 1])  # k000 first, a tied one last
        plan.append(("tie", n, None))
    # a near announcer decides beside far ones
    mixed = NEAR + KX + K0
    place("mixed", 8, 0, "d000", mixed, zz)
    place("mixed", 9, 0, "d000", mixed, zz)
    place("mixed", 9, 8, "s066", mixed)
    place("mixed", 65, 0, "d000", mixed, zz)
    place("mixed", 65, 63, "s066", mixed, zz)
    place("mixed", 65, 64, "s066", mixed)
    place("mixed", 130, 0, "d000", mixed, zz)
    place("mixed", 130, 86, "s066", mixed, zz)
    rows.append([S1_LONE])  # nothing reached (but by zz itself)
    plan.append(("lone", 1, None))
    return rows, plan


def min_kernel(c, root, p, signed=False, version=0):
    """(metric, count) of (root, prefix p) from a kernel that gathers the
    oracle's distances (kInf where unreached) and takes their minimum --
    unsigned as the right kernel does, or (signed) over int32 views, as `min`
    on the shuffled `int` or a signed `d < m` would; the tie count is
    `dist == m`, kInf never counted."""
    d = c.dists(root, p, version)
    if not d.size:
        return INF, 0
    m = int(d.view(np.int32).min().astype(np.int32).view(np.uint32)) if signed else int(d.min())
    return (INF, 0) if m == INF else (m, int((d == m).sum()))


def s1_preconditions(c):
    v, w = c.versions
    a, a1 = c.focus["a"], c.focus["a1"]
    assert L.words_of(v, a) == 5 and len(v.nbrs(a)) == 131 and L.words_of(v, a1) == 1
    assert v.nbrs(c.focus[S1_LONE]) == []
    assert sorted(set(n for _, n, _ in c.plan)) == [1, 8, 9, 65, 130]
    em, ec, _ = c.exp(5)
    changed, rebased, ea, eb = c.delta(5)
    assert not rebased
    for r in (a, a1):
        assert S1_LONE not in v.spf(True, [r])[v.names[r]]
        for p, (kind, n, q) in enumerate(c.plan):
            assert len(c.table[p]) == n
            d = c.dists(r, p)
            want = (int(em[r, p]), int(ec[r, p]))
            assert min_kernel(c, r, p) == want, (kind, n, q)  # the model, right, is the rule
            wrong = min_kernel(c, r, p, signed=True)
            at = np.nonzero(d == em[r, p])[0].tolist()
            if kind == "lone":
                assert want == (INF, 0)
                continue
            if kind in ("far", "tie"):
                assert em[r, p] >= B31 and (d >= B31).all()
                assert wrong == want  # see the module's note: no signed minimum differs here
                # the update moves the deciding distance from one far value to the next
                assert (r, p) in changed and eb[0][r, p] >= B31 and ea[0][r, p] == eb[0][r, p] + 1
                assert ea[1][r, p] == eb[1][r, p]
            if kind == "tie":
                assert ec[r, p] == len(at) == len(range(0, n + 1, 5)) >= 2
                assert at[0] == 0 and (n % 5 or at[-1] == n - 1)
                assert n < 130 or (sum(i < 64 for i in at) >= 2 and at[-1] >= 128)
            else:
                assert ec[r, p] == 1 and at == [q], (kind, n, q, at)
            if kind == "mixed":
                assert em[r, p] < B31 and ((d >= B31) & (d != INF)).any()
                assert wrong != want and wrong[0] >= B31, (kind, n, q, wrong, want)
                assert (r, p) not in changed
    placed = {(kind, n, q) for kind, n, q in c.plan}
    for kind in ("far", "mixed"):
        assert {(kind, 8, 0), (kind, 9, 0), (kind, 65, 0), (kind, 65, 63), (kind, 65, 64),
                (kind, 130, 0)} <= placed
    assert ("mixed", 130, 86) in placed and ("tie", 130, None) in placed
    assert 0 < len(changed) < v.V * len(c.table)


def s1():
    rows, plan = s1_rows()
    return make("S1", [D.Version(s1_dbs()), D.Version(s1_dbs(bump=True))], rows, roots=S1_ROOTS,
                focus=("a", "a1", S1_LONE), plan=plan)


# ---------------------------------------------------------------- S2 / S5
S2_HUBS = {"h2": 64, "h3": 96, "h4": 128, "h5": 129}  # distinct neighbours: W = 2, 3, 4, 5
S2_T = {"h2": 0, "h3": 63, "h4": 64, "h5": 65}        # the table positions of [t<w>]
S2_U = {"h2": 1, "h3": 2, "h4": 3, "h5": 4}           # ... of [u<w>]
S2_NINE, S2_LONG, S2_EMPTY, S2_HUBROW, S2_P = 5, 6, 7, 8, 70


def s2_dbs(top=False, low=False, moved=False):
    """The hubs h2, h3, h4, h5 over the first 64, 96, 128 and 129 of the spokes
    p000 .. p128 (2 either way). Behind hub h<w> the target t<w> hangs at 1 on
    the hub's two last neighbours -- the two highest bits in use; for h5 bit 31
    of word 3 and bit 0 of word 4 -- and the target u<w> at 1 on its first two
    and its last. w hangs off p000.
    top: the last neighbour's link towards t<w> costs 2, for all four hubs:
      the hub reaches t<w> through the other one alone -- the same metric and
      count, words 0 .. W - 2 unchanged, the top bit of word W - 1 gone.
    low: p000's link towards u<w> costs 2: bit 0 of word 0 goes, the last word
      keeps its top bit.
    moved (S5): h5 is linked to w instead of p128: 129 neighbours and five
      words as before, another id at position 128 of its list."""
    p = lambda i: f"p{i:03d}"  # noqa: E731
    links = []
    for hub, n in S2_HUBS.items():
        t, u = "t" + hub[1], "u" + hub[1]
        for i in range(n):
            if moved and hub == "h5" and i == n - 1:
                links.append((hub, "w", 2, 2))
            else:
                links.append((hub, p(i), 2, 2))
        links += [(p(n - 2), t, 1, 1), (p(n - 1), t, 2 if top else 1, 1)]
        links += [(p(0), u, 2 if low else 1, 1), (p(1), u, 1, 1), (p(n - 1), u, 1, 1)]
    links.append(("w", "p000", 3, 3))
    return metric_graph(links)


def s2_rows():
    """70 prefixes (a chunk of 64 and a tail of 6): the targets' at 0, 63, 64
    and 65, prefixes of 9 and 65 announcers, an empty one, single spokes"""
    p = lambda i: f"p{i:03d}"  # noqa: E731
    rows = [[p(2 * i + 1)] for i in range(S2_P)]
    for hub in S2_HUBS:
        rows[S2_T[hub]] = ["t" + hub[1]]
        rows[S2_U[hub]] = ["u" + hub[1]]
    rows[S2_NINE] = [p(i) for i in (5, 31, 32, 63, 64, 95, 96, 127, 128)]
    rows[S2_LONG] = [p(i) for i in range(30, 95)]
    rows[S2_EMPTY] = []
    rows[S2_HUBROW] = list(S2_HUBS)
    rows[66:70] = [["w"], [p(128)], [p(0)], ["t2", "t3", "t4", "t5"]]
    assert len(rows) == S2_P
    return rows


def last_word_blind(c, W, before, after):
    """the changed set of a kernel whose compare stops one word short of each
    root's own width"""
    _, rebased, ea, eb = c.delta(W, before, after)
    out = set()
    for r in c.judged:
        if r in rebased:
            continue
        w = L.words_of(c.versions[after], r)
        differ = (eb[0][r] != ea[0][r]) | (eb[1][r] != ea[1][r]) | \
            (eb[2][r, :, :w - 1] != ea[2][r, :, :w - 1]).any(axis=1)
        out |= {(r, int(p)) for p in np.nonzero(differ)[0]}
    return out


def s2_preconditions(c):
    v = c.base
    W = v.words
    assert W == 5 and len(c.table) == S2_P > CHUNK and c.roots is None
    assert [len(c.table[p]) for p in (S2_NINE, S2_LONG, S2_EMPTY)] == [9, 65, 0]
    changed, rebased, ea, eb = c.delta(W, 0, 1)
    assert not rebased and 0 < len(changed) < v.V * S2_P
    changed2, rebased2, ea2, eb2 = c.delta(W, 1, 2)
    assert not rebased2 and 0 < len(changed2) < v.V * S2_P
    blind = last_word_blind(c, W, 0, 1)
    for hub, n in S2_HUBS.items():
        h, w = c.ids[hub], int(hub[1])
        nb = v.nbrs(h)
        assert len(nb) == n and L.words_of(v, h) == w
        assert n == 32 * w if w < 5 else n == 32 * (w - 1) + 1  # the widest of W, the narrowest of 5
        top = len(nb) - 1          # the highest bit in use, from the root's own list
        tw, tb = top // 32, top % 32
        assert tw == w - 1
        e = c.exp(W)
        # the wave paths at this width: wide words from prefixes of 9 and 65
        assert e[1][h, S2_LONG] >= 34 and e[2][h, S2_LONG, :min(w, 3)].all()
        assert e[1][h, S2_NINE] >= 3 and e[0][h, S2_HUBROW] == 0 and not e[2][h, S2_HUBROW].any()
        # t<w>: behind the two last neighbours; the event takes the top bit only
        pt = S2_T[hub]
        assert c.table[pt] == [c.ids["t" + hub[1]]]
        for k in (top - 1, top):
            assert e[2][h, pt, k // 32] >> (k % 32) & 1
        assert PR.decode(e[2][h, pt], nb) == {nb[top - 1], nb[top]}
        assert (h, pt) in changed and (h, pt) not in blind
        assert eb[0][h, pt] == ea[0][h, pt] == 3 and eb[1][h, pt] == ea[1][h, pt] == 1
        assert np.nonzero(eb[2][h, pt] != ea[2][h, pt])[0].tolist() == [tw]
        assert int(eb[2][h, pt, tw]) ^ int(ea[2][h, pt, tw]) == 1 << tb
        assert PR.decode(ea[2][h, pt], nb) == {nb[top - 1]}
        # u<w>: the second event changes word 0 alone, the last word stays set
        pu = S2_U[hub]
        assert (h, pu) in changed2
        assert eb2[0][h, pu] == ea2[0][h, pu] and eb2[1][h, pu] == ea2[1][h, pu]
        assert np.nonzero(eb2[2][h, pu] != ea2[2][h, pu])[0].tolist() == [0]
        assert ea2[2][h, pu, tw] >> tb & 1 and ea2[2][h, pu, 0] == 2 and eb2[2][h, pu, 0] == 3
    assert [S2_T[h] for h in ("h2", "h3", "h4")] == [0, CHUNK - 1, CHUNK]
    assert blind < changed
    # S4 on this graph: the capacity falls among the five-word hub's records
    assert len(changed_of(changed, c.ids["h5"])) >= 3


def s2():
    return make("S2", [D.Version(s2_dbs()), D.Version(s2_dbs(top=True)),
                       D.Version(s2_dbs(top=True, low=True))], s2_rows(), focus=tuple(S2_HUBS))


S5_ROOTS = ("h2", "h4", "h5", "p000", "p127", "p128", "t5", "u5", "w")


def first_64_rebased(vb, va, roots):
    """the rebased roots of a kernel that compares the counts, the widths and
    the first 64 entries of the two neighbour lists"""
    out = []
    for r in roots:
        b, a = vb.nbrs(r), va.nbrs(r)
        if len(b) != len(a) or L.words_of(vb, r) != L.words_of(va, r) or b[:64] != a[:64]:
            out.append(r)
    return out


def s5_preconditions(c):
    vb, va = c.versions
    h5, p128, w = c.ids["h5"], c.ids["p128"], c.ids["w"]
    b, a = vb.nbrs(h5), va.nbrs(h5)
    assert len(b) == len(a) == 129 and L.words_of(vb, h5) == L.words_of(va, h5) == 5
    assert b[:128] == a[:128] and [i for i in range(129) if b[i] != a[i]] == [128]
    assert b[128] == p128 == max(b) and a[128] == w > p128 and w not in b
    changed, rebased, ea, eb = c.delta(5)
    assert rebased == sorted([h5, p128, w])
    assert len(vb.nbrs(p128)) == 3 and len(va.nbrs(p128)) == 2
    assert not changed_of(changed, h5) and changed
    assert (ea[2][h5] != eb[2][h5]).any()  # the bits mean other neighbours and say so
    assert first_64_rebased(vb, va, c.judged) == sorted([p128, w])


def s5():
    return make("S5", [D.Version(s2_dbs()), D.Version(s2_dbs(moved=True))], s2_rows(),
                roots=S5_ROOTS, focus=("h5", "p128", "w"))


# ---------------------------------------------------------------- S3 / S4
S3_CORE = 72
S3_SIZES = (64, 65, 256, 257, 321)
S4_LEAVES = (0, 63, 64, 255, 256, 320)  # the table positions of [t0] .. [t5]


def s3_dbs(stub=False, leaves=False):
    """A ring of 72 core nodes with chords (metrics 1 to 5, asymmetric), the
    stub root r on c07 and the stub leaves t0 .. t5: 79 nodes, every root one
    word. stub: r's link towards c07 costs 9 instead of 4 -- every distance
    from r grows, nothing else moves. leaves: each leaf's inbound direction
    costs 1 more -- every other root's distance to that leaf grows."""
    c = lambda i: f"c{i % S3_CORE:02d}"  # noqa: E731
    links = [(c(i), c(i + 1), 1 + i % 3, 1 + (i + 1) % 3) for i in range(S3_CORE)]
    links += [(c(i), c(7 * i + 11), 2 + i % 4, 3) for i in range(0, S3_CORE, 5)]
    links.append(("r", "c07", 9 if stub else 4, 2))
    links += [(c(11 * j + 3), f"t{j}", 3 if leaves else 2, 1 + j % 2) for j in range(6)]
    return metric_graph(links)


@functools.lru_cache(maxsize=None)
def s3_versions():
    return (D.Version(s3_dbs()), D.Version(s3_dbs(stub=True)),
            D.Version(s3_dbs(stub=True, leaves=True)))


def s3_rows(P, leaves=False):
    """single core announcers, a prefix of 9 and one of 65 announcers at the
    table's end (inside the last chunk where that holds two prefixes); leaves:
    S4's table, [t0] .. [t5] at S4_LEAVES and the two long prefixes before the
    last position"""
    c = lambda i: f"c{i % S3_CORE:02d}"  # noqa: E731
    rows = [[c(5 * p + 1)] for p in range(P)]
    end = P - 1 if leaves else P
    rows[end - 2] = [c(8 * i + 2) for i in range(9)]
    rows[end - 1] = [c(i) for i in range(3, 68)]
    if leaves:
        for j, p in enumerate(S4_LEAVES):
            rows[p] = [f"t{j}"]
    assert len(rows) == P and sorted(len(x) for x in rows)[-2:] == [9, 65]
    return rows


def s3_policy(table, P):
    """a random two-class policy, thresholds 0 .. 2, random prepend flags"""
    rng = np.random.default_rng(300 + P)
    pref, mnh = PR.random_policy(table, rng, classes=2, max_need=2)
    return dict(pref=pref, mnh=mnh, flags=SR.random_flags(table, rng))


def one_trip(want, prev):
    """what a kernel whose waves make one trip leaves behind: the cells of
    prefixes >= 256 keep `prev` (the stored entry, or the buffer's poison)"""
    out = np.array(want, copy=True)
    out[:, TRIP:] = prev[:, TRIP:] if isinstance(prev, np.ndarray) else prev
    return out


def s3_preconditions(c):
    v = c.base
    P = len(c.table)
    assert v.V == 79 <= 80 and v.words == 1 and c.roots is None and P in S3_SIZES
    assert sum(len(a) for a in c.table) < 1000
    r = c.ids["r"]
    assert all(r not in a for a in c.table)
    changed, rebased, ea, eb = c.delta(1)
    assert not rebased and changed == {(r, p) for p in range(P)}  # every prefix, r's alone
    assert 0 < len(changed) < v.V * P
    pchanged, prebased, pa, pb = c.pdelta(1)
    assert not prebased and {x[0] for x in pchanged} == {r} and len(pchanged) >= P - 8
    if P > TRIP:
        em = c.exp(1)[0]
        assert (em[:, TRIP:] != INF).any() and (c.pol(1)["metric"][:, TRIP:] != INF).any()
        assert (c.sr(1)[0]["metric"][:, TRIP:] != INF).any()
        assert any(p >= TRIP for _, p in changed) and any(p >= TRIP for _, p in pchanged)
        # a kernel of one trip: poison in the one-shot outputs, the stored entry in the state
        for k in range(2):
            assert (one_trip(c.exp(1)[k], INF) != c.exp(1)[k]).any()
        assert (one_trip(ea[0], eb[0]) != ea[0]).any()
        assert (one_trip(pa["metric"], pb["metric"]) != pa["metric"]).any()
        assert (one_trip(c.sr(1)[0]["links"], INF) != c.sr(1)[0]["links"]).any()
    else:
        assert (one_trip(ea[0], eb[0]) == ea[0]).all()
    # the long prefixes sit at the table's end
    assert [len(c.table[p]) for p in (P - 2, P - 1)] == [9, 65]


def s3(P):
    rows = s3_rows(P)
    c = make(f"S3-{P}", list(s3_versions()[:2]), rows, focus=("r",))
    c.__dict__.update(s3_policy(c.table, P))
    return c


def s4_preconditions(c):
    v = c.base
    P = len(c.table)
    assert P == 321 and c.roots is None
    r = c.ids["r"]
    leaves = [c.ids[f"t{j}"] for j in range(6)]
    assert [c.table[p] for p in S4_LEAVES] == [[t] for t in leaves]
    assert all(len(v.nbrs(x)) == 1 for x in [r] + leaves)
    # (i) a chunk whose 64 lanes all changed, of root r alone
    changed, rebased, ea, eb = c.delta(1, 0, 1)
    assert not rebased and 0 < len(changed) < v.V * P
    mine = changed_of(changed, r)
    assert any(all(p in mine for p in range(b, b + CHUNK)) for b in range(0, P - CHUNK + 1, CHUNK))
    assert mine == list(range(P)) and {x[0] for x in changed} == {r}
    # (ii) lone changes in lane 0 and lane 63 of a chunk, on both trips
    changed, rebased, ea, eb = c.delta(1, 1, 2)
    assert not rebased and 0 < len(changed) < v.V * P
    for x in range(v.V):
        if x not in leaves:
            assert changed_of(changed, x) == list(S4_LEAVES), v.names[x]
    assert {p % CHUNK for p in S4_LEAVES} == {0, CHUNK - 1}
    assert sum(p >= TRIP for p in S4_LEAVES) == 2


def s4():
    return make("S4", list(s3_versions()), s3_rows(321, leaves=True), focus=("r",))


# ---------------------------------------------------------------- the cases
CASES = {"S1": s1, "S2": s2, "S4": s4, "S5": s5}
CASES.update({f"S3-{P}": functools.partial(s3, P) for P in S3_SIZES})


def preconditions(c):
    {"S1": s1_preconditions, "S2": s2_preconditions, "S4": s4_preconditions,
     "S5": s5_preconditions}.get(c.name, s3_preconditions)(c)


@functools.lru_cache(maxsize=None)
def case(name):
    """a fixture with its table and expectations (built once, never changed);
    its preconditions have held"""
    c = CASES[name]()
    preconditions(c)
    return c


def prefixes_by_name(c):
    """the table in LinkState.all_sources_select's / track_select's form"""
    return D.prefixes_by_name(c.base.names, c.table)
