"""The policy selection at its word, key and count limits: explicit graphs,
their tables and their oracle-derived expectation (shared by
test_host_policy_limits.py and test_gpu_policy_limits.py).

policy_kernel, seldelta_policy_kernel and srmpls_kernel share the device
functions of spf_selpolicy_dev.h, and those have hard-coded limits: the 64-bit
key reduced over a wave as two 32-bit halves, kSelLaneW = 4 words kept in a
lane (the fourth component of a 16-B store), the 64-word block of the
lane-per-word path, and 16 bits per slot for a root's link counts. Every
fixture below sits on one of them:

  L1  keys with bit 31 set in either half, thresholds with bit 31 set, on the
      lane-per-announcer and the lane-per-word path;
  L2  a root of exactly four next-hop words beside one of five;
  L3  a root of 66 words;
  L4  65,535 and 65,536 parallel links between two nodes.

The expectation is selpolicy_ref.expect / srmpls_ref.expect / policy_delta_ref
over the CPU oracle's SPF and the CSR columns -- never the engine's rows or its
key -- and every case states, as an assert on that expectation, the property
that makes it a limit case (preconditions), so that a later change to a
fixture cannot silently turn the case into an ordinary one. The only place a
packed key appears is l1_wrong_kernel: a model of four WRONG kernels, used to
show that the fixture tells them from the right one."""
import functools
from types import SimpleNamespace

import numpy as np

import policy_delta_ref as PD
import seldelta_ref as D
import selpolicy_ref as PR
import srmpls_ref as SR
from graphs import metric_graph

INF = 0xFFFFFFFF
M31 = 0x7FFFFFFF     # the largest metric an adjacency admits (an i32)
B31 = 0x80000000
TOP = 2 ** 31 - 1    # the worst class rank: with the drained bit the key's high word is 0xFFFFFFFF


class Case(SimpleNamespace):
    """name; versions (seldelta_ref.Version: [0] the graph, [1] the graph after
    the state's update, when there is one); table / pref / mnh / flags per
    prefix (ids ascending); roots: the judged node ids (None: all); focus:
    {role: node id} of the nodes the case is about"""

    @property
    def base(self):
        return self.versions[0]

    @property
    def judged(self):
        return list(range(self.base.V)) if self.roots is None else list(self.roots)

    def pol(self, W, version=0):
        """selpolicy_ref.expect's dict at output width W (kept)"""
        key = ("pol", W, version)
        if key not in self._kept:
            self._kept[key] = PD.expect(self.versions[version], self.table, self.pref, self.mnh, W,
                                        roots=self.roots)
        return self._kept[key][0]

    def sr(self, W):
        """(srmpls_ref.expect's dict, facts) at output width W (kept)"""
        key = ("sr", W)
        if key not in self._kept:
            v = self.base
            self._kept[key] = SR.expect(v.spf(True, self.roots), v.names, v.csr, self.table,
                                        self.pref, self.mnh, self.flags, W, roots=self.roots)
        return self._kept[key]

    def delta(self, W, before=0, after=1):
        """the expected update between two versions -> (changed, rebased, ea, eb);
        only judged roots are in `changed`"""
        eb, ea = self.pol(W, before), self.pol(W, after)
        vb, va = self.versions[before], self.versions[after]
        rebased = [r for r in range(vb.V) if vb.nbrs(r) != va.nbrs(r)]
        keep = set(self.judged)
        changed = {c for c in PD.diff(eb, ea, rebased) if c[0] in keep}
        return changed, rebased, ea, eb


def make(name, versions, rows, roots=None, focus=()):
    """rows: per prefix [(node name, class rank, threshold, flag)], any order"""
    ids = {nm: i for i, nm in enumerate(versions[0].names)}
    assert all(v.names == versions[0].names for v in versions)
    table, pref, mnh, flags = [], [], [], []
    for ents in rows:
        ents = sorted((ids[nm], c, m, f) for nm, c, m, f in ents)
        assert len({e[0] for e in ents}) == len(ents), "a node twice in a prefix"
        table.append([e[0] for e in ents])
        pref.append([e[1] for e in ents])
        mnh.append([e[2] for e in ents])
        flags.append([e[3] for e in ents])
    return Case(name=name, versions=versions, table=table, pref=pref, mnh=mnh, flags=flags,
                roots=None if roots is None else sorted(ids[r] for r in roots),
                focus={r: ids[r] for r in focus}, ids=ids, _kept={})


def words_of(version, r):
    return max(1, (len(version.nbrs(r)) + 31) // 32)


def hub_links(c, root, p, W):
    """the links of `root`'s next hops of prefix p, from the expectation's
    words and the CSR's link counts"""
    v = c.base
    nb, cnt = v.nbrs(root), PR.link_counts(v.csr, root, False)
    return sum(cnt[k] for k in PR.decode(c.pol(W)["nh"][root, p], nb))


# ---------------------------------------------------------------- L1
L1_SPOKES, L1_CLUSTER = 129, 140
L1_DRAINED = ("k001", "k064", "k070", "k129", "d005", "s100")
L1_ROWS = ("high-words", "class-bit-31", "mixed-distances")
L1_WRONG = ("low half signed", "high half signed", "low half first", "signed max")


def spoke(j):
    """a's stub spokes: the first 64 sort before the cluster, the rest behind it"""
    return f"d{j:03d}" if j < 64 else f"s{j:03d}"


def l1_dbs():
    """a with 129 stub spokes (1 + j % 3 out, 1 back), a1 and b: 131 distinct
    neighbours, five words. a1 hangs off a at 1 (one word). a -> b costs
    0x7FFFFFFF (1 back) and b -> c 6 (1 back): c is at 0x80000005 from a, and
    the 140 cluster nodes behind c (1 + i % 5 out, 1 back) at 0x80000006 and
    above; the way back costs 1 a hop, so the distance bound stays below
    2^32 - 1. Some cluster nodes and two spokes are drained."""
    links = [("a", "a1", 1, 1), ("a", "b", M31, 1), ("b", "c", 6, 1)]
    links += [("a", spoke(j), 1 + j % 3, 1) for j in range(L1_SPOKES)]
    links += [("c", f"k{i:03d}", 1 + i % 5, 1) for i in range(L1_CLUSTER)]
    return metric_graph(links, overloaded=L1_DRAINED)


def l1_rows():
    """The rows of test_key_edges_unsigned_and_high_word_first, each as a
    prefix of 9, 65 and 130 announcers with ONE deciding announcer: in lane 0,
    in a middle lane, and at entry index >= 64 (a lane's second key, the second
    trip of the pass-2 walks). Then the two self-prepend prefixes.

    high-words: the winner alone at rank 2^31 - 2, far (>= 2^31); the losers at
      rank 2^31 - 1, one of them drained (its high word is kNoKey's), some near.
    class-bit-31: the winner alone at rank 1, far; the losers at rank 2^30
      (bit 31 of the high word), some near.
    mixed-distances: one class; the winner is the only spoke at distance 1 from
      a, beside spokes at 2 and 3 and cluster nodes at 2^31 and above. Its S'
      is the undrained rest: the thresholds 0x80000000 beside 5 and 0xFFFFFFFF
      sit there, outside L; a drained loser carries 0xFFFFFFFF where it must
      not count."""
    d = lambda js: [spoke(j) for j in js]                           # noqa: E731
    k = lambda lo, hi: [f"k{i:03d}" for i in range(lo, hi)]         # noqa: E731
    far3 = lambda js: [j for j in js if j % 3]                      # noqa: E731 (spokes not at 1)
    flag = lambda nm: int(nm[1:]) % 2 if nm[1:].isdigit() else 0    # noqa: E731

    def row(winner, losers, wrank, lrank, wneed, needs):
        ents = [(winner, wrank, wneed, flag(winner))]
        ents += [(nm, lrank, needs.get(nm, 0), flag(nm)) for nm in losers]
        return ents

    rows = []
    # high-words
    for winner, losers in (
            ("c", d([1, 2]) + k(1, 4) + d([64, 65, 66])),
            ("k000", d(range(30)) + k(1, 21) + d(range(64, 78))),
            ("k010", d(range(64)) + k(0, 10) + k(11, 41) + d(range(64, 89)))):
        rows.append(row(winner, losers, TOP - 1, TOP, 2, {"k002": INF, "d001": 7}))
    # class-bit-31
    for winner, losers in (
            ("b", ["c"] + d([3, 4]) + k(6, 8) + d([70, 71, 72])),
            ("k050", d(range(32)) + k(51, 71) + d(range(80, 92))),
            ("k040", d(range(64)) + k(20, 40) + k(41, 61) + d(range(90, 115)))):
        rows.append(row(winner, losers, 1, 2 ** 30, 3, {"d003": INF, "k055": INF, "k030": B31}))
    # mixed-distances
    for winner, losers, needs in (
            ("d000", d([1, 2]) + k(1, 4) + d([64, 65, 67]),
             {"k001": INF, "k002": B31, "d001": 5}),
            ("d030", d(far3(range(1, 41))) + k(0, 31) + d(far3(range(64, 72))),
             {"k001": B31, "k010": INF, "d002": 5}),
            ("s066", d(far3(range(64))) + k(0, 62) + d(far3(range(64, 101))),
             {"d001": B31, "s070": INF, "k003": 5, "k001": 9})):
        rows.append(row(winner, losers, 7, 7, 0, needs))
    # the root's own entry with a prepend label, alone in the best class
    for own, rest, need in (("a", ["b", "c"] + d([10, 11]) + k(20, 22) + d([100, 101]), 1),
                            ("a1", ["b", "c"] + d([12, 13]) + k(22, 24) + d([102, 103]), 0)):
        rows.append([(own, 0, need, 1)] + [(nm, 1, 3, flag(nm)) for nm in rest])
    return rows


L1_SELF = {"a": 9, "a1": 10}  # the self-prepend prefixes of l1_rows


def l1_keys(c, root, p):
    """per entry of prefix p (high word, low word) of the 64-bit key as the
    root sees it, None when unreached -- from the oracle's distances"""
    v = c.base
    res = v.spf(True, [root])[v.names[root]]
    drained = np.asarray(v.csr["no_transit"]).astype(bool)
    out = []
    for a, rank in zip(c.table[p], c.pref[p]):
        nm = v.names[a]
        out.append((rank << 1 | int(drained[a]), res[nm][0]) if nm in res else None)
    return out


def l1_wrong_kernel(c, root, p, wrong=None):
    """(metric, best, need) of (root, prefix p) from a kernel whose wave
    reductions are wrong in one way (L1_WRONG; None: the right kernel). The
    lanes fold their own keys (entries lane, lane + 64, ...) as the kernel
    does, unsigned; idle lanes hold kNoKey; then the wave reduces."""
    s32 = lambda x: x - (1 << 32) if x >= B31 else x  # noqa: E731
    keys = l1_keys(c, root, p)
    lanes = [(INF, INF)] * 64
    for i, key in enumerate(keys):
        if key is not None:
            lanes[i % 64] = min(lanes[i % 64], key)
    his, los = [h for h, _ in lanes], [lo for _, lo in lanes]
    if wrong == "low half first":
        lo = min(los)
        hi = min(h if l == lo else INF for h, l in lanes)
    else:
        hi = min(his, key=s32 if wrong == "high half signed" else None)
        lo = min((l if h == hi else INF for h, l in lanes),
                 key=s32 if wrong == "low half signed" else None)
    if (hi, lo) == (INF, INF):
        return INF, INF, 0
    S = [i for i, key in enumerate(keys) if key is not None and key[0] >> 1 == hi >> 1]
    Sf = [i for i in S if keys[i][0] == hi]
    s_ids = [c.table[p][i] for i in S]
    best = root if root in s_ids else min(s_ids, default=INF)
    need = [0] * 64  # the lanes' shares, then the wave's maximum
    for i in Sf:
        need[i % 64] = max(need[i % 64], c.mnh[p][i])
    return lo, best, max(need, key=s32 if wrong == "signed max" else None)


def l1_preconditions(c):
    v = c.base
    a, a1 = c.focus["a"], c.focus["a1"]
    assert words_of(v, a) == 5 and words_of(v, a1) == 1
    e = c.pol(5)
    for r in (a, a1):
        res = v.spf(True, [r])[v.names[r]]
        assert all(res[spoke(j)][0] < B31 for j in range(L1_SPOKES))
        assert all(res[f"k{i:03d}"][0] >= B31 for i in range(L1_CLUSTER)) and res["c"][0] >= B31
    assert v.spf(True, [a1])["a1"]["b"][0] == B31
    # the deciding announcer: lane 0, a middle lane, the second trip
    for g in range(3):
        for n, p, at in zip((9, 65, 130), range(3 * g, 3 * g + 3), (0, None, None)):
            assert len(c.table[p]) == n
            for r in (a, a1):
                assert e["count"][r, p] == 1, (L1_ROWS[g], n)
                res = v.spf(True, [r])[v.names[r]]
                won = [i for i, x in enumerate(c.table[p]) if res[v.names[x]][0] == e["metric"][r, p]
                       and (c.pref[p][i] << 1 | int(v.csr["no_transit"][x])) ==
                       min(q << 1 | int(v.csr["no_transit"][y]) for q, y in zip(c.pref[p], c.table[p]))]
                assert len(won) == 1
                assert (won[0] == 0) if n == 9 else (0 < won[0] < 64) if n == 65 else won[0] >= 64
    # the thresholds with bit 31 set are in S', outside L, and decide need
    assert [int(e["need"][a, p]) for p in (6, 7, 8)] == [B31, INF, INF]
    assert [int(e["need"][a1, p]) for p in (6, 7, 8)] == [B31, INF, INF]
    assert all(e["metric"][a, p] >= M31 and e["metric"][a1, p] >= B31 for p in range(6))
    assert sum(e["metric"][a, p] >= B31 for p in range(6)) == 5  # b is at 0x7FFFFFFF from a
    assert all(e["metric"][a, p] == 1 and e["metric"][a1, p] == 2 for p in (6, 7, 8))
    # the model is the rule: right, it is the expectation; wrong in any of the
    # four ways, it changes a cell of root a and one of root a1
    P = len(c.table)
    for r in (a, a1):
        want = [(int(e["metric"][r, p]), int(e["best"][r, p]), int(e["need"][r, p])) for p in range(P)]
        assert [l1_wrong_kernel(c, r, p) for p in range(P)] == want
        for wrong in L1_WRONG:
            hit = [p for p in range(P) if l1_wrong_kernel(c, r, p, wrong) != want[p]]
            assert hit, (wrong, v.names[r])
            # and on a prefix that fills every lane, where kNoKey in an idle
            # lane is not what gives the wrong kernel away
            assert any(len(c.table[p]) == 130 for p in hit), (wrong, v.names[r])
    # SR_MPLS: the root's flagged entry is all of S', D is empty
    s, facts = c.sr(5)
    assert facts["rule1208_fired"] == 0 and facts["self_prepend_only"] >= 2
    for nm, r in (("a", a), ("a1", a1)):
        p = L1_SELF[nm]
        assert len(c.table[p]) == 9 and c.table[p][0] == r and c.flags[p][0] == 1
        assert (s["metric"][r, p], s["count"][r, p], s["best"][r, p]) == (INF, 0, r)
        assert s["need"][r, p] == c.mnh[p][0] and e["metric"][r, p] == 0


def l1():
    return make("L1", [D.Version(l1_dbs())], l1_rows(), focus=("a", "a1"))


# ---------------------------------------------------------------- L2
L2_DRAINED = ("p003", "p097", "p120")


def l2_dbs(bump=False, moved=False):
    """h4 (and its twin g4) with the 128 neighbours p000 .. p127: four words;
    h5 with p000 .. p128: five. h4 - p<k> costs 1 + k % 2, the other hubs'
    links 2. p100 (slot 100 of h4) has a second link at its first one's metric,
    p110 a second one at 3 against 1. y hangs behind p101 and p102 at 1; bump:
    the link y - p102 costs 2. z hangs behind p106 and p108 at 1 and behind
    p112 at 2 (h4 reaches all three at 1, over one link each); moved: z - p106
    costs 2 and z - p112 costs 1, so h4 reaches z through p108 and p112 instead
    of p106 and p108: the same metric, count and links, another word 3. g4 is
    there so that a sweep over half the roots can own a four-word root without
    the five-word one."""
    p = [f"p{k:03d}" for k in range(129)]
    links = [("h4", p[k], 1 + k % 2, 1 + k % 2) for k in range(128)]
    links += [("g4", p[k], 2, 2) for k in range(128)]
    links += [("h5", p[k], 2, 2) for k in range(129)]
    links += [("h4", "p100", 1, 1), ("h4", "p110", 3, 3)]
    links += [("y", "p101", 1, 1), ("y", "p102", 2 if bump else 1, 2 if bump else 1)]
    a, b = (2, 1) if moved else (1, 2)
    links += [("z", "p106", a, a), ("z", "p108", 1, 1), ("z", "p112", b, b)]
    return metric_graph(links, overloaded=L2_DRAINED)


L2_Y, L2_P100, L2_P110, L2_SHORT, L2_HUBS, L2_LONG, L2_Z = 0, 1, 2, 4, 5, 6, 8


def l2_rows():
    """prefixes of 1, 8, 9 and 65 announcers, an empty one, z's, then single
    spokes up to P = 65: a chunk of 64 prefixes and a tail of one"""
    def ents(names, p):
        out = []
        for nm in names:
            n = int(nm[1:]) if nm[0] == "p" else 0
            out.append((nm, (n + p) % 2, (3 * n + p) % 4, 1 if nm[0] in "gh" else (n + p) % 2))
        return out

    rows = [["y"], ["p100"], ["p110"], ["p096"],
            ["p005", "p040", "p070", "p097", "p098", "p104", "p126", "p127"],
            ["g4", "h4", "h5", "p001", "p033", "p099", "p100", "p110", "p125"],
            [f"p{k:03d}" for k in range(60, 125)], [], ["z"]]
    rows += [[f"p{k:03d}"] for k in range(56)]
    assert len(rows) == 65
    return [ents(names, p) for p, names in enumerate(rows)]


def l2_preconditions(c):
    v = c.base
    h4, h5, g4 = c.focus["h4"], c.focus["h5"], c.focus["g4"]
    assert (words_of(v, h4), words_of(v, g4), words_of(v, h5)) == (4, 4, 5) and v.words == 5
    assert v.nbrs(h4) == [c.ids[f"p{k:03d}"] for k in range(128)]  # slot k is p<k>
    assert len(c.table) == 65 and [len(c.table[p]) for p in (0, 4, 5, 6)] == [1, 8, 9, 65]
    e = c.pol(5)
    assert not e["nh"][h4, :, 4].any()
    short = [p for p in range(65) if len(c.table[p]) <= 8 and e["nh"][h4, p, 3]]
    long = [p for p in range(65) if len(c.table[p]) > 8 and e["nh"][h4, p, 3]]
    assert L2_SHORT in short and L2_P100 in short and {L2_HUBS, L2_LONG} & set(long), (short, long)
    # a slot >= 96 whose count is 2, and the unequal pair beside it
    cnt = PR.link_counts(v.csr, h4, False)
    assert cnt[c.ids["p100"]] == 2 and cnt[c.ids["p110"]] == 1
    assert PR.link_counts(v.csr, h4, True)[c.ids["p110"]] == 2
    assert e["links"][h4, L2_P100] == 2 == hub_links(c, h4, L2_P100, 5)
    assert e["links"][h4, L2_P110] == 1
    assert e["links"][h4, L2_LONG] == hub_links(c, h4, L2_LONG, 5) > e["count"][h4, L2_LONG]
    # SR_MPLS: per-entry rows with word 3 in use
    s, facts = c.sr(5)
    assert facts["rule1208_fired"] == 0 and s["dst_nh"][h4, :, 3].any()
    # the update: a record of h4 whose words differ in word 3 (and are not zero there)
    changed, rebased, ea, eb = c.delta(5)
    assert not rebased and (h4, L2_Y) in changed
    assert eb["nh"][h4, L2_Y, 3] != ea["nh"][h4, L2_Y, 3] and ea["nh"][h4, L2_Y, 3]
    assert (eb["nh"][h4, L2_Y, :3] == ea["nh"][h4, L2_Y, :3]).all()
    assert 0 < len(changed) < v.V * 65
    # the second update: a record of h4 that keeps its header and differs in
    # word 3 only -- nothing but the kernel's word-3 compare reports it
    changed, rebased, ea, eb = c.delta(5, 1, 2)
    assert not rebased and (h4, L2_Z) in changed and (g4, L2_Z) in changed
    for k in PD.COLS:
        assert eb[k][h4, L2_Z] == ea[k][h4, L2_Z], k
    assert (ea["metric"][h4, L2_Z], ea["count"][h4, L2_Z], ea["links"][h4, L2_Z]) == (2, 1, 2)
    assert np.nonzero(eb["nh"][h4, L2_Z] != ea["nh"][h4, L2_Z])[0].tolist() == [3]
    assert (int(eb["nh"][h4, L2_Z, 3]), int(ea["nh"][h4, L2_Z, 3])) == \
        (1 << 10 | 1 << 12, 1 << 12 | 1 << 16)


def l2():
    return make("L2", [D.Version(l2_dbs()), D.Version(l2_dbs(bump=True)),
                       D.Version(l2_dbs(bump=True, moved=True))], l2_rows(),
                focus=("g4", "h4", "h5"))


# ---------------------------------------------------------------- L3
L3_SPOKES = 2100
L3_ROOTS = ("hub", "s0000", "s0010", "s2050", "s2052", "s2099", "x")
L3_X, L3_EQUAL, L3_UNEQUAL = 0, 1, 2


def l3_dbs(moved=False):
    """seldelta_ref.star_dbs(2100, ring=False)'s shape with the metrics pinned:
    the hub with 2,100 spokes (66 words) at 1 + i % 3, but s2050 .. s2052 at 1;
    s2060 (slot >= 2048) over two links at 2, s2070 over one at 1 and one at 3;
    x behind s2050 and s2051 at 1 and behind s2052 at 2. moved: x - s2050 costs
    2 and x - s2052 costs 1, so the hub reaches x through s2051 and s2052
    instead of s2050 and s2051: the same metric, count and links, another word
    64."""
    s = [f"s{i:04d}" for i in range(L3_SPOKES)]
    special = {2050: 1, 2051: 1, 2052: 1, 2060: 2, 2070: 1}
    links = [("hub", s[i], special.get(i, 1 + i % 3), special.get(i, 1 + i % 3))
             for i in range(L3_SPOKES)]
    links += [("hub", s[2060], 2, 2), ("hub", s[2070], 3, 3)]
    a, b = (2, 1) if moved else (1, 2)
    links += [("x", s[2050], a, a), ("x", s[2051], 1, 1), ("x", s[2052], b, b)]
    return metric_graph(links)


def l3_rows():
    """25 announcer entries: dst_nh of 2,102 roots at 130 words stays below 30 MB"""
    names = [["x"], ["s2060"], ["s2070"], ["s0005"],
             ["s0001", "s0040", "s1000", "s2047", "s2048", "s2060", "s2070", "s2099", "x"],
             ["hub", "s0000", "s0010", "s0031", "s0064", "s2049", "s2050", "s2051", "s2052",
              "s2080", "s2090", "x"], []]
    rows = []
    for p, nms in enumerate(names):
        rows.append([(nm, (i + p) % 2 if len(nms) > 1 else 0, (i * 3 + p) % 4,
                      1 if nm in ("hub", "x") else i % 2) for i, nm in enumerate(nms)])
    return rows


def l3_preconditions(c):
    v, w = c.versions
    hub = c.focus["hub"]
    assert words_of(v, hub) == 66 == v.words and v.V == L3_SPOKES + 2
    assert v.nbrs(hub) == [c.ids[f"s{i:04d}"] for i in range(L3_SPOKES)]  # slot i is s<i>
    assert sum(len(a) for a in c.table) <= 40
    e = c.pol(66)
    assert e["nh"][hub, :, 64:].any()
    s, facts = c.sr(66)
    assert facts["rule1208_fired"] == 0 and s["dst_nh"][hub, :, 64:].any()
    cnt = PR.link_counts(v.csr, hub, False)
    assert cnt[c.ids["s2060"]] == 2 and cnt[c.ids["s2070"]] == 1
    assert e["links"][hub, L3_EQUAL] == 2 and e["links"][hub, L3_UNEQUAL] == 1
    assert e["nh"][hub, L3_EQUAL].tolist() == [0] * 64 + [1 << 12, 0]
    # the update: the hub's [x] entry keeps its header and changes word 64 only
    changed, rebased, ea, eb = c.delta(66)
    assert not rebased, "a rebased root"
    assert (hub, L3_X) in changed
    for k in PD.COLS:
        assert eb[k][hub, L3_X] == ea[k][hub, L3_X], k
    assert (ea["metric"][hub, L3_X], ea["count"][hub, L3_X], ea["links"][hub, L3_X]) == (2, 1, 2)
    differ = np.nonzero(eb["nh"][hub, L3_X] != ea["nh"][hub, L3_X])[0].tolist()
    assert differ == [64]
    assert (int(eb["nh"][hub, L3_X, 64]), int(ea["nh"][hub, L3_X, 64])) == (0b01100, 0b11000)


def l3():
    return make("L3", [D.Version(l3_dbs()), D.Version(l3_dbs(moved=True))], l3_rows(),
                roots=L3_ROOTS, focus=("hub", "x"))


# ---------------------------------------------------------------- L4
L4_FITS, L4_OVER = 65535, 65536  # OSPF_MAX_PARALLEL_LINKS and one more


def l4_dbs(n):
    """r = x over n parallel up links of metric 1, x - t"""
    return metric_graph([("r", "x", 1, 1)] * n + [("x", "t", 1, 1)])


def l4_rows():
    return [[("x", 0, 0, 0)], [("t", 0, L4_FITS, 0)], [("t", 0, L4_OVER, 0), ("x", 1, 0, 1)],
            [("r", 0, 0, 1), ("t", 0, 0, 0)]]


def l4_preconditions(c):
    v = c.base
    n = L4_OVER if c.name == "L4-65536" else L4_FITS
    r, t, x = c.focus["r"], c.focus["t"], c.focus["x"]
    assert v.names == ["r", "t", "x"] and v.nbrs(r) == [x]
    assert PR.link_counts(v.csr, r, False) == {x: n} == PR.link_counts(v.csr, r, True)
    e = c.pol(1)
    assert e["links"][r].tolist() == [n, n, n, 0] and e["metric"][r].tolist() == [1, 2, 2, 0]
    # a threshold of 65,535 is met by both, one of 65,536 only by the larger group
    assert e["installed"][r].tolist() == [True, True, n >= L4_OVER, False]
    s, _ = c.sr(1)
    assert s["links"][r].tolist() == [n, n, n, n]  # the flagged root routes to t
    assert s["dst_links"][r].tolist() == [n, n, n, 0, 0, n]
    assert e["links"][x].tolist() == [0, 1, 1, n + 1]


def l4(n):
    return make(f"L4-{n}", [D.Version(l4_dbs(n))], l4_rows(), focus=("r", "t", "x"))


# ---------------------------------------------------------------- the cases
CASES = {"L1": l1, "L2": l2, "L3": l3, "L4-65535": lambda: l4(L4_FITS),
         "L4-65536": lambda: l4(L4_OVER)}


def preconditions(c):
    {"L1": l1_preconditions, "L2": l2_preconditions, "L3": l3_preconditions}.get(
        c.name, l4_preconditions)(c)


@functools.lru_cache(maxsize=None)
def case(name):
    """a fixture with its table and expectations (built once, never changed);
    its preconditions have held"""
    c = CASES[name]()
    preconditions(c)
    return c


# ---------------------------------------------------------------- the product's faces
def rank_attrs(rank):
    """(path preference, source preference, distance) of class rank `rank`:
    the larger path preference wins"""
    return (TOP - rank, 0, 0)


def policy_prefixes(c):
    """the table in LinkState.all_sources_select_policy's form"""
    names = c.base.names
    return {f"p{p}": [(names[a],) + rank_attrs(k) + (m or None,)
                      for a, k, m in zip(ann, c.pref[p], c.mnh[p])]
            for p, ann in enumerate(c.table)}


def srmpls_prefixes(c):
    names = c.base.names
    return {f"p{p}": [(names[a],) + rank_attrs(k) + (m or None, bool(f))
                      for a, k, m, f in zip(ann, c.pref[p], c.mnh[p], c.flags[p])]
            for p, ann in enumerate(c.table)}
