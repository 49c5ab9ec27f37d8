"""The multi-area selection at its area and entry limits: explicit graphs,
their tables and their oracle-derived expectation (shared by
test_host_areas_limits.py and test_gpu_areas_limits.py).

The multi-area kernels (areas_kernel, areas_delta_kernel and the device
functions of spf_selareas_dev.h) have hard-coded limits: 32 areas behind a u32
mask built with 1u << a, the 64-entry step of walk 4 with its carry across
steps, unsigned metrics compared across areas, the packed link counts of a
root's areas one after the other, the 16-B store of a 4-word root and the class
word 0xFFFFFFFF beside kNoKey's. Every fixture below sits on one of them. The
expectation is areas_ref.expect over the CPU oracle's SPF of every area --
never the engine's rows or its key -- and every case states, as an assert on
that expectation, the property that makes it a limit case (the
*_preconditions functions), so that a later change to a fixture cannot
silently turn the case into an ordinary one.

An area is areas_ref's dict {names, csr, spf} with its name, its AdjDbs and a
host-path LinkState beside them. Areas are built once per (name, links,
overloaded) and shared between the groups: an unchanged area of two versions
is the same dict object."""
import functools
from types import SimpleNamespace

import numpy as np

import areas_ref as AR
from graphs import metric_graph
from openr_amd.adjdb import AdjDbStream
from openr_amd.linkstate import LinkState, root_neighbor_ids
from oracle import Oracle, parse_spf_text
from selpolicy_ref import link_counts

FF = 0xFFFFFFFF
M31 = 0x7FFFFFFF       # the largest metric an adjacency admits (an i32)
FAR = 0x80000005       # y from x in a heavy area: M31 + 6
TOP = 2 ** 31 - 1      # the worst class rank: with the drained bit the class word is FF
N_AREAS = 32
TAIL = 5               # u0 .. u4 behind y in the heavy areas
N_FILL = 48            # f00 .. f47, one per area round-robin
N_FILL2 = 20           # g00 .. g19 likewise: only the 129-entry prefix needs them
N_SPOKES = 130


@functools.lru_cache(maxsize=None)
def _area(name, links, overloaded):
    dbs = metric_graph(list(links), overloaded)
    st = AdjDbStream.from_dbs(dbs)
    ls = LinkState(area=name)
    ls.set_host_spf(True)
    ls.apply(st)
    names, csr = ls.node_names(), ls.csr()
    orc = Oracle(st)
    spf = {r: parse_spf_text(orc.spf_text(r, True)) for r in names}
    return dict(name=name, ls=ls, names=names, csr=csr, spf=spf, dbs=dbs)


def area(name, links, overloaded=()):
    return _area(name, tuple(tuple(ln) for ln in links), tuple(sorted(overloaded)))


def words(areas):
    """per area the widest root's next-hop words"""
    return tuple(max(1, max((root_neighbor_ids(a["csr"], r).size + 31) // 32
                            for r in range(len(a["names"])))) for a in areas)


def gid_of(areas):
    return {n: i for i, n in enumerate(AR.union(areas)[0])}


# ---------------------------------------------------------------- F32
def f32_links(i, first=None, heavy=False, solo=False, fill=False, spokes=None, down=False):
    """area i of F32: x - s<i> - y with 1 + i % 3 (or `first`) on the first link
    and 2 on the second. heavy: x -(M31 out, 1 back)- s -(6 out, 1 back)- y and
    u0 .. u4 behind y, everything from y on at 2^31 and above from x; solo: q
    behind s, in this area only; fill: the private fillers of the area behind
    y at 5; spokes: a tag, N_SPOKES more neighbours of x; down: the first link
    reported down"""
    s = f"s{i:02d}"
    m = 1 + i % 3 if first is None else first
    if heavy:
        links = [("x", s, M31, 1), (s, "y", 6, 1)]
        links += [("y", f"u{k}", 1 + k, 1) for k in range(TAIL)]
    else:
        links = [("x", s, m, m) + (("down",) if down else ()), (s, "y", 2, 2)]
    if solo:
        links.append((s, "q", 1, 1))
    if fill:
        links += [("y", f"f{j:02d}", 5, 5) for j in range(N_FILL) if j % N_AREAS == i]
        links += [("y", f"g{j:02d}", 5, 5) for j in range(N_FILL2) if j % N_AREAS == i]
    if spokes:
        links += [("x", f"{spokes}{k:03d}", 1, 1) for k in range(N_SPOKES)]
    return links


def f32_area(i, **kw):
    return area(f"a{i:02d}", f32_links(i, **kw))


WIDE = {5: "h", 6: "k"}  # x's wide areas in the wide straddle group, and their spokes' tags


def f32(variant="plain"):
    """the 32 areas a00 .. a31 (name order is index order) of a variant:
    plain; uniform (every area 1 + 2: all of them tie); heavy (areas 30 and 31
    heavy); solo (q in area 31 only); fill (the fillers); fillwide (the fillers,
    and x with N_SPOKES more neighbours in areas 5 and 6: area 5 loses under
    F32's metrics and area 6 wins, so walk 4 by words runs in an area whose
    link counts are not the first of the packed ones, beside a wide area that
    is written as zeros)"""
    kw = {
        "plain": lambda i: {},
        "uniform": lambda i: dict(first=1),
        "heavy": lambda i: dict(heavy=i >= 30),
        "solo": lambda i: dict(solo=i == 31),
        "fill": lambda i: dict(fill=True),
        "fillwide": lambda i: dict(fill=True, spokes=WIDE.get(i)),
    }[variant]
    return [f32_area(i, **kw(i)) for i in range(N_AREAS)]


def f32_table(areas):
    """case 1's prefixes: y into all 32 areas; into area 31 only; into areas 0
    and 31 with the better class in 31; into every area with thresholds, the
    largest in area 1 (a losing area wherever the areas differ); the same with
    a threshold no root's links reach; the own prefix of q (of s31 where there
    is no q); an empty one"""
    g = gid_of(areas)
    y, own = g["y"], g.get("q", g["s31"])
    every = range(N_AREAS)
    return [[(y, a, 0, 0) for a in every],
            [(y, 31, 0, 0)],
            [(y, 0, 1, 0), (y, 31, 0, 0)],
            [(y, a, 0, 5 if a == 1 else a % 3) for a in every],
            [(y, a, 0, 40 if a == 2 else 0) for a in every],
            [(own, 31, 0, 1)],
            []]


HEAVY_AT = 7  # where heavy_table's prefixes start behind f32_table's


def heavy_table(areas):
    """case 2's prefixes behind f32_table's: y into areas 0 and 31 (3 against
    FAR, by the lane); into the heavy areas 30 and 31 only (both at FAR); into
    every area but 30 (31 entries: by the wave); y and the tail into both heavy
    areas (12 entries, nothing below 2^31: by the wave); the tail alone; u0 into
    area 31 alone"""
    g = gid_of(areas)
    y, u = g["y"], [g[f"u{k}"] for k in range(TAIL)]
    tail = [(n, a, 0, 0) for n in u for a in (30, 31)]
    return f32_table(areas) + [
        [(y, 0, 0, 0), (y, 31, 0, 0)],
        [(y, 30, 0, 0), (y, 31, 0, 0)],
        [(y, a, 0, 0) for a in range(N_AREAS) if a != 30],
        tail + [(y, 30, 0, 0), (y, 31, 0, 0)],
        tail,
        [(u[0], 31, 0, 2)]]


def popcount(x):
    return bin(int(x)).count("1")


def only_area(areas, a):
    """the global ids of the nodes that area a alone holds"""
    _, gids = AR.union(areas)
    held = np.zeros(len(AR.union(areas)[0]), np.uint32)
    for gs in gids:
        held[gs] += 1
    return [int(g) for g in gids[a] if held[g] == 1]


def f32_preconditions(c, variant):
    """bit 31 of the mask, a root whose only area is 31, and per variant the
    cells it was made for"""
    e, g = c.exp, gid_of(c.areas)
    x = g["x"]
    assert len(c.areas) == N_AREAS == 32
    assert [a["name"] for a in c.areas] == sorted(a["name"] for a in c.areas)
    assert (e["areas"] >> 31).any(), "bit 31 of the mask is never set"
    assert only_area(c.areas, 31), "no root whose only area is 31"
    assert e["areas"][x, 1] == 0x80000000 and e["nh"][31][c.areas[31]["names"].index("x"), 1].any()
    assert e["areas"][x, 2] == 0x80000000, "the better class in area 31 does not win"
    if variant == "uniform":
        assert e["areas"][x, 0] == FF and e["count"][x, 0] == 32 and e["links"][x, 0] == 32
        assert e["metric"][x, 0] == 3
    if variant in ("plain", "solo"):
        assert e["areas"][x, 0] == 0x49249249 and c.facts["need_from_loser"] > 0
        assert c.facts["withheld"] > 0
    if variant == "solo":
        q = g["q"]
        assert only_area(c.areas, 31) == sorted([q, g["s31"]])
        assert e["areas"][q, 0] == 0x80000000 and e["metric"][x, 5] == 3
    if variant == "heavy":
        assert e["metric"][x, 1] == FAR and e["areas"][x, 1] == 0x80000000


def heavy_preconditions(c):
    """a metric at or above 2^31 that loses to a smaller one, two that tie, and
    which cell a signed compare gets wrong -- from the oracle's numbers"""
    e, g, h = c.exp, gid_of(c.areas), HEAVY_AT
    x = g["x"]
    for a in (30, 31):
        spf = c.areas[a]["spf"]["x"]
        assert spf["y"][0] == FAR and spf[f"s{a}"][0] == M31 and spf["u0"][0] == FAR + 1
    assert c.areas[0]["spf"]["x"]["y"][0] == 3
    # 3 against FAR: as i32 FAR is negative, so a signed compare takes area 31
    assert int(np.uint32(FAR).astype(np.int32)) < 3 < FAR
    assert (e["metric"][x, h], e["areas"][x, h], e["count"][x, h]) == (3, 1, 1)
    assert (e["metric"][x, h + 1], e["areas"][x, h + 1], e["count"][x, h + 1]) == (FAR, 0xC0000000, 2)
    assert len(c.table[h + 2]) == 31 and e["metric"][x, h + 2] == 3
    assert e["areas"][x, h + 2] == 0x09249249  # the areas i % 3 == 0 below 30
    assert len(c.table[h + 3]) == 12
    assert (e["metric"][x, h + 3], e["areas"][x, h + 3], e["count"][x, h + 3]) == (FAR, 0xC0000000, 2)
    assert e["metric"][x, h + 4] == FAR + 1 and e["areas"][x, h + 4] == 0xC0000000
    assert e["metric"][x, h + 5] == FAR + 1 and e["areas"][x, h + 5] == 0x80000000


# ---------------------------------------------------------------- the straddle
STRADDLE_AT = (48, 33, 63, 32, 97)  # entries before y's 32; 32 is the control


def straddle_table(areas):
    """fillers first, then y's 32 entries at positions K .. K + 31 for K of
    STRADDLE_AT: the run lies across positions 63 / 64 (K = 48, 33, 63), ends at
    63 (K = 32, no straddle) or lies across 127 / 128 (K = 97, 129 entries). The
    entries before y are reached and never at the metric: f<even>, g* and s* in
    a worse class, f<odd> in y's class and farther. Last an 8-entry prefix with
    y in 3 areas (by its own lane on a narrow root)."""
    g = gid_of(areas)
    pre = [(g[f"f{j:02d}"], j % N_AREAS, 1 - j % 2, j % 3) for j in range(N_FILL)]
    pre += [(g[f"g{j:02d}"], j % N_AREAS, 1, 0) for j in range(N_FILL2)]
    pre += [(g[f"s{i:02d}"], i, 1, 1) for i in range(N_AREAS)]
    assert pre == sorted(pre) and len(pre) == 100
    run = [(g["y"], a, 0, 0) for a in range(N_AREAS)]
    table = [pre[:k] + run for k in STRADDLE_AT]
    table.append(pre[:5] + [(g["y"], a, 0, 0) for a in (0, 3, 6)])
    return table


def straddle_preconditions(c):
    """y's entries on both sides of a 64-entry step, and count == 1 per winning
    area for root x"""
    e, g = c.exp, gid_of(c.areas)
    x, y = g["x"], g["y"]
    for p, k in enumerate(STRADDLE_AT):
        ents = c.table[p]
        assert len(ents) == k + 32 and all(n == y for n, _, _, _ in ents[k:])
        cut = 128 if k == 97 else 64
        across = len(ents) > cut and ents[cut - 1][0] == y and ents[cut][0] == y
        assert across == (k != 32), k
        assert e["areas"][x, p] == 0x49249249, k
        assert e["count"][x, p] == popcount(e["areas"][x, p]) == 11, k
        assert e["metric"][x, p] == 3
    p = len(STRADDLE_AT)
    assert len(c.table[p]) == 8 and e["areas"][x, p] == 0b1001001 and e["count"][x, p] == 3
    if c.name == "straddle-wide":
        W = [(root_neighbor_ids(a["csr"], a["names"].index("x")).size + 31) // 32 for a in c.areas]
        assert [a for a, w in enumerate(W) if w > 4] == sorted(WIDE) and W[5] == W[6] == 5
        assert not e["areas"][x, 0] >> 5 & 1 and e["areas"][x, 0] >> 6 & 1


# ---------------------------------------------------------------- Fwide
def fwide_links(bump=False):
    """area 0: the hub with one neighbour; area 1: 140 spokes s000 .. s139 (5
    words); area 2: 170 spokes s130 .. s299 (6 words): ten spokes are in both.
    Every 7th (area 1) and every 5th (area 2) spoke has two equal parallel
    links, some spokes are linked in pairs, s135 is drained in area 1 only.
    bump: the hub's link to s204 in area 2 (at 1, no parallel link) costs 7 more"""
    sp1 = [f"s{i:03d}" for i in range(140)]
    sp2 = [f"s{i:03d}" for i in range(130, 300)]
    l0 = [("hub", "n0", 1, 1), ("n0", "n1", 2, 2)]
    l1 = [("hub", s, 1 + i % 3, 1 + i % 2) for i, s in enumerate(sp1)]
    l1 += [("hub", s, 1 + i % 3, 1 + i % 2) for i, s in enumerate(sp1) if i % 7 == 0]
    l1 += [(sp1[i], sp1[i + 1], 2, 2) for i in range(1, 61, 2)]
    l2 = [("hub", s, 1 + (i + 1) % 3 + (7 if bump and s == "s204" else 0), 1 + i % 2)
          for i, s in enumerate(sp2)]
    l2 += [("hub", s, 1 + (i + 1) % 3, 1 + i % 2) for i, s in enumerate(sp2) if i % 5 == 1]
    l2 += [(sp2[i], sp2[i + 1], 1, 2) for i in range(20, 90, 2)]
    return [(l0, ()), (l1, ("s135",)), (l2, ())]


def fwide(bump=False):
    base = fwide_links()
    return [area(f"a{i}", *(fwide_links(True)[i] if bump and i == 2 else base[i]))
            for i in range(3)]


FWIDE_ALL, FWIDE_ONLY2 = 4, 5  # fwide_table's prefixes the preconditions name


def fwide_table(areas):
    """prefixes of 1, 9, 65 and 130 entries over the spokes of both wide areas;
    every spoke of both; one only area 2 wins; the spoke drained in area 1 only
    from both areas; an empty one"""
    g = gid_of(areas)
    _, gids = AR.union(areas)
    hub = g["hub"]
    pairs = sorted((int(n), a) for a in (1, 2) for n in gids[a] if int(n) != hub)
    assert len(pairs) == 310

    def attrs(ents):
        return [(n, a, 1 if (n + a) % 9 == 4 else 0, n % 4) for n, a in ents]

    return [[(g["s000"], 1, 0, 0)],
            attrs(pairs[::35][:9]),
            attrs(pairs[::4][:65]),
            attrs(pairs[1::2][:130]),
            [(n, a, 0, 0) for n, a in pairs],
            [(g["s001"], 1, 1, 0), (g["s004"], 1, 1, 3)] + [(g[f"s{i}"], 2, 0, 1) for i in (200, 204, 205)],
            [(g["s135"], 1, 0, 0), (g["s135"], 2, 0, 0)],
            []]


def area_links_of(c, a, root, p):
    """the links of global root `root`'s next hops of prefix p in area a, from
    the expectation's words and the CSR's link counts"""
    ar = c.areas[a]
    r = ar["names"].index(root)
    nb = root_neighbor_ids(ar["csr"], r)
    cnt = link_counts(ar["csr"], r, False)
    w = c.exp["nh"][a][r, p]
    return sum(cnt[int(nb[k])] for k in range(nb.size) if int(w[k // 32]) >> (k % 32) & 1)


def fwide_preconditions(c):
    """the hub is wide in two areas that are not the first, and a cell of it has
    links from both packed ranges"""
    e, g = c.exp, gid_of(c.areas)
    hub = g["hub"]
    ns = [root_neighbor_ids(a["csr"], a["names"].index("hub")).size for a in c.areas]
    assert ns == [1, 140, 170]  # so the counts of areas 1 and 2 start at 1 and 141
    assert c.W == (1, 5, 6)
    assert [len(t) for t in c.table[:5]] == [1, 9, 65, 130, 310]
    both = [p for p in range(len(c.table))
            if area_links_of(c, 1, "hub", p) > 0 and area_links_of(c, 2, "hub", p) > 0]
    assert FWIDE_ALL in both and len(both) >= 2, both
    for p in both:
        assert e["areas"][hub, p] == 0b110
        assert e["links"][hub, p] == area_links_of(c, 1, "hub", p) + area_links_of(c, 2, "hub", p)
    assert e["areas"][hub, FWIDE_ONLY2] == 0b100 and e["links"][hub, FWIDE_ONLY2] > 0
    # slot 0 of area 1 (s000, two links) is not slot 0 of the packed counts (n0, one link)
    assert e["links"][hub, 0] == 2 and link_counts(c.areas[0]["csr"], 0, False) == {1: 1}
    assert c.facts["filtered"] > 0 and c.facts["drained_in_one_area"] > 0


# ---------------------------------------------------------------- F4w
def f4w_links(down=False):
    """area 0: the hub behind m0 (a 1-word root), m0 before two of the spokes;
    area 1: the hub with 100 spokes t000 .. t099 (4 words), some linked in
    pairs. down: the hub's link to t007 reported down"""
    sp = [f"t{i:03d}" for i in range(100)]
    l0 = [("hub", "m0", 1, 1), ("m0", "m1", 2, 2), ("m0", "t003", 1, 1), ("m0", "t010", 2, 2)]
    l1 = [("hub", s, 1 + i % 3, 1 + i % 2) + (("down",) if down and s == "t007" else ())
          for i, s in enumerate(sp)]
    l1 += [(sp[i], sp[i + 1], 1, 1) for i in range(0, 40, 2)]
    return [(l0, ()), (l1, ("t012",))]


def f4w(down=False):
    return [area(f"a{i}", *x) for i, x in enumerate(f4w_links(down))]


def f4w_table(areas, P):
    """P prefixes: a 9-entry one, a 65-entry one, two over both areas, then the
    spokes one by one"""
    g = gid_of(areas)
    t = [g[f"t{i:03d}"] for i in range(100)]
    table = [[(t[i], 1, i % 2, i % 3) for i in range(0, 90, 10)],
             [(t[i], 1, 0, i % 4) for i in range(34, 99)],  # t096: a bit of the hub's 4th word
             [(t[3], 0, 0, 0), (t[3], 1, 0, 1), (t[10], 0, 0, 0)],
             [(g["m1"], 0, 0, 0), (t[7], 1, 0, 0), (t[8], 1, 0, 0)]]
    table += [[(t[i], 1, 0, i % 3)] for i in range(P - len(table))]
    assert len(table) == P
    return table


def f4w_preconditions(c):
    hub = [a["names"].index("hub") for a in c.areas]
    W = [(root_neighbor_ids(a["csr"], r).size + 31) // 32 for a, r in zip(c.areas, hub)]
    assert W == [1, 4] and c.W == (1, 4), "the hub is no 4-word root"
    h = gid_of(c.areas)["hub"]
    assert (c.exp["areas"][h] == 2).any() and c.exp["nh"][1][hub[1]][:, 3].any()


# ---------------------------------------------------------------- the class word
def classtop_areas():
    """area 0: r - m at 3 with m drained, and an island i00 - ... - i39; area 1:
    r - e - m (m not drained there), the same island and a second one w0 - w1"""
    isl = [(f"i{k:02d}", f"i{k + 1:02d}", 1, 1) for k in range(39)]
    l0 = [("r", "m", 3, 3), ("r", "b", 1, 1)] + isl
    l1 = [("r", "e", 2, 2), ("e", "m", 1, 1), ("w0", "w1", 1, 1)] + isl
    return [area("a0", l0, ("m",)), area("a1", l1)]


def classtop_table(areas):
    """the only entry r reaches is m's in area 0, of class rank 2^31 - 1 on a
    node drained there; beside it island entries of rank 0 and 2^31 - 1 with
    larger thresholds. 3 entries (by the lane) and 70 (by the wave, m in the
    second 64-entry step)"""
    g = gid_of(areas)
    m = (g["m"], 0, TOP, 1)
    short = [(g["i00"], 0, 0, 9), m, (g["w0"], 1, TOP, 7)]
    isl = [(g[f"i{k:02d}"], a, TOP if (k + a) % 2 else 0, 9) for k in range(33) for a in (0, 1)]
    isl.append((g["i33"], 0, 0, 9))
    long = isl + [m, (g["w0"], 1, TOP, 7), (g["w1"], 1, 0, 8)]
    return [short, long, [(g["i00"], 1, 0, 0)]]


def classtop_preconditions(c):
    e, g = c.exp, gid_of(c.areas)
    r = g["r"]
    a0 = c.areas[0]
    assert np.asarray(a0["csr"]["no_transit"])[a0["names"].index("m")]
    assert (TOP << 1 | 1) == FF  # the class word: rank << 1 | drained
    assert [len(t) for t in c.table[:2]] == [3, 70]
    for p, at in ((0, 1), (1, 67)):
        assert c.table[p][at] == (g["m"], 0, TOP, 1)
        assert e["selected"][r, p] == (at,), "m's entry is not the only reached one"
        assert (e["metric"][r, p], e["best"][r, p], e["need"][r, p], e["count"][r, p]) == (3, at, 1, 1)
        assert e["areas"][r, p] == 1
    assert c.facts["all_drained"] > 0 and c.facts["unreached_best"] > 0


# ---------------------------------------------------------------- the cases
CASES = {
    "f32": (lambda: f32("plain"), f32_table, "x"),
    "f32-uniform": (lambda: f32("uniform"), f32_table, "x"),
    "f32-solo": (lambda: f32("solo"), f32_table, "x"),
    "f32-heavy": (lambda: f32("heavy"), heavy_table, "x"),
    "straddle": (lambda: f32("fill"), straddle_table, "x"),
    "straddle-wide": (lambda: f32("fillwide"), straddle_table, "x"),
    "fwide": (fwide, fwide_table, "hub"),
    "f4w-63": (f4w, lambda a: f4w_table(a, 63), "hub"),
    "f4w-64": (f4w, lambda a: f4w_table(a, 64), "hub"),
    "f4w-65": (f4w, lambda a: f4w_table(a, 65), "hub"),
    "classtop": (classtop_areas, classtop_table, "r"),
}


def preconditions(c):
    if c.name.startswith("f32"):
        f32_preconditions(c, c.name[4:] or "plain")
    if c.name == "f32-heavy":
        heavy_preconditions(c)
    if c.name.startswith("straddle"):
        straddle_preconditions(c)
    if c.name == "fwide":
        fwide_preconditions(c)
    if c.name.startswith("f4w"):
        f4w_preconditions(c)
    if c.name == "classtop":
        classtop_preconditions(c)


@functools.lru_cache(maxsize=None)
def case(name):
    """a fixture with its table and expectation (built once, never changed):
    areas, table, W (the areas' widths), exp, facts and root, the name of the
    node the case is about (it announces none of the prefixes)"""
    make, table_of, root = CASES[name]
    areas = make()
    table = table_of(areas)
    W = words(areas)
    exp, facts = AR.expect(areas, table, W)
    c = SimpleNamespace(name=name, areas=areas, table=table, W=W, exp=exp, facts=facts, root=root)
    preconditions(c)
    return c


def checked_cells(c):
    """the prefixes whose route the case's root installs without announcing
    them: what a comparison with the product's route build checks of that root"""
    r = gid_of(c.areas)[c.root]
    return [p for p, ents in enumerate(c.table)
            if not any(n == r for n, _, _, _ in ents) and c.exp["installed"][r, p]]


# ---------------------------------------------------------------- versions for the resident state
def f32_versions():
    """plain F32; area 31's first link at 1 (area 31 joins the winners: bit 31
    appears in the masks); then area 0's first link down as well. Each event
    touches one area: the others are the same dict objects."""
    v0 = f32("plain")
    v1 = v0[:31] + [f32_area(31, first=1)]
    v2 = [f32_area(0, down=True)] + v1[1:]
    return v0, v1, v2


def best_in_31(table):
    """f32_table's attributes with area 31's entry of every prefix alone in the
    best class"""
    return [[(n, a, 0 if a == 31 else 1, m) for n, a, _, m in ents] for ents in table]
