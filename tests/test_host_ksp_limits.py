"""The shapes of ksp_ref.py are what test_gpu_ksp_limits.py says they are
(checked on the host against the oracle and the CSR restatement, never the
engine, so the GPU tests cannot be vacuous): path counts and lengths for
k = 1 and k = 2, claimed links, record words, the ignore set and how many of
its links touch the source, the affected set of the masked rerun, the row
entries it owns, the hints it takes, the candidate order at the H
destinations, the depth bound, and that odl::LinkState's host path gives the
oracle's KSP2 text."""
import pytest

import ksp_ref as K
from graphs import depth_bound
from openr_amd.linkstate import LinkState

NAMES = list(K.BUILD)


@pytest.fixture(scope="module")
def link_ids():
    cache = {}

    def of(name):
        if name not in cache:
            keys = LinkState(stream=K.shape(name).stream).link_keys()
            cache[name] = {k: i for i, k in enumerate(keys)}
        return cache[name]
    return of


@pytest.mark.parametrize("name", NAMES)
def test_shape_is_what_it_claims(name, link_ids):
    st, g = K.STATED[name], K.shape(name)
    src = g.ids[st["src"]]
    k1, k2 = K.paths(name)
    for ps, (n, ln) in ((k1, st["k1"]), (k2, st["k2"])):
        assert len(ps) == n
        assert ln is None or all(len(p) == ln for p in ps)
        flat = [l for p in ps for l in p]
        assert len(flat) == len(set(flat))  # edge-disjoint: claims == links
        for p in ps:  # a path from src to dst
            assert st["src"] in K.key_ends(p[0]) and st["dst"] in K.key_ends(p[-1])
    assert not ({l for p in k1 for l in p} & {l for p in k2 for l in p})
    unit = all(int(m) == 1 for m, up in zip(g.csr["metric"], g.csr["edge_up"]) if up)
    assert unit == st["unit"]
    assert (depth_bound(g.csr) > 253) == bool(st.get("deep"))
    # the record fits its cap unless the status says otherwise, and a status
    # bit has its reason: a path past 256 links, claims past 1,536, or (k = 2)
    # a masked distance past the level bytes
    over = [max(map(len, ps), default=0) > 256 or K.claims(ps) > 1536 for ps in (k1, k2)]
    over[1] = over[1] or K.past_levels(name)
    fits = [K.record_words(ps) <= st["cap"] for ps in (k1, k2)]
    want = (K.OVF1 | K.OVF2) if over[0] or not fits[0] else \
        (K.RERUN if k1 else 0) | (K.OVF2 if over[1] or not fits[1] else 0)
    assert st["status"] == want
    if st["status"] & K.OVF1:
        return
    ign = [link_ids(name)[l] for p in k1 for l in p]
    assert len(ign) == st["nign"] == K.claims(k1)
    if "at_src" in st:
        assert sum(st["src"] in K.key_ends(l) for p in k1 for l in p) == st["at_src"]
    A = K.affected(g.csr, src, ign)
    if "A" in st:
        assert len(A) == st["A"]
    if "edges" in st:
        assert K.owned_entries(g.csr, A, src) == st["edges"]
    if "keys" in st:
        assert K.lost_hints(g.csr, src, ign) == st["keys"]
    # who answers the rerun follows from the budgets: 256 ignored links and
    # 16 of the source's (presplit); 192 affected nodes, 384 keys, 4,096 row
    # entries, 384 claimed links (the decremental kernel gives the run up)
    cut = K.source_cut(g.csr, src, ign)  # answered before the affected set is built
    assert cut == bool(st.get("cut"))
    assert st["route"] == K.route(g.csr, src, ign, k2)
    if "bound" in st:
        assert depth_bound(g.csr) == st["bound"]
    # the furniture: an ECMP diamond, a no-transit destination, a down link, an island
    if "fa" in g.ids:
        at = st.get("at", st["src"])
        assert len(g.oracle.kth_paths(at, "fc", 1)) == 2
        assert g.csr["no_transit"][g.ids["fo"]] == 1 and g.oracle.kth_paths(at, "fo", 1)
        assert g.oracle.kth_paths(at, "za", 1) == [] and g.oracle.kth_paths("za", "zb", 1) != []
        assert (g.csr["edge_up"] == 0).sum() == 2


@pytest.mark.parametrize("name", NAMES)
def test_host_path_gives_the_oracles_text(name):
    g, st = K.shape(name), K.STATED[name]
    p = LinkState(stream=g.stream)
    p.set_host_spf(True)
    dsts = [st["dst"], st["src"], g.names[-1]]
    assert p.ksp2_text(st["src"], dsts) == g.oracle.ksp2_text(st["src"], dsts)
    assert p.kth_paths(st["src"], st["dst"], 1) == [list(x) for x in K.paths(name)[0]]


def test_limits_sit_on_their_edges():
    """each pair differs by one unit of its budget, on and just past it"""
    c = {n: K.claims(K.paths(n)[0]) for n in ("C768", "C800", "C1536", "C1568")}
    assert c == {"C768": 768, "C800": 800, "C1536": 1536, "C1568": 1568}
    assert [K.claims(K.paths(n)[1]) for n in ("D384", "D392")] == [384, 392]
    assert [len(K.paths(n)[1][0]) for n in ("P256", "P257", "P256w", "P257w")] == [256, 257, 256, 257]
    assert [len(K.paths(n)[0][0]) for n in ("L256", "L257")] == [256, 257]
    assert (K.record_words(K.paths("R")[0]), K.record_words(K.paths("R")[1])) == K.R_WORDS
    # the 768 / 800 records fit the 1,024-word cap whose trace has the small hash
    assert K.record_words(K.paths("C800")[0]) <= 1024 < K.record_words(K.paths("C1536")[0]) <= 2048
    assert K.record_words(K.paths("C1568")[0]) <= 2048  # C1568 overflows on claims, not on words


def test_second_destination_half_way_round_the_even_ring():
    g = K.shape("P257")  # 258 nodes
    k1 = g.oracle.kth_paths("r0000", "r0129", 1)
    assert [len(p) for p in k1] == [129, 129] and g.oracle.kth_paths("r0000", "r0129", 2) == []


@pytest.mark.parametrize("fail", [15, 16, 17, 31, 32, 33, 64, 65])
def test_heavy_shapes_candidate_order(fail):
    """d's tight predecessors in row order are p001 .. p(c); path 1 takes the
    first through b0, path 2 the last through b1, so the fail = c - 2 between
    them fail in order; they start at row position H_PAD."""
    name = f"H{fail}"
    g = K.shape(name)
    s, d = g.ids["s"], g.ids["d"]
    base = K.masked_dist(g.csr, s)
    sup = K.supports(g.csr, s, base, d)
    assert [g.names[u] for u, _ in sup] == [f"p{j:03d}" for j in range(1, fail + 3)]
    rp, col = g.csr["row_ptr"], g.csr["col"]
    row = [g.names[int(col[e])] for e in range(int(rp[d]), int(rp[d + 1]))]
    assert row.index("p001") == K.H_PAD and (row.index(f"p{fail + 2:03d}") >= 64) == (fail >= 23)
    k1, k2 = K.paths(name)
    for path, cand, via in ((k1[0], "p001", "b0"), (k1[1], f"p{fail + 2:03d}", "b1")):
        assert cand in K.key_ends(path[-1]) and via in K.key_ends(path[0])
    # every chain is private and one level of lookahead sees nothing wrong with it
    assert all(int(rp[g.ids[f"p{j:03d}"] + 1]) - int(rp[g.ids[f"p{j:03d}"]]) == 2 for j in range(1, fail + 3))
    assert int(rp[g.ids["b0"] + 1]) - int(rp[g.ids["b0"]]) == fail + 2


@pytest.mark.parametrize("row", [16, 17])
def test_lookahead_shapes(row, link_ids):
    """every candidate of d has a row of exactly `row` entries and one tight
    predecessor; p001 .. p005 share b0, whose only way on path 1 claims"""
    name = f"K{row}"
    g = K.shape(name)
    s, d = g.ids["s"], g.ids["d"]
    base = K.masked_dist(g.csr, s)
    rp = g.csr["row_ptr"]
    cands = [f"p{j:03d}" for j in range(1, K.K_CAND + 1)]
    assert [g.names[u] for u, _ in K.supports(g.csr, s, base, d)] == cands
    for j, p in enumerate(cands):
        v = g.ids[p]
        assert int(rp[v + 1]) - int(rp[v]) == row
        assert [g.names[u] for u, _ in K.supports(g.csr, s, base, v)] == ["b1" if j == K.K_CAND - 1 else "b0"]
    assert len(K.supports(g.csr, s, base, g.ids["b0"])) == 1
    k1 = K.paths(name)[0]
    assert "p001" in K.key_ends(k1[0][-1]) and cands[-1] in K.key_ends(k1[1][-1])


def test_level_byte_shapes(link_ids):
    """All have depth bound 252, so the multi-source reruns serve them.
    V252's masked distance is 252 (level byte 253). V253 .. V255 settle the
    open question: graphs within the bound whose masked distance is 253, 254
    and 255 exist -- a shortcut that k = 1 takes keeps the bound low and is
    ignored by the rerun. Their k = 2 path still fits the 256 links of a path."""
    for name, far in (("V252", 252), ("V253", 253), ("V254", 254), ("V255", 255)):
        g = K.shape(name)
        assert depth_bound(g.csr) == 252
        assert g.csr["no_transit"][g.ids["s"]] == 1 and g.csr["no_transit"][g.ids["t"]] == 1
        ign = [link_ids(name)[l] for p in K.paths(name)[0] for l in p]
        masked = K.masked_dist(g.csr, g.ids["s"], ign)
        assert masked[g.ids["t"]] == far == max(x for x in masked if x != K.INF)
        assert [len(p) for p in K.paths(name)[1]] == [far] and far <= 256


def test_mixed_batch_shape(link_ids):
    """more than 256 runs the decremental kernel gives up and two presplit ones"""
    g = K.shape("X")
    s = g.ids["s"]
    routes = {}
    for d in set(K.mixed_dsts()):
        k1, k2 = K.paths("X", d)
        if k1:
            routes[d] = K.route(g.csr, s, [link_ids("X")[l] for p in k1 for l in p], k2)
    assert routes["dp"] == routes["dq"] == "presplit"
    assert sum(r == "full" for r in routes.values()) == 2 * (K.X_FAN + K.X_FAN ** 2) + 1 > 256  # (+ ma)
    assert routes["ma"] == "full" and all(K.paths("X", d)[1] for d in routes)  # every run has a k = 2 path
