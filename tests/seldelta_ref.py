"""Oracle-derived expectation for the selection delta (shared by
test_gpu_select_delta.py and test_host_select_delta.py).

A graph version is an AdjDb list; its expectation is select_ref.expect over a
fresh CPU oracle's SPF results. The expected delta between two versions is the
numpy diff of their expectations; the rebased roots are those whose
select_ref.root_neighbor_ids differ. Nothing here reads the code under test
beyond LinkState's ingest (node ids and the CSR snapshot, as select_ref does).

Events are edits of the AdjDb list, picked by position so that a seed stays a
seed; each test asserts that its expectation is not vacuous."""
import copy

import numpy as np

import select_ref as R
from openr_amd.adjdb import AdjDb, AdjDbStream, create_adjacency
from openr_amd.linkstate import LinkState
from oracle import Oracle, parse_spf_text


class Version:
    """One graph version: stream, node names (id order), CSR, lazily the
    oracle's SPF of chosen roots."""

    def __init__(self, dbs):
        self.dbs = dbs
        self.stream = AdjDbStream.from_dbs(dbs)
        ls = LinkState()
        ls.set_host_spf(True)
        ls.apply(self.stream)
        self.names, self.csr = ls.node_names(), ls.csr()
        self.V = len(self.names)
        self._orc = None
        self._spf = {}

    def nbrs(self, r):
        return R.root_neighbor_ids(self.csr, r).tolist()

    @property
    def words(self):
        return max(1, max((len(self.nbrs(r)) + 31) // 32 for r in range(self.V)))

    def spf(self, use_link_metric=True, roots=None):
        """{root name: parsed oracle SPF} for `roots` (ids; None = all)."""
        if self._orc is None:
            self._orc = Oracle(self.stream)
        out = {}
        for r in (range(self.V) if roots is None else roots):
            key = (r, use_link_metric)
            if key not in self._spf:
                self._spf[key] = parse_spf_text(self._orc.spf_text(self.names[r], use_link_metric))
            out[self.names[r]] = self._spf[key]
        return out

    def expect(self, table, W, use_link_metric=True, roots=None):
        """select_ref.expect by node id; with `roots` only those rows are
        computed (the others stay INF / 0)."""
        if roots is None:
            return R.expect(self.spf(use_link_metric), self.names, self.csr, table, W)
        # select_ref.expect walks every name as a root: the roots not asked
        # for get an empty SPF result (nothing reached)
        spf = self.spf(use_link_metric, roots)
        return R.expect({nm: spf.get(nm, {}) for nm in self.names}, self.names, self.csr, table, W)


def delta(before, after, table, W, use_link_metric=True, roots=None):
    """-> (changed {(root, prefix)}, rebased [roots], expectation after,
    expectation before). Rebased roots' entries are not in `changed`. With
    `roots` only those roots are looked at."""
    assert before.names == after.names
    eb = before.expect(table, W, use_link_metric, roots)
    ea = after.expect(table, W, use_link_metric, roots)
    look = range(before.V) if roots is None else roots
    rebased = [r for r in look if before.nbrs(r) != after.nbrs(r)]
    mask = (eb[0] != ea[0]) | (eb[1] != ea[1]) | (eb[2] != ea[2]).any(axis=2)
    mask[rebased] = False
    if roots is not None:
        keep = np.zeros(before.V, bool)
        keep[list(roots)] = True
        mask[~keep] = False
    changed = {(int(r), int(p)) for r, p in np.argwhere(mask)}
    return changed, rebased, ea, eb


def records(rec, nh):
    """update()'s arrays -> {(root, prefix): (metric, count, words tuple)};
    asserts that no entry is listed twice."""
    out = {}
    for i in range(len(rec)):
        key = (int(rec["root"][i]), int(rec["prefix"][i]))
        assert key not in out, ("listed twice", key)
        out[key] = (int(rec["metric"][i]), int(rec["count"][i]), tuple(int(x) for x in nh[i]))
    return out


def wanted(changed, ea):
    return {(r, p): (int(ea[0][r, p]), int(ea[1][r, p]), tuple(int(x) for x in ea[2][r, p]))
            for r, p in changed}


# ---------------------------------------------------------------- events
def base_dbs(kind, seed, n=70):
    st, _ = R.graph(kind, seed, n)
    return st.to_dbs()


def up_adjs(dbs):
    """(db index, adjacency index) of every adjacency not reported down, in
    stream order."""
    return [(i, j) for i, d in enumerate(dbs) for j, a in enumerate(d.adjs) if not a.overloaded]


def link_down(dbs, k):
    """the k-th up adjacency reported overloaded (the link goes down; the
    neighbour lists stay)"""
    out = copy.deepcopy(dbs)
    i, j = up_adjs(out)[k]
    out[i].adjs[j].overloaded = True
    return out


def metric_bump(dbs, k, by=1):
    out = copy.deepcopy(dbs)
    i, j = up_adjs(out)[k]
    out[i].adjs[j].metric += by
    return out


def node_overload(dbs, k):
    out = copy.deepcopy(dbs)
    free = [i for i, d in enumerate(out) if not d.overloaded]
    out[free[k]].overloaded = True
    return out


def link_up(dbs, a, b, metric=1):
    """a new link between nodes a and b (names)"""
    out = copy.deepcopy(dbs)
    by = {d.name: d for d in out}
    by[a].adjs.append(create_adjacency(b, f"{a}-{b}-new", f"{b}-{a}-new", metric))
    by[b].adjs.append(create_adjacency(a, f"{b}-{a}-new", f"{a}-{b}-new", metric))
    return out


def non_neighbours(v, k=0):
    """the k-th pair of node names (id order) without a link between them"""
    seen = 0
    for a in range(v.V):
        na = set(v.nbrs(a))
        for b in range(a + 1, v.V):
            if b not in na:
                if seen == k:
                    return v.names[a], v.names[b]
                seen += 1
    raise AssertionError("complete graph")


def star_dbs(spokes, ring=True, extra=0, seed=5):
    """A hub with `spokes` spokes (metrics 1-3); with `ring` the spokes in a
    ring; `extra` more nodes hung off the first spokes (not linked to the hub)."""
    rng = np.random.default_rng(seed)
    names = ["hub"] + [f"s{i:04d}" for i in range(spokes)] + [f"x{i}" for i in range(extra)]
    adjs = {nm: [] for nm in names}

    def link(a, b, m):
        adjs[a].append(create_adjacency(b, f"{a}-{b}", f"{b}-{a}", m))
        adjs[b].append(create_adjacency(a, f"{b}-{a}", f"{a}-{b}", m))

    for i in range(spokes):
        link("hub", names[1 + i], int(rng.integers(1, 4)))
        if ring and spokes > 2:
            link(names[1 + i], names[1 + (i + 1) % spokes], int(rng.integers(1, 4)))
    for i in range(extra):
        link(f"x{i}", names[1 + i], 1)
    return [AdjDb(nm, adjs[nm], i + 1) for i, nm in enumerate(names)]


def prefixes_by_name(names, table):
    return {f"p{i}": [names[a] for a in ann] for i, ann in enumerate(table)}
