"""The cases of repair_ref.py are what test_gpu_repair_limits.py says they
are (checked on the host against the oracle alone, never the engine, so the
GPU tests cannot be vacuous): a batch leaves the CSR's structure alone; the
propagation counter gives exactly the stated pushes, pops and queue length on
the budget shapes and stays below half of each budget everywhere else, which
makes "status 1 iff a distance moved" exact there; every case has roots of
both statuses and repaired roots whose next hops really change; the numpy
affected predicate is sound against the oracle; and odl::LinkState's host
path answers a drain published in one AdjDb like the oracle."""
import numpy as np
import pytest

import repair_ref as R
from graphs import dist_bound

MODES = (True, False)  # use_link_metric
SMALL = R.MIX_CASES + R.RND_CASES + ["L7R"]  # every node is a root


@pytest.mark.parametrize("name", list(R.CASES))
def test_batch_keeps_the_structure(name):
    c = R.case(name)
    a, b = c.g0.csr, c.g1.csr
    for k in ("row_ptr", "col", "link_id", "twin", "link_rank"):
        assert np.array_equal(a[k], b[k]), (name, k)
    ch, ups, (nodes, bits) = R.csr_delta(a, b)
    assert len(ch) == len(ups) + len(nodes) == len(c.ops), (name, ch, c.ops)
    assert [x[0] for x in R.csr_delta(a, b, node_first=True)[0]] == \
        [R.NODE] * len(nodes) + [R.LINK] * len(ups)


@pytest.mark.parametrize("name", list(R.STATED))
def test_budget_shapes_sit_on_their_numbers(name):
    """pushes, pops and the largest queue of the stated root, exactly: one
    more queued node than H1024 or one more pop than P8192 passes a budget"""
    c = R.case(name)
    root, pushes, pops, qmax = R.STATED[name]
    i = c.roots.index(c.g0.ids[root])
    for mode in MODES:
        d0, _, d1, _ = R.rows(name, mode)
        assert np.array_equal(d0[i], d1[i])
        k = R.counts(name, mode)[i]
        assert (k["pushes"], k["pops"], k["qmax"], k["moved"]) == (pushes, pops, qmax, False), (name, k)
        over = qmax > R.HEAP_CAP or pops > R.POPS
        assert over == name.endswith(("1025", "8193"))
        st = R.expected_status(name, mode)
        assert st[i] == int(over)
        # the same launch holds roots whose distances move and a small repair
        others = [j for j in range(len(c.roots)) if j != i]
        assert any(st[j] == 1 for j in others) and any(st[j] == 0 for j in others), (name, st)
    assert c.g0.V <= 8300 and len(c.roots) == 5


def test_budget_pairs_differ_by_one_node():
    assert R.case("H1025").g0.V == R.case("H1024").g0.V + 1
    assert R.case("P8193").g0.V == R.case("P8192").g0.V + 1
    assert R.HEAP_CAP == 1024 and R.POPS == 8192


@pytest.mark.parametrize("name", [c for c in R.CASES if c not in R.STATED])
def test_counter_stays_below_half_of_each_budget(name):
    """A condition on the inputs: with at most 512 queued nodes and 4,096
    pops no budget is near, so a root's status is 1 iff a distance moves. The
    counter never sees a moved distance on a root whose oracle rows keep
    theirs."""
    for mode in MODES:
        for node_first in (False, True):
            for k in R.counts(name, mode, node_first):
                if k is not None:
                    assert k["qmax"] <= R.HEAP_CAP // 2 and k["pops"] <= R.POPS // 2, (name, k)
                    assert not k["moved"], (name, mode, node_first, k)
            d0, _, d1, _ = R.rows(name, mode)
            assert np.array_equal(R.expected_status(name, mode, node_first),
                                  (d0 != d1).any(axis=1).astype(np.uint32))


def kept_and_changed(name, mode):
    """roots with expected status 0 whose next-hop rows differ before and after"""
    _, n0, _, n1 = R.rows(name, mode)
    return (R.expected_status(name, mode) == 0) & (n0 != n1).any(axis=(1, 2))


@pytest.mark.parametrize("name", [c for c in R.CASES if len(R.CASES[c][2] or "many") > 1])
def test_cases_are_not_vacuous(name):
    """over the two metric modes: a repaired root whose next hops change, and
    a root that must be flagged"""
    assert any(kept_and_changed(name, m).any() for m in MODES), name
    assert any((R.expected_status(name, m) == 1).any() for m in MODES), name


def test_single_root_cases_are_repairs():
    for name in R.WIDE_CASES:
        if len(R.case(name).roots) == 1:
            assert kept_and_changed(name, True).all() and kept_and_changed(name, False).all()


def test_random_cases_mostly_repair():
    """at least a quarter of the (case, mode, root) triples of RND are
    repaired roots whose next hops change; at least half the batches hold
    both kinds of change"""
    share = np.concatenate([kept_and_changed(n, m) for n in R.RND_CASES for m in MODES])
    assert share.mean() >= 0.25, share.mean()
    mixed = [len({op[0] == "over" for op in R.case(n).ops}) == 2 for n in R.RND_CASES]
    assert sum(mixed) * 2 >= len(mixed)
    sizes = [len(R.case(n).ops) for n in R.RND_CASES]
    assert min(sizes) >= 1 and max(sizes) <= 6 and len(set(sizes)) >= 4
    kinds = {op[0] + (str(op[2]) if op[0] == "over" else "") for n in R.RND_CASES for op in R.case(n).ops}
    assert kinds == {"down", "up", "metric", "overTrue", "overFalse"}
    assert all(40 <= R.case(n).g0.V <= 70 for n in R.RND_CASES)


def test_mix_drain_moves_next_hops_only():
    """M1 / M2 as the issue states them: root r keeps every distance and
    v's next hops go from {a, b} to {b}; M3 is the way back"""
    for b in ("M1", "M2", "M3"):
        c = R.case(f"MIX-{b}")
        i, v = c.roots.index(c.g0.ids["r"]), c.g0.ids["v"]
        d0, n0, d1, n1 = R.rows(c.name, True)
        assert np.array_equal(d0[i], d1[i]) and d0[i, v] == 2
        both, only_b = 0b11, 0b10  # r's neighbours in id order: a, b
        assert (int(n0[i, v, 0]), int(n1[i, v, 0])) == ((only_b, both) if b == "M3" else (both, only_b))


def test_wide_cases_sit_on_the_word_groups():
    for name, K in R.WIDE.items():
        c = R.case(f"{name}-{K - 1}")
        assert c.W == (K + 31) // 32 and c.W == int(name[1:])
        h, t = c.g0.ids["h"], c.g0.ids["t"]
        i = c.roots.index(h)
        _, n0, _, n1 = R.rows(c.name, True)
        gone = np.nonzero(np.unpackbits((n0[i, t] ^ n1[i, t]).view(np.uint8), bitorder="little"))[0]
        assert gone.tolist() == [K - 1]
        # the neighbour that lost one of its two links to h keeps its own bit
        last = c.g0.ids[f"n{K - 1:04d}"]
        assert np.array_equal(n0[i, last], n1[i, last]) and n1[i, last, (K - 1) // 32] == 1 << ((K - 1) % 32)


def test_l7r_sits_under_the_distance_bound():
    c = R.case("L7R")
    root, far = R.L7R_FAR
    i = c.roots.index(c.g0.ids[root])
    assert dist_bound(c.g0.csr) == 2 ** 32 - 2
    d0, _, d1, _ = R.rows("L7R", True)
    assert int(d0[i][d0[i] != R.INF].max()) == far == int(d1[i][d1[i] != R.INF].max())
    assert d0[i, c.g0.ids["fc"]] == far and R.expected_status("L7R", True)[i] == 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_affected_predicate_is_sound(name):
    """a root the predicate leaves unflagged has the same oracle rows and the
    same spf_text before and after"""
    c = R.case(name)
    ch = R.csr_delta(c.g0.csr, c.g1.csr)[0]
    for mode in MODES:
        d0, n0, d1, n1 = R.rows(name, mode)
        f = R.affected(c.g1.csr, d0, ch, not mode).astype(bool)
        for i in np.nonzero(~f)[0]:
            nm = c.g0.names[c.roots[i]]
            assert np.array_equal(d0[i], d1[i]) and np.array_equal(n0[i], n1[i]), (name, nm)
            assert c.g0.oracle.spf_text(nm, mode) == c.g1.oracle.spf_text(nm, mode), (name, nm)
        if name in SMALL:
            assert f.any() and not f.all(), (name, mode)


def test_linkstate_host_path_drain_in_one_publication():
    R.check_linkstate_drain(host=True)
