"""The in-place repair and the affected-roots kernel at their budgets,
against the CPU oracle.

  R1  1,024 queued nodes (kHeapCap): H1024 is repaired, H1025 flagged;
  R2  8,192 re-derivations (kPops): P8192 is repaired, P8193 flagged;
  R3  next-hop words in groups of 8: W8 / W9 / W16 / W17, bits 0, 255, 256,
      511, 512 and the last, and the root's own bit found by binary search;
  R4  LINK and NODE changes in one batch: MIX (M1 - M6, either order, both
      metric modes, every root) and RND (random graphs and batches);
  R5  distances under the u32 distance bound: L7R.

Every case uploads the oracle's rows of the state before the batch as the
finished runs (rows the kernel did not write), patches the resident graph and
calls ospf_repair_runs and ospf_affected_roots. The status array is asserted
exactly: 1 iff the oracle's dist row moves or repair_ref.py's counter passes a
budget; repaired rows are the oracle's rows after the batch; flagged rows keep
their distances; the affected flags equal the header's predicate.
test_host_repair_limits.py proves the cases sit where this file says."""
import numpy as np
import pytest

import repair_ref as R
from openr_amd.engine import Engine

pytestmark = pytest.mark.gpu

HOP = 0x1  # OSPF_HOP_COUNT


def run_case(name, use_link_metric=True, node_first=False, pick=None, empty=False):
    """One launch of the case's roots (or of positions `pick` of them).
    -> (status [n], dist [n, V], nh [n, V, W], affected [n]) and what was
    uploaded / is expected, as a dict. empty: no patch and n_changes = 0."""
    import torch
    c = R.case(name)
    d0, n0, d1, n1 = R.rows(name, use_link_metric)
    want = R.expected_status(name, use_link_metric, node_first)
    ch, ups, (nodes, bits) = R.csr_delta(c.g0.csr, c.g1.csr, node_first)
    pick = list(range(len(c.roots))) if pick is None else list(pick)
    roots = np.array(c.roots, np.uint32)[pick]
    if empty:
        ch, ups, nodes, d1, n1, want = [], [], [], d0, n0, np.zeros_like(want)
    flags = 0 if use_link_metric else HOP
    eng = Engine(0)
    try:
        eng.load({k: v.copy() for k, v in c.g0.csr.items()})
        d_roots = torch.from_numpy(roots.view(np.int32).copy()).cuda()
        d_dist = torch.from_numpy(d0[pick].view(np.int32).copy()).cuda()
        d_nh = torch.from_numpy(n0[pick].view(np.int32).copy()).cuda()
        d_st = torch.full((len(pick),), -1, dtype=torch.int32, device="cuda")
        d_aff = torch.full((len(pick),), 255, dtype=torch.uint8, device="cuda")
        if ups:
            eng.update_links(ups, version=2)
        if nodes:
            eng.update_nodes(nodes, bits, version=3)
        # (the affected test reads the rows of before the batch: it goes first)
        eng.affected(d_dist.data_ptr(), len(pick), ch, d_aff.data_ptr(), flags)
        eng.repair(d_roots.data_ptr(), len(pick), c.W, d_dist.data_ptr(), d_nh.data_ptr(), ch,
                   d_st.data_ptr(), flags)
        eng.sync()
        got = dict(status=d_st.cpu().numpy().view(np.uint32),
                   dist=d_dist.cpu().numpy().view(np.uint32),
                   nh=d_nh.cpu().numpy().view(np.uint32), affected=d_aff.cpu().numpy())
        fresh = eng.run(roots, c.W, hop_count=not use_link_metric) if not empty else None
    finally:
        eng.close()
    exp = dict(status=want[pick], d0=d0[pick], d1=d1[pick], n1=n1[pick], fresh=fresh,
               affected=R.affected(c.g0.csr if empty else c.g1.csr, d0[pick], ch, not use_link_metric))
    return got, exp


def check_case(name, use_link_metric=True, node_first=False, pick=None, empty=False):
    got, exp = run_case(name, use_link_metric, node_first, pick, empty)
    tag = (name, use_link_metric, node_first)
    assert np.array_equal(got["status"], exp["status"]), (tag, got["status"], exp["status"])
    ok = exp["status"] == 0
    assert np.array_equal(got["dist"][ok], exp["d1"][ok]), tag
    bad = np.nonzero(ok)[0][(got["nh"][ok] != exp["n1"][ok]).any(axis=(1, 2))]
    assert bad.size == 0, (tag, "repaired next hops differ from the oracle's, root positions", bad)
    # the repair never writes a distance
    assert got["dist"].tobytes() == exp["d0"].tobytes(), tag
    assert np.array_equal(got["affected"], exp["affected"]), (tag, got["affected"], exp["affected"])
    return got, exp


# ------------------------------------------------------ R4. mixed batches
@pytest.mark.parametrize("node_first", [False, True], ids=["links_first", "nodes_first"])
@pytest.mark.parametrize("use_link_metric", [True, False], ids=["metric", "hops"])
@pytest.mark.parametrize("name", R.MIX_CASES)
def test_r4_mixed_batches_on_the_diamond(name, use_link_metric, node_first):
    """M1 / M2: a node that sets overload and loses (or re-metrics) a link in
    one batch: the link's old tightness must not be judged by the tail's new
    transit bit. M3 the way back, M4 with distances moving, M5 tightness
    moving inside a parallel pair, M6 overload bits of the root itself, an
    island node and the root's neighbour."""
    check_case(name, use_link_metric, node_first)


@pytest.mark.parametrize("use_link_metric", [True, False], ids=["metric", "hops"])
@pytest.mark.parametrize("name", R.RND_CASES)
def test_r4_random_graphs_and_batches(name, use_link_metric):
    check_case(name, use_link_metric, node_first=name.endswith(("1", "3")))


@pytest.mark.parametrize("n", [1, 4, 5])
def test_r4_runs_per_block(n):
    """1, 4 and 5 runs (kRWaves = 4 per block) of M1's roots, r among them"""
    c = R.case("MIX-M1")
    i = c.roots.index(c.g0.ids["r"])
    got, _ = check_case("MIX-M1", pick=[i, 0, 1, 2, len(c.roots) - 1][:n])
    assert got["status"][0] == 0


def test_no_changes_leave_rows_and_status_alone():
    got, exp = check_case("MIX-M1", empty=True)
    assert not got["status"].any() and not got["affected"].any()
    assert got["nh"].tobytes() == exp["n1"].tobytes()


# ------------------------------------------------- R1 / R2. the budgets
@pytest.mark.parametrize("name", list(R.STATED))
def test_r1_r2_on_and_past_the_budgets(name):
    """The stated root queues 1,024 / 1,025 nodes at once (H) or pops 8,192 /
    8,193 (P): repaired on the budget, flagged one past it; the other roots
    of the launch (a leaf whose distances move, b's small repair) are
    answered as if alone."""
    c = R.case(name)
    got, exp = check_case(name)
    i = c.roots.index(c.g0.ids[R.STATED[name][0]])
    assert got["status"][i] == (1 if name.endswith(("1025", "8193")) else 0)
    check_case(name, use_link_metric=False)


# ---------------------------------------------------- R3. word groups of 8
@pytest.mark.parametrize("name", R.WIDE_CASES)
def test_r3_word_groups(name):
    """h has 256 / 257 / 512 / 513 neighbours (8, 9, 16, 17 words): t loses
    the next hop at one bit, and the neighbour that loses one of its two links
    to h keeps its bit, found by the root's binary search, with status 0."""
    c = R.case(name)
    got, exp = check_case(name)
    assert got["status"][c.roots.index(c.g0.ids["h"])] == 0


# ---------------------------------------------------- R5. distance bound
@pytest.mark.parametrize("use_link_metric", [True, False], ids=["metric", "hops"])
def test_r5_under_the_distance_bound(use_link_metric):
    c = R.case("L7R")
    got, _ = check_case("L7R", use_link_metric)
    i = c.roots.index(c.g0.ids[R.L7R_FAR[0]])
    assert got["status"][i] == 0
    if use_link_metric:
        assert got["dist"][i, c.g0.ids["fc"]] == R.L7R_FAR[1]


# ------------------------------------------------- the two references tied
@pytest.mark.parametrize("name", ["MIX-M1", "MIX-M4", "RND1-2", "H1024", "W17-512", "L7R"])
def test_oracle_rows_are_what_a_fresh_run_computes(name):
    for mode in (True, False):
        _, exp = run_case(name, mode)
        assert np.array_equal(exp["fresh"]["dist"], exp["d1"]), (name, mode)
        assert np.array_equal(exp["fresh"]["nh"], exp["n1"]), (name, mode)


def test_linkstate_device_path_drain_in_one_publication():
    R.check_linkstate_drain(host=False)
