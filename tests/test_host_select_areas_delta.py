"""The expectation the GPU tests of ospf_areastate_* use (areas_delta_ref), on
a machine without a GPU: every step of every fixture is checked for being
non-vacuous, so that an input which changes nothing (or everything) is caught
before a GPU is used."""
import numpy as np
import pytest

import areas_delta_ref as DR
import areas_ref as AR
import seldelta_ref as SR

FF = 0xFFFFFFFF


def facts_of(before, after, tb, ta, hop=False):
    W = tuple(max(x, y) for x, y in zip(DR.words(before), DR.words(after)))
    changed, rebased, ea, eb = DR.delta(before, after, tb, ta, W, hop)
    G, P = ea["metric"].shape
    return dict(changed=len(changed), cells=G * P, rebased=len(rebased),
                mask=int(sum(eb["areas"][c] != ea["areas"][c] for c in changed)),
                one_area=int(sum(DR.only_one_areas_words(before, eb, ea)[c] for c in changed)),
                lost=int(sum(eb["metric"][c] != FF and ea["metric"][c] == FF for c in changed)))


@pytest.mark.parametrize("unit,hop,sizes,nb", DR.RANDOM_CASES)
def test_random_versions_are_not_vacuous(unit, hop, sizes, nb):
    vs = DR.random_versions(11 + len(sizes), sizes, nb, unit, hop)
    table = DR.random_table(vs[0])
    assert len(table) > 64 and {0, 1, 8, 9, 64, 65, 130} <= {len(e) for e in table}
    tot = dict(mask=0, lost=0)
    for step, (b, a) in enumerate(zip(vs, vs[1:])):
        f = facts_of(b, a, table, table, hop)
        assert 0 < f["changed"] < f["cells"], (step, f)
        for k in tot:
            tot[k] += f[k]
    assert all(tot.values()), tot
    # only area 0 moved in the first step, only the last area in the second
    assert [x is y for x, y in zip(vs[0], vs[1])] == [False] + [True] * (len(sizes) - 1)
    assert [x is y for x, y in zip(vs[1], vs[2])] == [True] * (len(sizes) - 1) + [False]


def test_four_node_steps_are_not_vacuous():
    t = [[(3, 0, 0, 0), (3, 1, 0, 0)], [(1, 1, 0, 0)], [(2, 0, 0, 0)]]
    steps = [DR.four_nodes(m) for m in (10, 5, 20)]
    for b, a in zip(steps, steps[1:]):
        f = facts_of(b, a, t, t)
        assert 0 < f["changed"] < f["cells"] and f["mask"] > 0 and f["rebased"] == 0, f


def test_swap_step_moves_one_areas_words_only():
    before, after, table = DR.swap_versions()
    f = facts_of(before, after, table, table)
    assert 0 < f["changed"] < f["cells"] and f["one_area"] > 0 and f["rebased"] == 0, f


def test_hub_step_is_not_vacuous():
    before = [DR.area_links(*x) for x in DR.hub_links()]
    after = [DR.area_links(*DR.hub_links(DR.DEAR)[0]), before[1]]
    table = DR.random_table_hub(before)
    assert len(table) > 64
    W = DR.words(before)
    assert W[0] == 5 and W[1] <= 2
    changed, rebased, ea, eb = DR.delta(before, after, table, table, W)
    g = AR.union(before)[0].index("hub")
    mine = {p for r, p in changed if r == g}
    assert not rebased and 0 < len(mine) < len(table)
    assert 0 < len(changed) < ea["metric"].size


def test_rebase_steps_are_not_vacuous():
    v0, v1 = DR.rebase_versions()
    table = DR.rebase_table(v0)
    gnames, _ = AR.union(v0)
    for b, a in ((v0, v1), (v1, v0)):
        W = tuple(max(x, y) for x, y in zip(DR.words(b), DR.words(a)))
        changed, rebased, ea, eb = DR.delta(b, a, table, table, W)
        assert rebased == sorted(gnames.index(n) for n in ("hub", "x0"))
        assert 0 < len(changed) < ea["metric"].size
    assert DR.words(v0)[0] == 1 and DR.words(v1)[0] == 2


def test_attribute_step_is_not_vacuous():
    vs = DR.random_versions(13, (60, 70), 5, False)
    table = DR.random_table(vs[0])
    f = facts_of(vs[0], vs[0], table, DR.other_attrs(table))
    assert 0 < f["changed"] < f["cells"] and f["rebased"] == 0, f


# ---------------------------------------------------------------- the tracker on the host path
from openr_amd.linkstate import AreasTracker  # noqa: E402


def test_tracker_on_the_host_random_versions():
    vs = DR.random_versions(13, (60, 70), 5, False)
    table = DR.random_table(vs[0])
    lss = DR.ls_areas(vs[0], host=True)
    tr = AreasTracker(lss, DR.ls_prefixes(vs[0], table))
    try:
        DR.assert_tracked(tr, vs[0], table)
        for b, a in zip(vs, vs[1:]):
            DR.ls_load(lss, b, a)
            DR.assert_tracker_delta(tr, b, a, table, table, on_device=False)
        d = tr.delta()  # nothing moved
        assert not d["full"] and len(d["changes"]) == 0 and d["rebased"].size == 0
    finally:
        tr.close()


def test_tracker_on_the_host_rebase_attributes_and_full():
    v0, v1 = DR.rebase_versions()
    table = DR.rebase_table(v0)
    lss = DR.ls_areas(v0, host=True)
    tr = AreasTracker(lss, DR.ls_prefixes(v0, table))
    try:
        for b, a in ((v0, v1), (v1, v0)):
            DR.ls_load(lss, b, a)
            DR.assert_tracker_delta(tr, b, a, table, table, on_device=False)
        # the attributes alone
        other = DR.other_attrs(table, seed=4)
        tr.set_policy(DR.ls_prefixes(v0, other))
        DR.assert_tracker_delta(tr, v0, v0, table, other, on_device=False)
        with pytest.raises(ValueError):
            tr.set_policy(DR.ls_prefixes(v0, other[:-1]))
        # a node more in area 1: the global ids move, a new baseline
        _, grown = DR.grown_versions()
        assert AR.union(grown)[0] != AR.union(v0)[0]
        DR.ls_load(lss, [None, None], grown)
        back = DR.other_attrs(table, seed=6)
        # the table's global ids are v0's: name the entries before the union grows
        pref = DR.ls_prefixes(v0, back)
        tr.set_policy(pref)  # while the name set differs: not lost
        d = tr.delta()
        assert d["full"] and len(d["changes"]) == 0 and d["rebased"].size == 0 and not d["on_device"]
        DR.assert_tracked(tr, grown, DR.renamed(v0, grown, back))
    finally:
        tr.close()
