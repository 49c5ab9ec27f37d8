"""The multi-area selection kernels at their area and entry limits
(areas_kernel, areas_delta_kernel and the device functions of
spf_selareas_dev.h): 32 areas and bit 31 of the mask, the 64-entry step of
walk 4, metrics of 2^31 and above across areas, the packed link counts of a
wide area that is not the first, a 4-word root in the resident state and the
class word 0xFFFFFFFF.

The fixtures, and the asserts on the expectation that make each a limit case,
are in areas_limits.py (areas_limits.case runs them before anything is asked
of the engine). Expected values come from areas_ref.expect and areas_delta_ref
over the CPU oracle's SPF of every area -- never the engine's rows or its key;
test_host_areas_limits.py proves the same expectation against the product's
route build without a GPU. Every comparison is exact."""
import contextlib

import numpy as np
import pytest
import torch

import areas_delta_ref as DR
import areas_limits as L
import areas_ref as AR
from openr_amd.adjdb import AdjDbStream
from openr_amd.engine import (Engine, EngineError, Sweep, select_policy_areas,
                              select_policy_areas_dev)
from openr_amd.linkstate import LinkState, all_areas_select_policy
from test_gpu_select_areas import GUARD, HDR, dev_buffer, run_sweeps, select
from test_gpu_select_areas_delta import Dev, state, step
from test_host_select_areas import product_tables

pytestmark = pytest.mark.gpu

POISON = np.uint32(0xA5A5A5A5)
MODES = ("batch", "derive", "wderive")
ALL = AR.KEYS + ("nh",)


@contextlib.contextmanager
def loaded(areas):
    """the areas with an Engine each holding the area's graph"""
    out = []
    try:
        for a in areas:
            eng = Engine()
            out.append(dict(a, eng=eng))
            eng.load(a["csr"])
        yield out
    finally:
        for a in out:
            a["eng"].close()


# The one fixture whose sweeps do not capture a HIP graph: 32 contexts alive at
# once, two of them (areas 5 and 6) with two width classes, i.e. a captured
# graph with parallel branches. With the default graph sweeps the replay of one
# of them (ospf_sweep_run -> hipGraphLaunch, after the same sweep's eager run
# at creation had succeeded) ended the process with a segmentation fault on an
# MI355X. The cause is not found ("Graph sweeps with many
# live contexts"); 32 one-class contexts and a few contexts with several
# classes replay their graphs here and in the other areas tests.
NO_GRAPH = {"straddle-wide"}


def eager_sweep(eng, mode):
    """a run sweep without a captured HIP graph: every run queues its launches
    one by one (for NO_GRAPH's fixture only)"""
    sw = Sweep(eng, mode=mode, hip_graph=False)
    try:
        sw.run()
        eng.sync()
    except EngineError:
        sw.close()
        raise
    return sw


@contextlib.contextmanager
def swept(areas, mode, graph=True):
    """one run sweep per area (the default graph sweeps of run_sweeps, or
    eager_sweep's), or None where an area's contract does not admit the mode
    (EngineError -4 at sweep creation)"""
    sws = []
    try:
        if graph:
            sws = run_sweeps(areas, mode) or []
            yield sws or None
        else:
            try:
                for a in areas:
                    sws.append(eager_sweep(a["eng"], mode))
            except EngineError as e:
                assert e.code == -4, (mode, e)
                yield None
            else:
                yield sws
    finally:
        for sw in sws:
            sw.close()


def check_modes(c, extra=None):
    """the one-shot kernel in every admitted sweep mode == the expectation;
    `extra(areas, sweeps)` runs once more under the batch sweeps"""
    L.preconditions(c)
    ran = []
    with loaded(c.areas) as areas:
        for mode in MODES:
            with swept(areas, mode, c.name not in NO_GRAPH) as sws:
                if sws is None:
                    continue
                assert tuple(max(1, s.max_nh_words) for s in sws) == c.W
                AR.assert_equal(select(areas, sws, c.table), c.exp, ctx=(c.name, mode))
                if mode == "batch" and extra:
                    extra(areas, sws)
                ran.append(mode)
    assert "batch" in ran, ran
    return ran


# ---------------------------------------------------------------- 32 areas
def guarded_dev_call(c, areas, sws):
    """the _dev call with poisoned words around every output: each wanted word
    is written, no other. The areas column may hold 0xFFFFFFFF: the body is
    compared with the expectation, not searched for the poison."""
    gnames, gids = AR.union(areas)
    G, P, A = len(gnames), len(c.table), len(areas)
    sizes = {k: G * P for k in HDR}
    sizes.update({("nh", a): len(areas[a]["names"]) * P * c.W[a] for a in range(A)})
    bufs = {k: dev_buffer(n) for k, n in sizes.items()}
    ptr = lambda k: bufs[k].data_ptr() + 4 * GUARD  # noqa: E731
    select_policy_areas_dev(sws, gids, G, *AR.csr_table(c.table), c.W,
                            **{f"d_{k}": ptr(k) for k in HDR},
                            d_nh=[ptr(("nh", a)) for a in range(A)])
    torch.cuda.synchronize()
    for k, b in bufs.items():
        h = b.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == POISON).all() and (h[-GUARD:] == POISON).all(), (c.name, k)
        w = c.exp["nh"][k[1]] if isinstance(k, tuple) else c.exp[k]
        assert np.array_equal(h[GUARD:-GUARD], w.reshape(-1)), (c.name, k)


def refused_at_33(c, areas, sws):
    gnames, gids = AR.union(areas)
    G, cols = len(gnames), AR.csr_table(c.table)
    assert len(sws) == 32
    with pytest.raises(EngineError) as e:
        select_policy_areas(sws + sws[:1], gids + gids[:1], G, *cols)
    assert e.value.code == -1
    buf = dev_buffer(64)
    p = buf.data_ptr() + 4 * GUARD
    with pytest.raises(EngineError) as e:
        select_policy_areas_dev(sws + sws[:1], gids + gids[:1], G, *cols, (1,) * 33, d_metric=p,
                                d_areas=p, d_nh=[p] * 33)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == POISON).all()


@pytest.mark.parametrize("name", ["f32", "f32-uniform", "f32-solo"])
def test_32_areas_one_shot(name):
    """bit 31 of the mask, a root whose only area is 31 (filled by thread 31 of
    a one-wave block), all 32 areas tying at mask 0xFFFFFFFF; 32 areas accepted
    and 33 refused with nothing written"""
    c = L.case(name)

    def extra(areas, sws):
        guarded_dev_call(c, areas, sws)
        refused_at_33(c, areas, sws)

    check_modes(c, extra)


def test_metrics_of_bit_31_across_areas():
    """take_area and wave_min compare unsigned: 3 beats 0x80000005, two areas
    tie at 0x80000005, by the lane and by the wave (areas_limits.
    heavy_preconditions states which cells a signed compare gets wrong)"""
    c = L.case("f32-heavy")
    check_modes(c, lambda areas, sws: guarded_dev_call(c, areas, sws))


# ---------------------------------------------------------------- the 64-entry step
@pytest.mark.parametrize("name", ["straddle", "straddle-wide"])
def test_node_across_a_64_entry_step_counts_once(name):
    """y's 32 entries across positions 63 / 64 and 127 / 128: tight_step's carry.
    A wrong carry only doubles count. On a narrow root (area_by_wave) and on a
    root wide in two areas (area_by_words in the winning one, area_by_wave in
    the others); the 8-entry prefix is area_by_lane's prev"""
    check_modes(L.case(name))


# ---------------------------------------------------------------- wide areas behind the first
def test_wide_areas_with_packed_counts_behind_the_first():
    """the hub's link counts of areas 1 and 2 start at 1 and 141 of the packed
    ones: with and without links (another wend), in the roots' widths and padded"""
    c = L.case("fwide")
    padded = (2, 8, 7)
    wide, _ = AR.expect(c.areas, c.table, padded)

    def extra(areas, sws):
        no_links = tuple(k for k in ALL if k != "links")
        got = select(areas, sws, c.table, want=no_links)
        assert "links" not in got
        AR.assert_equal(got, c.exp, keys=no_links, ctx="no links")
        AR.assert_equal(select(areas, sws, c.table, want=("count", "links")), c.exp,
                        keys=("count", "links"), ctx="links, no words")
        AR.assert_equal(select(areas, sws, c.table, nh_words=padded), wide, ctx="padded")
        AR.assert_equal(select(areas, sws, c.table, nh_words=padded, want=no_links), wide,
                        keys=no_links, ctx="padded, no links")
        guarded_dev_call(c, areas, sws)

    check_modes(c, extra)


# ---------------------------------------------------------------- the class word
def test_class_word_all_ones_is_not_the_missing_key():
    """rank 2^31 - 1 on a node drained in its own area: the key's high word is
    0xFFFFFFFF as kNoKey's is, and the entry is the only reached one"""
    check_modes(L.case("classtop"))


# ---------------------------------------------------------------- the resident state
class EagerDev(Dev):
    """Dev with eager_sweep's sweeps (for NO_GRAPH's fixture only)"""

    def resweep(self, a, hop=None):
        if self.sws[a] is not None:
            self.sws[a].close()
            self.sws[a] = None
        self.sws[a] = eager_sweep(self.engs[a], self.mode)
        return self.sws[a]


@contextlib.contextmanager
def primed(areas, table, graph=True):
    """(Dev, AreaSelState) primed with the areas' batch sweeps"""
    dev, st = (Dev() if graph else EagerDev()), None
    try:
        sws = dev.load(areas)
        st = state(sws, areas, table)
        st.prime(sws)
        yield dev, st
    finally:
        if st is not None:
            st.close()
        dev.close()


def test_state_at_32_areas():
    c = L.case("f32")
    L.preconditions(c)
    v0, v1, v2 = L.f32_versions()
    table, W = c.table, c.W
    G, P = c.exp["metric"].shape
    with primed(v0, table) as (dev, st):
        DR.assert_state(st, v0, c.exp, W, what="prime")
        rec, nh, reb = st.update(dev.sws, cap=8, cap_rebased=4, nh_words=W)
        assert len(rec) == 0 and reb.size == 0
        # area 31 alone is swept again: bit 31 appears, and area 31's words are
        # the last of a record's row
        kept = list(dev.sws)
        changed, rebased, ea = step(st, dev, v0, v1, table, table, what="area 31")
        assert [s is k for s, k in zip(dev.sws, kept)] == [True] * 31 + [False]
        assert not rebased and any(ea["areas"][cell] >> 31 for cell in changed)
        assert any(DR.by_global(v1, ea)[r, p, -1] for r, p in changed)
        # then area 0 alone
        kept = list(dev.sws)
        _, rebased, _ = step(st, dev, v1, v2, table, table, what="area 0")
        assert [s is k for s, k in zip(dev.sws, kept)] == [False] + [True] * 31 and not rebased
        # area 31's entries alone in the best class
        other = L.best_in_31(table)
        changed, rebased, ea, _ = DR.delta(v2, v2, table, other, W)
        x = L.gid_of(v2)["x"]
        assert (x, 0) in changed and ea["areas"][x, 0] == 0x80000000 and not rebased
        _, _, _, pref, mnh = AR.csr_table(other)
        st.set_policy(pref, mnh)
        rec, nh, reb = st.update(dev.sws, cap=G * P, cap_rebased=4, nh_words=W)
        assert DR.records(rec, nh) == DR.wanted(v2, changed, ea) and reb.size == 0
        DR.assert_state(st, v2, ea, W, what="set_policy")


def test_state_wide_areas_behind_the_first():
    """a metric bump in area 2 only: the words of areas 1 and 2 come from their
    own ranges of the block and of a record's row"""
    c = L.case("fwide")
    L.preconditions(c)
    after = L.fwide(bump=True)
    assert [a is b for a, b in zip(c.areas, after)] == [True, True, False]
    with primed(c.areas, c.table) as (dev, st):
        DR.assert_state(st, c.areas, c.exp, c.W, what="prime")
        changed, rebased, ea = step(st, dev, c.areas, after, c.table, c.table)
        hub = L.gid_of(after)["hub"]
        mine = {p for r, p in changed if r == hub}
        assert not rebased and L.FWIDE_ONLY2 in mine and len(mine) < len(c.table)
        # a changed cell of the hub that keeps next hops in both wide areas
        nh = DR.by_global(after, ea)[hub]
        assert any(nh[p, 1:6].any() and nh[p, 6:].any() for p in mine)


@pytest.mark.parametrize("P", [63, 64, 65])
def test_state_4_word_root(P):
    """store_chunk_words' 16-B path and its plain path: the hub's 4 words lie
    behind 7 P words of its block, aligned with P = 64 and not with 63 and 65"""
    c = L.case(f"f4w-{P}")
    L.preconditions(c)
    assert len(c.table) == P
    after = L.f4w(down=True)
    with primed(c.areas, c.table) as (dev, st):
        DR.assert_state(st, c.areas, c.exp, c.W, what="prime")
        changed, rebased, _ = step(st, dev, c.areas, after, c.table, c.table)
        assert not rebased and L.gid_of(after)["hub"] in {r for r, _ in changed}


@pytest.mark.parametrize("name", ["straddle", "straddle-wide"])
def test_state_node_across_a_64_entry_step(name):
    c = L.case(name)
    L.preconditions(c)
    with primed(c.areas, c.table, name not in NO_GRAPH) as (dev, st):
        x = L.gid_of(c.areas)["x"]
        got = st.copy([x], c.W)
        assert np.array_equal(got["count"], c.exp["count"][[x]])
        DR.assert_state(st, c.areas, c.exp, c.W)


# ---------------------------------------------------------------- the LinkState call
def test_linkstate_call_over_32_areas_on_the_device():
    c = L.case("f32")
    L.preconditions(c)
    lss = []
    for a in c.areas:
        ls = LinkState(area=a["name"])
        ls.set_degrade(True)
        ls.apply(AdjDbStream.from_dbs(a["dbs"]))
        lss.append(ls)
    _, policy = product_tables(c.areas, c.table)
    got = all_areas_select_policy(lss, policy)
    assert got["on_device"] and got["names"] == AR.union(c.areas)[0]
    assert got["area_names"] == [a["name"] for a in c.areas]
    AR.assert_equal(got, c.exp)
    assert np.array_equal(got["installed"], c.exp["installed"])
    assert all(ls.counters()["engine_errors"] == 0 for ls in lss)
    assert all(ls.counters()["engine_degraded"] == 0 for ls in lss)
