"""The policy selection kernels at their word, key and count limits
(policy_kernel, seldelta_policy_kernel, srmpls_kernel and the device functions
of spf_selpolicy_dev.h): keys and thresholds with bit 31 set on the wave paths,
a root of exactly kSelLaneW = 4 next-hop words, a root of 66 words, and 65,535
/ 65,536 parallel links behind a 16-bit slot count.

The fixtures, and the asserts on the expectation that make each a limit case,
are in policy_limits.py (policy_limits.case runs them before anything is asked
of the engine). Expected values come from selpolicy_ref.expect,
srmpls_ref.expect and policy_delta_ref over the CPU oracle's SPF -- never the
engine's rows or its key; test_host_policy_limits.py proves the same
expectation against the product's host path without a GPU. Every comparison
is exact. Per fixture and admitted sweep mode all three kernels run: the
one-shot calls into poisoned device buffers with guards, the resident state
primed and then updated. One engine is alive at a time."""
import numpy as np
import pytest
import torch

import policy_delta_ref as PD
import policy_limits as L
import select_ref as R
import selpolicy_ref as PR
import srmpls_ref as SR
from openr_amd.engine import Engine, EngineError, SelState, Sweep
from test_gpu_select_delta import Rig
from test_gpu_select_srmpls import FF, GUARD, select_dev

pytestmark = pytest.mark.gpu

MODES = ("batch", "wderive", "wcover")


def policy_dev(sw, c, W, skew=0):
    """select_policy_dev into poisoned buffers (nh `skew` words off 16 B) ->
    the outputs by node id; the guards must be untouched"""
    off, nodes = R.csr_table(c.table)
    n, P = sw.n_roots, len(c.table)
    bufs = {}
    for k in PR.KEYS:
        first = GUARD + (skew if k == "nh" else 0)
        shp = (n, P, W) if k == "nh" else (n, P)
        t = torch.full((first + int(np.prod(shp)) + GUARD,), -1, dtype=torch.int32, device="cuda")
        bufs[k] = (t, first, shp)
    torch.cuda.synchronize()
    sw.select_policy_dev(off, nodes, PR.flat(c.pref), PR.flat(c.mnh), W,
                         **{f"d_{k}": t.data_ptr() + 4 * first for k, (t, first, _) in bufs.items()})
    torch.cuda.synchronize()
    out = {}
    for k, (t, first, shp) in bufs.items():
        h = t.cpu().numpy().view(np.uint32)
        words = int(np.prod(shp))
        assert (h[:first] == FF).all() and (h[first + words:] == FF).all(), (c.name, k)
        full = np.zeros((sw.engine.V,) + shp[1:], np.uint32)
        full[sw.roots] = h[first:first + words].reshape(shp)
        out[k] = full
    return out


def rows_of(arrs, roots, keys):
    return {k: arrs[k][roots] for k in keys}


def one_shot(c, sw, W, skew=0, ctx=""):
    """policy_kernel and srmpls_kernel at output width W == the expectation,
    on the judged roots the sweep owns (the guards are checked for all)"""
    roots = sorted(set(c.judged) & set(sw.roots.tolist()))
    assert roots
    ctx = (c.name, ctx, W, skew)
    PR.assert_equal(rows_of(policy_dev(sw, c, W, skew), roots, PR.KEYS),
                    rows_of(c.pol(W), roots, PR.KEYS), ctx=ctx)
    got = select_dev(sw, c.table, c.pref, c.mnh, c.flags, W, skew=skew)
    SR.assert_equal(rows_of(got, roots, SR.KEYS), rows_of(c.sr(W)[0], roots, SR.KEYS), ctx=ctx)


def host_call(c, sw):
    """Sweep.select_policy (host outputs, the sweep's own width)"""
    off, nodes = R.csr_table(c.table)
    got = sw.select_policy(off, nodes, PR.flat(c.pref), PR.flat(c.mnh))
    W = max(1, sw.max_nh_words)
    at = {int(r): i for i, r in enumerate(sw.roots)}
    roots = [r for r in c.judged if r in at]
    PR.assert_equal({k: got[k][[at[r] for r in roots]] for k in PR.KEYS},
                    rows_of(c.pol(W), roots, PR.KEYS), ctx=(c.name, "host outputs"))


def update(st, sw, c, W, before, after, ctx=""):
    """one update_policy read at width W == the expected delta on the judged
    roots (other roots' records are not judged); -> the records"""
    changed, rebased, ea, _ = c.delta(W, before, after)
    V, P = c.base.V, len(c.table)
    rec, nh, reb = st.update_policy(sw, cap=V * P, cap_rebased=4, nh_words=W)
    assert sorted(reb.tolist()) == rebased == [], (c.name, ctx)
    keep = np.isin(rec["root"], c.judged)
    got, want = PD.records(rec[keep], nh[keep]), PD.wanted(changed, ea)
    assert set(got) == set(want), (c.name, ctx, sorted(set(got) ^ set(want))[:8])
    assert got == want, (c.name, ctx, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:3])
    PD.assert_state(st, ea, W, roots=c.judged, what=(c.name, ctx))
    return got


def run_fixture(c, widths, modes=MODES, steps=((0, 1, None),), extra=None):
    """Per admitted sweep mode: the one-shot kernels at every width, then the
    resident state primed and walked through `steps` (before, after, width of
    the read; None: the graph's). extra(rig, sw) runs under the batch sweep.
    EngineError -4 at sweep creation skips the mode; batch must run."""
    L.preconditions(c)
    off, nodes = R.csr_table(c.table)
    W0 = c.base.words
    ran = []
    for mode in modes:
        rig, st = Rig(mode), None
        try:
            sw = rig.sweep(c.base)
            if sw is None:
                continue
            assert max(1, sw.max_nh_words) == W0
            for W in widths:
                one_shot(c, sw, W, ctx=mode)
            if mode == "batch":
                host_call(c, sw)
                if extra:
                    extra(rig, sw)
            st = SelState(rig.eng, off, nodes, PR.flat(c.pref), PR.flat(c.mnh))
            st.prime(sw)
            PD.assert_state(st, c.pol(W0), W0, roots=c.judged, what=(c.name, mode, "prime"))
            if len(c.versions) == 1:  # nothing moved: nothing reported
                rec, _, reb = st.update_policy(sw, cap=8, cap_rebased=4, nh_words=W0)
                assert len(rec) == 0 and len(reb) == 0
            else:
                for before, after, W in steps:
                    sw = rig.sweep(c.versions[after])
                    assert sw is not None
                    update(st, sw, c, W or W0, before, after, ctx=(mode, after))
            ran.append(mode)
        finally:
            if st is not None:
                st.close()
            rig.close()
    print(f"{c.name}: sweep modes {ran}")
    assert "batch" in ran, ran
    return ran


# ---------------------------------------------------------------- L1
def test_keys_and_thresholds_with_bit_31_on_the_wave_paths():
    """wave_min64 / wave_max and the lanes' 64-bit folds with bit 31 set in
    either half, on the lane-per-announcer path (root a1) and the lane-per-word
    path (root a), in policy_min, sr_entry<true> and class_fold. Catches: `min`
    on int in wave_min (either half of the key), the low half reduced before
    the high one, `max` on int in wave_max (a threshold of 0x80000000 or
    0xFFFFFFFF loses to 5), a signed `key < m` in a lane's fold -- each changes
    a metric, best or need cell of both roots (policy_limits.l1_preconditions
    proves it from the oracle's numbers)."""
    c = L.case("L1")
    ran = run_fixture(c, widths=(5, 8))
    assert ran, "no sweep mode admits the 0x7FFFFFFF metric"


# ---------------------------------------------------------------- L2
def four_word_parts(c, rig, sw):
    """Wout = 4 needs a sweep without the five-word root: the half of the
    roots that owns a four-word hub and not h5. Wout = 4 and 8 take the 16-B
    stores, 4 through a pointer one word off 16 B the plain ones."""
    hubs = {c.focus["h4"], c.focus["g4"]}
    ran = 0
    for part in (0, 1):
        ps = Sweep(rig.eng, mode="batch", part=part, n_parts=2)
        try:
            ps.run()
            rig.eng.sync()
            if ps.max_nh_words != 4 or not hubs & set(ps.roots.tolist()):
                continue
            assert c.focus["h5"] not in ps.roots.tolist()
            for W, skew in ((4, 0), (4, 1), (8, 0)):
                one_shot(c, ps, W, skew, ctx=("part", part))
            ran += 1
        finally:
            ps.close()
    assert ran, "no half of the roots owns a four-word root without the five-word one"


def test_root_of_exactly_four_words_beside_one_of_five():
    """Word 3 of a kSelLaneW-word root. Catches: dropping `v.w = acc[3]` in
    store_chunk_words' 16-B store, `k < 3` in its plain store, `w < 3` in
    links_of (p100's two links sit in slot 100), `w < 3` in the word compare
    of seldelta_policy_kernel (the second update moves z from behind p106 and
    p108 to behind p108 and p112: h4's entry keeps its header and changes word
    3 only, so nothing else reports it), a chg_nh record written without
    acc[3] -- and a five-word root taking the four-word path (W <= kSelLaneW
    off by one). P = 65: a chunk of 64 prefixes and a tail of one."""
    c = L.case("L2")
    h4 = c.focus["h4"]

    def extra(rig, sw):
        assert rig.eng.nh_words(h4) == 4 and rig.eng.nh_words(c.focus["h5"]) == 5
        one_shot(c, sw, 5, skew=1, ctx="skewed")
        four_word_parts(c, rig, sw)

    run_fixture(c, widths=(5, 8), steps=((0, 1, None), (1, 2, None)), extra=extra)


# ---------------------------------------------------------------- L3
def test_root_of_66_words():
    """The hub's words cross the 64-word block. Catches: `wb == 0` guarding the
    gather instead of the count in policy_by_words (words 64, 65 stay zero, or
    count doubles), `w < W` / `w < Wout` swapped at the third, padding-only
    block (Wout = 130), `x / Wout` with Wout > 64 and the `w += 64` link sum in
    sr_write_by_words, cslot[b] with b >= 2048, `w < 64` in the delta kernel's
    compare (the hub's [x] entry changes in word 64 only: no record), the
    by-wave chg_nh record at nh_words 66 and 130. The oracle answers for the
    hub and six other roots; the other roots' cells are not judged, the guards
    are."""
    c = L.case("L3")
    hub = c.focus["hub"]
    changed, _, ea, _ = c.delta(130, 1, 0)  # the way back, read at 130 words
    assert (hub, L.L3_X) in changed and not ea["nh"][hub, L.L3_X, 66:].any()

    def extra(rig, sw):
        assert rig.eng.nh_words(hub) == 66

    # v0 -> v1 read at 66 words, v1 -> v0 read at 130
    run_fixture(c, widths=(66, 67, 130), steps=((0, 1, 66), (1, 0, 130)), extra=extra)


# ---------------------------------------------------------------- L4
L4_MODES = MODES + ("derive",)  # the graph is unit


def test_65535_parallel_links_are_counted_exactly():
    """OSPF_MAX_PARALLEL_LINKS links r = x: build_links' u16 pack holds 0xFFFF
    itself, not a cap. Catches: a pack to fewer bits, a cap one too low, a
    threshold of 65,535 compared against a wrapped count."""
    run_fixture(L.case("L4-65535"), widths=(1,), modes=L4_MODES)


def test_patch_to_65536_parallel_links_is_refused_and_the_graph_stays():
    """ospf_update_rows with one link more than OSPF_MAX_PARALLEL_LINKS between
    r and x: OSPF_E_RANGE, and the loaded graph of 65,535 links still answers
    65,535 in a new sweep. Catches: the limit checked at ospf_load_graph only,
    so that a patch brings the 16-bit pack's cap within reach."""
    fits, over = L.case("L4-65535"), L.case("L4-65536")
    r, x = fits.focus["r"], fits.focus["x"]
    off, nodes = R.csr_table(fits.table)
    eng = Engine()
    try:
        eng.load(fits.base.csr)
        with pytest.raises(EngineError) as ei:
            eng.update_rows(over.base.csr, [r, x], 2)
        assert ei.value.code == -4 and "parallel" in str(ei.value), ei.value
        sw = Sweep(eng, mode="batch")
        try:
            sw.run()
            eng.sync()
            got = sw.select_policy(off, nodes, PR.flat(fits.pref), PR.flat(fits.mnh))
            at = sw.roots.tolist().index(r)
            assert got["links"][at].tolist() == fits.pol(1)["links"][r].tolist()
            assert got["links"][at, 0] == L.L4_FITS
        finally:
            sw.close()
    finally:
        eng.close()


def test_65536_parallel_links_are_refused_or_exact():
    """One link more than a slot's 16 bits hold: the load refuses the graph with
    OSPF_E_RANGE (include/openr_spf.h, OSPF_MAX_PARALLEL_LINKS) -- or, should
    the count ever be widened, every kernel answers 65,536. A silent 65,535
    (`min(c32, 0xFFFF)` reached) is the failure."""
    c = L.case("L4-65536")
    eng = Engine()
    try:
        eng.load(c.base.csr)
    except EngineError as e:
        assert e.code == -4 and "parallel" in str(e), e
        # nothing is loaded: no sweep, nothing written
        with pytest.raises(EngineError) as ei:
            Sweep(eng, mode="batch")
        assert ei.value.code == -2
        # the engine still takes the graph one link below
        fits = L.case("L4-65535")
        eng.load(fits.base.csr, version=2)
        assert eng.nh_words(fits.focus["r"]) == 1
        return
    finally:
        eng.close()
    run_fixture(c, widths=(1,), modes=L4_MODES)
