"""The KSP2 kernels at their trace and rerun budgets, against the CPU oracle
(DESIGN.md section 2, K1 - K14).

  K1  256 links per path (kStack): P256 / P257 (k = 2 the long way round a
      ring, unit and weighted), L256 / L257 (k = 1 along a chain), under
      every tracer: the decremental kernel, the full reruns, the rows path,
      the single-wave DFS alone, the 16-wave kernels;
  K2  claimed links (kHM): C768 / C800 across the 1,024-slot hash's 768
      (the 16-wave kernel takes over and succeeds), C1536 / C1568 the last
      that fits and the first OVF1, D384 / D392 the decremental kernel's 384
      (392: the `tier` fallback, the same record from the full rerun);
  K3  record words: R at path_cap = n2, n2 - 1, n1, n1 - 1;
  K4  the decremental kernel's ignore list: I256 / I257;
  K5  the source cut: S16 / S17;
  K6  the affected set: A192 / A193;
  K7  the map's keys: F384 / F385;
  K8  the out-links an expansion scans: E4096 / E4097;
  K9  the 16 candidates of a heavy round: H15 .. H65;
  K10 runs per batch and waves per trace block: R's graph queried with
      1 .. 129 destinations;
  K13 the lookahead row length: K16 / K17;
  K14 the last level bytes of the masked multi-source reruns: V252 .. V255;
  and X, one batch of presplit runs and more than 256 fallbacks.

Expected paths are ksp_ref.py's, from the oracle's kth_paths, as link ids of
the LinkState the CSR came from; nothing is compared with another engine
path. test_host_ksp_limits.py proves the shapes sit where this file says."""
import numpy as np
import pytest

import ksp_ref as K
from oracle import Oracle
from openr_amd.engine import Engine
from openr_amd.linkstate import LinkState

pytestmark = pytest.mark.gpu

TRACERS = {
    "default": {},
    "no_decr": {"OSPF_KSP_NODECR": "1"},
    "rows": {"OSPF_KSP_ROWS": "1"},
    "no_heavy": {"OSPF_KSP_NOHEAVY": "1"},
    "heavy": {"OSPF_KSP_BUDGET": "3"},
}
_loaded = {}


def loaded(name):
    """(shape, CSR, {link key: id}) of a shape, made once: read only"""
    if name not in _loaded:
        g = K.shape(name)
        ls = LinkState(stream=g.stream)
        csr = ls.csr()
        assert all(np.array_equal(csr[k], g.csr[k]) for k in csr)
        _loaded[name] = (g, csr, {k: i for i, k in enumerate(ls.link_keys())})
    return _loaded[name]


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def as_ids(ids, ps):
    return [[ids[l] for l in p] for p in ps]


def want_status(name, dst, cap):
    """the status word of one destination from the oracle's paths alone: a
    path past 256 links, claims past 1,536 or a record past `cap` words flags
    its k; a flagged k = 1 flags k = 2; RERUN = k = 1 found a path"""
    k1, k2 = K.paths(name, dst)
    bad = [max(map(len, ps), default=0) > 256 or K.claims(ps) > 1536 or K.record_words(ps) > cap
           for ps in (k1, k2)]
    if bad[0]:
        return K.OVF1 | K.OVF2
    return (K.RERUN if k1 else 0) | (K.OVF2 if bad[1] else 0)


def check_engine(name, dsts=None, cap=None, tag=None, flag_k2=()):
    """Engine.ksp2 of the shape's query (or of `dsts`): exact status words,
    flagged records decode to None, the others are the oracle's paths.
    flag_k2: destinations whose k = 2 must be flagged OVF2 for a budget the
    paths alone do not show (the level bytes). -> the ksp2_stats deltas"""
    g, csr, ids = loaded(name)
    st = K.STATED[name]
    dsts = dsts or [st["dst"]]
    cap = cap or st["cap"]
    eng = Engine(0)
    eng.load({k: v.copy() for k, v in csr.items()})
    try:
        s0 = eng.ksp2_stats()
        k1, k2, status = eng.ksp2(g.ids[st["src"]], [g.ids[d] for d in dsts], path_cap=cap)
        s1 = eng.ksp2_stats()
    finally:
        eng.close()
    for i, d in enumerate(dsts):
        want = want_status(name, d, cap)
        o1, o2 = K.paths(name, d)
        if d in flag_k2:
            want |= K.OVF2
        assert int(status[i]) == want, (name, tag, d, int(status[i]), want)
        assert k1[i] == (None if want & K.OVF1 else as_ids(ids, o1)), (name, tag, d, "k1")
        assert k2[i] == (None if want & (K.OVF1 | K.OVF2) else as_ids(ids, o2)), (name, tag, d, "k2")
    return {k: s1[k] - s0[k] for k in s0}


def both(stream):
    o, p = Oracle(), LinkState()
    assert o.apply(stream) == p.apply(stream)
    p.set_degrade(False)
    return o, p


def check_product(name, dsts=None, tag=None):
    """LinkState.ksp2_text and spf_runs == the oracle's, no engine error and
    no degrading (flagged destinations are answered by the host path)"""
    g, st = K.shape(name), K.STATED[name]
    dsts = dsts or [st["dst"], st["src"], "za" if "za" in g.ids else g.names[1], g.names[-1]]
    o, p = both(g.stream)
    assert p.ksp2_text(st["src"], dsts) == o.ksp2_text(st["src"], dsts), (name, tag)
    assert p.spf_runs == o.spf_runs, (name, tag)
    c = p.counters()
    assert c["engine_errors"] == 0 and c["engine_degraded"] == 0, (name, tag, p.last_engine_error())


# ------------------------------------- every shape: records, status, routing
@pytest.mark.parametrize("name", list(K.BUILD))
def test_engine_records_status_and_routing(name):
    """On each limit and one past it: the exact status word, the oracle's
    paths as link ids, and who answered the k = 2 rerun (ksp2_stats): at the
    limit the decremental kernel, with the stated affected set; one past it
    the full reruns, with the same kind of answer."""
    st = K.STATED[name]
    flag = (st["dst"],) if K.past_levels(name) else ()
    assert want_status(name, st["dst"], st["cap"]) | (K.OVF2 if flag else 0) == st["status"]
    d = check_engine(name, flag_k2=flag)
    route = st["route"]
    assert d["decremental"] == (1 if route == "decr" else 0), (name, d)
    assert d["full_reruns"] == (1 if route in ("full", "presplit") else 0), (name, d)
    # (affected nodes are summed over the runs whose destination the masked
    # rerun still reaches, i.e. the ones with a k = 2 path)
    if route == "decr" and "A" in st and st["k2"][0]:
        assert d["affected"] == st["A"], (name, d)
    if route != "decr" or not st["k2"][0]:
        assert d["affected"] == 0, (name, d)


@pytest.mark.parametrize("name", list(K.BUILD))
def test_product_text_and_spf_runs(name, monkeypatch):
    if K.STATED[name]["cap"] != 1024:
        monkeypatch.setenv("ODL_KSP_CAP", str(K.STATED[name]["cap"]))
    check_product(name)


# ---------------------------------------------------- K1. 256 links per path
@pytest.mark.parametrize("knob", list(TRACERS))
@pytest.mark.parametrize("name", ["P256", "P257", "P256w", "P257w", "L256", "L257"])
def test_k1_path_length_under_every_tracer(name, knob, monkeypatch):
    """256 links are traced and 257 are flagged by each tracer -- OVF2 alone
    where k = 1 fits (P257), OVF1 | OVF2 along the chain (L257). The even
    ring's second destination half-way round has two k = 1 paths of 129."""
    set_env(monkeypatch, TRACERS[knob])
    st = K.STATED[name]
    dsts = [st["dst"]] + (["r0129", "r0128", "fc"] if name.startswith("P257") else [])
    check_engine(name, dsts, tag=knob)
    check_product(name, dsts, tag=knob)


# ------------------------------------------------------- K2. claimed links
@pytest.mark.parametrize("knob", ["no_decr", "no_heavy", "heavy", "rows"])
@pytest.mark.parametrize("name", ["C768", "C800", "C1536", "C1568", "D384", "D392"])
def test_k2_claims_under_the_other_tracers(name, knob, monkeypatch):
    """C800 passes the 1,024-slot hash's 768 claims and must still succeed
    (the 16-wave kernel's hash holds 1,536; without it the single-wave trace
    has the large hash); D392's record from the full reruns == the oracle's."""
    set_env(monkeypatch, TRACERS[knob])
    check_engine(name, tag=knob)


# -------------------------------------------------------- K3. record words
@pytest.mark.parametrize("knob", ["default", "no_decr", "heavy"])
def test_k3_record_words_on_and_past_the_cap(knob, monkeypatch):
    """R's k = 1 record needs n1 = 7 words, its k = 2 record n2 = 9: both fit
    at 9, k = 2 alone is flagged at 8 and at 7, both at 6; never truncated."""
    set_env(monkeypatch, TRACERS[knob])
    n1, n2 = K.R_WORDS
    want = {n2: K.RERUN, n2 - 1: K.RERUN | K.OVF2, n1: K.RERUN | K.OVF2, n1 - 1: K.OVF1 | K.OVF2}
    for cap, status in want.items():
        assert want_status("R", "d", cap) == status
        check_engine("R", ["d", "s", "fc", "za", "u000_001"], cap=cap, tag=(knob, cap))


@pytest.mark.parametrize("cap", [9, 8, 7, 6])
def test_k3_product_at_small_caps(cap, monkeypatch):
    monkeypatch.setenv("ODL_KSP_CAP", str(cap))
    check_product("R", K.shape("R").names, tag=cap)


# ------------------------------------------- K9. heavy candidate rounds
@pytest.mark.parametrize("knob", ["default", "heavy", "no_heavy", "no_decr"])
@pytest.mark.parametrize("fail", [15, 16, 17, 31, 32, 33, 64, 65])
def test_k9_heavy_candidate_rounds(fail, knob, monkeypatch):
    """fail = c - 2 candidates of d fail before the last reaches s over the
    second source link: with a budget of 3 steps nearly all of them are taken
    16 at a time by the 16-wave kernel (a slip in the resume index skips or
    repeats one); the single-wave DFS alone (no_heavy) must give the same,
    the reference's second path. (That the default budget hands 64 failing
    candidates over is observed on the G shapes below.)"""
    set_env(monkeypatch, TRACERS[knob])
    name = f"H{fail}"
    check_engine(name, ["d", f"p{fail + 2:03d}", f"p{fail + 1:03d}", "a000"], tag=knob)
    check_product(name, tag=knob)


# --------------------------------------------------------- K10. batch edges
@pytest.mark.parametrize("knob", ["default", "no_decr"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 128, 129])
def test_k10_batch_edges(n, knob, monkeypatch):
    """1 .. 129 destinations (4 waves per trace block, 64 runs per
    multi-source batch): the list cycles through every node, so it holds s
    itself, island nodes and, from 15 on, duplicates."""
    set_env(monkeypatch, TRACERS[knob])
    g = K.shape("R")
    order = ["d", "s", "za"] + [nm for nm in g.names if nm not in ("d", "s", "za")]
    dsts = [order[i % len(order)] for i in range(n)]
    d = check_engine("R", dsts, tag=(knob, n))
    reruns = sum(1 for x in dsts if K.paths("R", x)[0])
    if knob == "default":  # (OSPF_KSP_NODECR's reruns are not counted)
        assert d["decremental"] + d["full_reruns"] == reruns, (d, reruns)
    check_product("R", dsts, tag=(knob, n))


# -------------------------------------------- K9. the hand-over, observed
@pytest.mark.parametrize("fail", [15, 64, 65])
def test_k9_default_budget_reaches_the_16_wave_kernel(fail, monkeypatch, capfd):
    """G*: the same search in the k = 2 trace of the decremental kernel, whose
    queue for the 16-wave kernel OSPF_KSP_DEBUG's line counts: with 64 and 65
    failing candidates the default budget of 256 steps hands the run over,
    with 15 it does not."""
    monkeypatch.setenv("OSPF_KSP_DEBUG", "1")
    capfd.readouterr()
    d = check_engine(f"G{fail}", tag="debug")
    err = capfd.readouterr().err
    assert d["decremental"] == 1, d
    heavy = [int(ln.split(" heavy ")[1].split()[0]) for ln in err.splitlines() if ln.startswith("ksp2 decr:")]
    # 15 failing candidates cost at most 2 steps per node of their 6-node
    # ways down to b0: 180 steps, within the budget
    assert heavy == [1 if fail >= 64 else 0], err


@pytest.mark.parametrize("knob", ["heavy", "no_heavy", "no_decr"])
@pytest.mark.parametrize("fail", [15, 64, 65])
def test_k9_heavy_rounds_in_the_k2_trace(fail, knob, monkeypatch):
    set_env(monkeypatch, TRACERS[knob])
    check_engine(f"G{fail}", tag=knob)
    check_product(f"G{fail}", tag=knob)


# ------------------------------------------------ K13. lookahead row length
@pytest.mark.parametrize("knob", ["default", "heavy", "no_heavy", "look0"])
@pytest.mark.parametrize("row", [16, 17])
def test_k13_lookahead_row_length(row, knob, monkeypatch):
    """Candidates without an open pathLink whose row has 16 entries (probed
    and marked dead) and 17 (entered, failing), as a call's first candidate
    (the whole wave) and as later lanes'; with the budget of 3 steps the
    16-wave kernel gathers them, each lane probing its own. Without lookahead
    (OSPF_KSP_LOOK=0) every one is entered. The reference's paths each way."""
    set_env(monkeypatch, {"OSPF_KSP_LOOK": "0"} if knob == "look0" else TRACERS[knob])
    check_engine(f"K{row}", ["d", "p003", "p006", "w004_00"], tag=knob)
    check_product(f"K{row}", tag=knob)


# ------------------------------------------------------- K14. level bytes
LEVEL_KNOBS = {
    "default": {},
    "no_decr": {"OSPF_KSP_NODECR": "1"},
    "no_decr_d0": {"OSPF_KSP_NODECR": "1", "OSPF_KSP_D0": "2"},
    "d0": {"OSPF_KSP_D0": "2"},
    "rows": {"OSPF_KSP_ROWS": "1", "OSPF_KSP_NODECR": "1"},
}


@pytest.mark.parametrize("knob", list(LEVEL_KNOBS))
@pytest.mark.parametrize("name", ["V252", "V253", "V254", "V255"])
def test_k14_last_level_bytes(name, knob, monkeypatch):
    """The masked multi-source reruns run the levels 1 .. 253 at most, from
    the first launch or through the +8 continuation from 2 (2, 10, .., 250,
    254): level d finds the nodes at distance d + 1 and writes byte d + 2. So
    masked distances 252, 253 and 254 (bytes 253, 254, 255: the last byte)
    are traced exactly, and 255 is the first the `d >= 254` branch flags --
    OVF2 alone, a record of None, the text from the host path. The rows path
    has no such limit: 255 links fit a path. V252's run is the decremental
    kernel's unless OSPF_KSP_NODECR sends it here; the others' 193 and more
    affected nodes bring them by themselves."""
    set_env(monkeypatch, LEVEL_KNOBS[knob])
    st = K.STATED[name]
    levels = "OSPF_KSP_ROWS" not in LEVEL_KNOBS[knob] and \
        ("OSPF_KSP_NODECR" in LEVEL_KNOBS[knob] or st["route"] == "full")
    flagged = ("t",) if levels and st.get("far", 252) >= 255 else ()
    # (a flagged batch of 64 runs is flagged whole: t's run alone)
    check_engine(name, ["t"] if flagged else ["t", "fc", "c010"], tag=knob, flag_k2=flagged)
    check_product(name, ["t", "fc", "c010", "s"], tag=knob)


# ------------------------------------------------------------ mixed batch
@pytest.mark.parametrize("knob", ["default", "heavy", "no_split"])
def test_mixed_batch_of_presplit_runs_and_fallbacks(knob, monkeypatch):
    """One batch with two presplit runs and 421 runs the decremental kernel
    gives up (more than the 256 a presplit round may take over, kFold).
    Whether they are folded depends on timing: only the results are asserted."""
    set_env(monkeypatch, {"OSPF_KSP_NOSPLIT": "1"} if knob == "no_split" else TRACERS[knob])
    dsts = K.mixed_dsts()
    d = check_engine("X", dsts, tag=knob)
    reruns = sum(1 for x in dsts if K.paths("X", x)[0])
    assert d["decremental"] + d["full_reruns"] == reruns, (d, reruns)
    # 420 tree nodes and ma twice are given up; dp and dq are presplit, and
    # without the presplit only dq's 288 ignored links are past a budget
    assert d["full_reruns"] == 422 + (1 if knob == "no_split" else 2), d
    check_product("X", dsts, tag=knob)
