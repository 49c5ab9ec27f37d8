#!/usr/bin/env python3
"""The delta of the policy selection on the 100k-node fabric, one MI355X.

F100k with 5 % of the announcers drained, the 1,782-prefix table and the "full
policy" attributes of scripts/bench_select_policy.py (three classes, thresholds
0-4). In one process on one box, timed with HIP events around the synchronous
calls, the median of --reps:

  (a) SelState.update_policy after a LINK DOWN (ospf_update_links) + re-sweep;
  (b) update_policy after set_policy (two classes swapped) with no re-sweep;
  (c) the plain SelState.update on the same table and event;
  (d) what a caller without the state does: ospf_sweep_select_policy to the
      host plus a numpy diff of all six columns against the previous result.

The first call after an event carries the changes; the repeats on the same
sweep report none and do the same device work (every entry is selected, stored
and compared). Parity: the records of (a) against the numpy diff of (d)'s two
full results, for every root that was not rebased.

Usage: python scripts/bench_select_policy_delta.py [--out profiles/r10/select_policy_delta_f100k.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import selpolicy_ref as PR  # noqa: E402
from bench_select_policy import csr_table, log, table_of  # noqa: E402
from openr_amd import topology as T  # noqa: E402
from openr_amd.adjdb import AdjDbStream  # noqa: E402
from openr_amd.engine import Engine, SelState, Sweep  # noqa: E402
from openr_amd.linkstate import LinkState  # noqa: E402

COLS = ("metric", "count", "links", "need", "best")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10",
                                                  "select_policy_delta_f100k.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_policy_delta.py needs an MI355X: no HIP device")

    t0 = time.time()
    plain_st = T.fabric(pods=args.pods, planes=args.planes)
    ls = LinkState()
    ls.apply(plain_st)
    names = ls.node_names()
    table = table_of(names, args.seed)
    off, nodes = csr_table(table)
    # 5 % of the announcers drained, as bench_select_policy.py's case (c)
    rng = np.random.default_rng(args.seed + 1)
    ann = np.unique(nodes)
    drained = rng.choice(ann, size=max(1, ann.size // 20), replace=False)
    cols = dict(plain_st.cols)
    ov = cols["db_overloaded"].copy()
    by_name = {plain_st.strings[s]: i for i, s in enumerate(cols["db_name"])}
    for v in drained.tolist():
        ov[by_name[names[v]]] = 1
    cols["db_overloaded"] = ov
    ls = LinkState()
    ls.apply(AdjDbStream(plain_st.strings, cols))
    assert ls.node_names() == names
    csr = ls.csr()
    V, P = len(names), len(table)
    pref, mnh = PR.random_policy(table, rng, classes=3, max_need=4)
    fpref, fmnh = PR.flat(pref), PR.flat(mnh)
    swapped = np.where(fpref == 0, 1, np.where(fpref == 1, 0, fpref)).astype(np.uint32)
    log(f"graph: V={V} P={P} announcers={nodes.size} drained={drained.size} in {time.time() - t0:.1f}s")
    # the event: the first link of a rack in the middle (rack -- fabric switch)
    rack = [i for i, nm in enumerate(names) if nm.startswith("3-")][V // 3]
    e = int(csr["row_ptr"][rack])
    link = (int(csr["link_id"][e]), 0, int(csr["metric"][e]), int(csr["metric"][csr["twin"][e]]))
    if rack > int(csr["col"][e]):
        link = (link[0], 0, link[3], link[2])

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    eng = Engine()
    eng.load(csr, version=1)
    sw = Sweep(eng, hip_graph=False)
    sw.run()
    eng.sync()
    W = sw.max_nh_words

    def by_node(sweep, arrs):
        out = {}
        for k, a in arrs.items():
            b = np.empty_like(a)
            b[sweep.roots] = a
            out[k] = b
        return out

    def diff(prev, now):
        mask = (prev["nh"] != now["nh"]).any(axis=2)
        for k in COLS:
            mask |= prev[k] != now[k]
        return mask

    before = by_node(sw, sw.select_policy(off, nodes, fpref, fmnh, W))
    pst = SelState(eng, off, nodes, fpref, fmnh)
    plain = SelState(eng, off, nodes)
    prime_ms = timed(lambda: pst.prime(sw), 1 + args.reps)[1:]
    plain.prime(sw)
    policy_bytes, plain_bytes = pst.device_bytes, plain.device_bytes
    sw.close()
    eng.update_links([link], version=2)
    sw = Sweep(eng, hip_graph=False)
    sw.run()
    eng.sync()

    def update(state, fn_name, box):
        cap = 1 << 16
        while True:
            try:
                box["r"] = getattr(state, fn_name)(sw, cap=cap, cap_rebased=64, nh_words=W)
                return
            except Exception as ex:  # SelStateOverflow: the complete counts, retry
                if getattr(ex, "code", 0) != -4:
                    raise
                cap = max(cap * 2, ex.n_changes)

    # (a) and (c): the first update carries the event, the repeats the same device work
    ga, gc = {}, {}
    a_first = timed(lambda: update(pst, "update_policy", ga), 1)[0]
    a_ms = timed(lambda: pst.update_policy(sw, cap=16, cap_rebased=16, nh_words=W), args.reps)
    c_first = timed(lambda: update(plain, "update", gc), 1)[0]
    c_ms = timed(lambda: plain.update(sw, cap=16, cap_rebased=16, nh_words=W), args.reps)
    rec, nh, reb = ga["r"]
    # (d): the full policy select to the host and a numpy diff, the caller's way today
    gd = {}

    def caller():
        now = by_node(sw, sw.select_policy(off, nodes, fpref, fmnh, W))
        gd["now"], gd["mask"] = now, diff(before, now)

    d_ms = timed(caller, args.reps)
    mask = gd["mask"].copy()
    mask[reb] = False
    now = gd["now"]
    want = {(int(r), int(p)): tuple(int(now[k][r, p]) for k in COLS) + (tuple(now["nh"][r, p].tolist()),)
            for r, p in np.argwhere(mask)}
    have = {(int(x["root"]), int(x["prefix"])): tuple(int(x[k]) for k in COLS) + (tuple(nh[i].tolist()),)
            for i, x in enumerate(rec)}
    # (b): set_policy with the same sweep
    gb = {}
    pst.set_policy(swapped, fmnh)
    b_first = timed(lambda: update(pst, "update_policy", gb), 1)[0]
    b_ms = timed(lambda: pst.update_policy(sw, cap=16, cap_rebased=16, nh_words=W), args.reps)
    med = lambda x: float(np.median(x))  # noqa: E731
    res = dict(topology=f"fabric pods={args.pods} planes={args.planes}", V=V, n_prefixes=P,
               n_announcers=int(nodes.size), drained=int(drained.size), nh_words=W,
               device=torch.cuda.get_device_name(0), event="one rack--fabric link down",
               prime_ms=prime_ms,
               a_update_policy_first_ms=a_first, a_update_policy_ms=a_ms, a_ms_median=med(a_ms),
               a_changes=int(len(rec)), a_rebased=int(len(reb)),
               b_set_policy_first_ms=b_first, b_set_policy_ms=b_ms, b_ms_median=med(b_ms),
               b_changes=int(len(gb["r"][0])),
               c_plain_update_first_ms=c_first, c_plain_update_ms=c_ms, c_ms_median=med(c_ms),
               c_changes=int(len(gc["r"][0])),
               d_select_policy_host_diff_ms=d_ms, d_ms_median=med(d_ms),
               policy_state_device_bytes=int(policy_bytes), plain_state_device_bytes=int(plain_bytes),
               a_over_c=med(a_ms) / med(c_ms), a_over_d=med(a_ms) / med(d_ms),
               parity_changed=len(want), parity_ok=bool(have == want))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    pst.close()
    plain.close()
    sw.close()
    eng.close()
    if not res["parity_ok"]:
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
