#!/usr/bin/env python3
"""The multi-area selection kept resident (ospf_areastate_*) on the 100k-node
fabric in two areas, one MI355X: what a link event costs as a delta on the
device against the full ospf_areas_select_policy_dev call.

The fabric, its two areas (they share the spines) and the table are
bench_select_areas.py's. The event is one rack -- fabric-switch link of area
a0 going down (ospf_update_links in place), a0 swept again, a1's sweep reused;
it is then brought up and taken down again, so three updates are timed. Wall
clock around the synchronous calls, median of three:

  prime         AreaSelState.prime on the base sweeps
  update        AreaSelState.update after down / up / down (+ re-sweep of a0,
                not in the time)
  full          select_policy_areas_dev on the same sweeps, in this process
                (HIP events, after one untimed launch): the comparator
  attrs         set_policy with classes 0 and 1 swapped, then update with the
                same sweeps

Parity (the only pass condition): the changed set and the new values of the
last down event, and of the attribute change, equal the diff of two full
device selections -- areas_kernel's, not the code under test -- taken before
and after, compared on the device; the committed cells of a sample of roots
are read back with copy and compared with the selection after.

Usage: python scripts/bench_select_areas_delta.py [--out profiles/r12/select_areas_delta_f100k.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_select_areas import area_streams, csr_of, table_of, union  # noqa: E402
from openr_amd.engine import (AreaSelState, Engine, SelStateOverflow, Sweep,  # noqa: E402
                              select_policy_areas_dev)
from openr_amd.linkstate import LinkState  # noqa: E402

HDR = ("metric", "count", "links", "need", "best", "areas")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class Area:
    def __init__(self, name, stream_):
        t0 = time.time()
        ls = LinkState(area=name)
        ls.apply(stream_)
        self.names, self.csr = ls.node_names(), ls.csr()
        self.eng = Engine()
        self.eng.load(self.csr)
        self.ver = 1
        self.sw = None
        self.sweep()
        log(f"area {name}: V={self.eng.V} mode={self.sw.mode} W={self.W} in {time.time() - t0:.1f}s")

    def sweep(self):
        if self.sw is not None:
            self.sw.close()
        self.sw = Sweep(self.eng, hip_graph=False)
        self.sw.run()
        self.eng.sync()
        self.W = max(1, self.sw.max_nh_words)

    def close(self):
        self.sw.close()
        self.eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12",
                                                  "select_areas_delta_f100k.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_areas_delta.py needs an MI355X: no HIP device")
    stream = torch.cuda.Stream()

    areas = [Area(f"a{i}", st) for i, st in enumerate(area_streams(args.pods, args.planes))]
    torch.cuda.synchronize()
    names = [a.names for a in areas]
    gnames, gids = union(names)
    gix = {n: i for i, n in enumerate(gnames)}
    G, table = len(gnames), table_of(names, args.seed)
    P = len(table)
    off, rows = csr_of(table, lambda e: (gix[e[0]], e[1]))
    col = lambda f: np.array([f(e) for r in rows for e in r], np.uint32)  # noqa: E731
    t_node, t_area = col(lambda e: gix[e[0]]), col(lambda e: e[1])
    t_pref, t_mnh = col(lambda e: e[2]), col(lambda e: e[3])
    swapped = np.where(t_pref == 0, 1, np.where(t_pref == 1, 0, t_pref)).astype(np.uint32)
    Ws = [a.W for a in areas]
    log(f"union: G={G} P={P} entries={t_node.size} words={Ws}")
    d_gid = [torch.from_numpy(g.astype(np.int64)).cuda() for g in gids]
    lid = []
    for g in gids:
        x = np.full(G, -1, np.int64)
        x[g] = np.arange(g.size)
        lid.append(x)

    # ---- the full call: the comparator, and the reference of the parity check
    new = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device="cuda")  # noqa: E731

    def buffers():
        return {k: new(G, P) for k in HDR}, [new(a.eng.V, P, w) for a, w in zip(areas, Ws)]

    def full(bufs, pref):
        hdr, nh = bufs
        select_policy_areas_dev([a.sw for a in areas], gids, G, off, t_node, t_area, pref, t_mnh,
                                Ws, **{f"d_{k}": hdr[k].data_ptr() for k in HDR},
                                d_nh=[x.data_ptr() for x in nh], stream=stream.cuda_stream)

    def full_ms(bufs, pref):
        full(bufs, pref)  # untimed: row table upload, code load
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            full(bufs, pref)
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def changed_mask(b0, b1, rebased):
        """[G, P] bool on the device: any column or any area's word differs"""
        mask = torch.zeros((G, P), dtype=torch.bool, device="cuda")
        for k in HDR:
            mask |= b0[0][k] != b1[0][k]
        for a in range(len(areas)):
            mask[d_gid[a]] |= (b0[1][a] != b1[1][a]).any(dim=2)
        if len(rebased):
            mask[torch.from_numpy(np.asarray(rebased, np.int64)).cuda()] = False
        return mask

    def parity(rec, nh, rebased, b0, b1, what):
        """records == the diff of the two full selections, values from the second"""
        mask = changed_mask(b0, b1, rebased)
        want = mask.nonzero().cpu().numpy()
        got = np.stack([rec["root"].astype(np.int64), rec["prefix"].astype(np.int64)], axis=1)
        order = np.lexsort((got[:, 1], got[:, 0]))
        ok = got.shape == want.shape and bool(np.array_equal(got[order], want))
        r = torch.from_numpy(got[:, 0]).cuda()
        p = torch.from_numpy(got[:, 1]).cuda()
        for k in HDR:
            v = b1[0][k][r, p].cpu().numpy().view(np.uint32)
            ok = ok and bool(np.array_equal(v, rec[k]))
        o = 0
        for a in range(len(areas)):
            la = lid[a][got[:, 0]]
            here = la >= 0
            exp = np.zeros((got.shape[0], Ws[a]), np.uint32)
            if here.any():
                rows_ = b1[1][a][torch.from_numpy(la[here]).cuda(), p[torch.from_numpy(here).cuda()]]
                exp[here] = rows_.cpu().numpy().view(np.uint32)
            ok = ok and bool(np.array_equal(nh[:, o:o + Ws[a]], exp))
            o += Ws[a]
        log(f"parity of {what}: {got.shape[0]} records against {want.shape[0]} changed cells: {ok}")
        return ok

    def parity_copy(st, b1, roots, what):
        got = st.copy(roots, Ws)
        r = torch.from_numpy(np.asarray(roots, np.int64)).cuda()
        ok = True
        for k in HDR:
            ok = ok and bool(np.array_equal(got[k], b1[0][k][r].cpu().numpy().view(np.uint32)))
        for a in range(len(areas)):
            la = lid[a][np.asarray(roots)]
            exp = np.zeros_like(got["nh"][a])
            here = la >= 0
            if here.any():
                exp[here] = b1[1][a][torch.from_numpy(la[here]).cuda()].cpu().numpy().view(np.uint32)
            ok = ok and bool(np.array_equal(got["nh"][a], exp))
        log(f"parity of copy ({what}, {len(roots)} roots): {ok}")
        return ok

    def update(st, cap):
        sws = [a.sw for a in areas]
        try:
            ms, out = wall(lambda: st.update(sws, cap=cap, cap_rebased=4096, nh_words=Ws))
            return ms, out, cap
        except SelStateOverflow as e:  # the state is unchanged: once more with the counts
            cap = max(cap, e.n_changes)
            ms, out = wall(lambda: st.update(sws, cap=cap, cap_rebased=max(4096, e.n_rebased),
                                             nh_words=Ws))
            return ms, out, cap

    before, after = buffers(), buffers()
    ms_full = full_ms(before, t_pref)
    torch.cuda.synchronize()

    # ---- the state
    st = AreaSelState([a.sw for a in areas], gids, G, off, t_node, t_area, t_pref, t_mnh)
    sws = [a.sw for a in areas]
    prime_ms = [wall(lambda: st.prime(sws))[0] for _ in range(3)]
    device_bytes = st.device_bytes()
    log(f"prime {np.median(prime_ms):.1f} ms, device_bytes {device_bytes}")

    # the event: the first link of a rack in the middle of a0 (rack -- fabric switch)
    a0 = areas[0]
    csr = a0.csr
    racks = [i for i, nm in enumerate(a0.names) if nm.startswith("3-")]
    rack = racks[len(racks) // 3]
    e = int(csr["row_ptr"][rack])
    lo, hi = int(csr["metric"][e]), int(csr["metric"][csr["twin"][e]])
    if rack > int(csr["col"][e]):
        lo, hi = hi, lo
    lid_link = int(csr["link_id"][e])
    sample = sorted({int(gids[0][rack]), int(gids[0][int(csr["col"][e])]), 0, G - 1} |
                    {int(x) for x in np.random.default_rng(args.seed).integers(0, G, 60)})

    cap = 1 << 20
    events, ok = [], True
    for i, up in enumerate((0, 1, 0)):
        a0.ver += 1
        a0.eng.update_links([(lid_link, up, lo, hi)], version=a0.ver)
        a0.sweep()  # a1's sweep is reused
        ms, (rec, nh, reb), cap = update(st, cap)
        events.append(dict(event="down" if not up else "up", ms=ms, n_changes=int(len(rec)),
                           n_rebased=int(reb.size)))
        log(json.dumps(events[-1]))
    full(after, t_pref)
    torch.cuda.synchronize()
    ok_event = parity(rec, nh, reb.tolist(), before, after, "the link-down update")
    ok_copy = parity_copy(st, after, sample, "after the event")
    ms_full_after = full_ms(after, t_pref)

    # ---- the attributes alone: classes 0 and 1 swapped, the same sweeps
    st.set_policy(swapped, t_mnh)
    ms_attr, (rec, nh, reb), cap = update(st, cap)
    full(before, swapped)  # `before` now holds the selection under the new attributes
    torch.cuda.synchronize()
    ok_attr = parity(rec, nh, reb.tolist(), after, before, "the attribute-only update")
    ok_copy2 = parity_copy(st, before, sample, "after set_policy")
    attrs = dict(ms=ms_attr, n_changes=int(len(rec)), n_rebased=int(reb.size))

    upd = [x["ms"] for x in events]
    full_med = float(np.median(ms_full_after))
    ok = ok_event and ok_copy and ok_attr and ok_copy2
    summary = dict(G=G, P=P, entries=int(t_node.size), nh_words=Ws, device_bytes=int(device_bytes),
                   prime_ms=prime_ms, prime_ms_median=float(np.median(prime_ms)),
                   update_ms=upd, update_ms_median=float(np.median(upd)),
                   n_changes=events[-1]["n_changes"], n_rebased=events[-1]["n_rebased"],
                   full_ms_before=ms_full, full_ms=ms_full_after, full_ms_median=full_med,
                   update_over_full=float(np.median(upd)) / full_med, attrs_update=attrs,
                   attrs_over_full=ms_attr / full_med, cap=int(cap),
                   parity_event=ok_event, parity_copy=ok_copy and ok_copy2, parity_attrs=ok_attr,
                   parity=ok)
    print(json.dumps(summary), flush=True)
    out = dict(topology=f"fabric pods={args.pods} planes={args.planes} in two areas sharing the spines",
               device=torch.cuda.get_device_name(0), events=events, **summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    st.close()
    for a in areas:
        a.close()
    if not ok:
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
