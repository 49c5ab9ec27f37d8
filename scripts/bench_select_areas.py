#!/usr/bin/env python3
"""Route selection across several areas on the 100k-node fabric, one MI355X:
ospf_areas_select_policy_dev beside ospf_sweep_select_policy_dev.

The fabric is split into two areas that share the spines: area "a0" holds the
spines and the first half of the pods, area "a1" the spines and the rest. The
table is DESIGN.md section 6's multi-entry one carried over to (node, area)
entries: one anycast prefix per pod announced by four of its racks (in the
pod's area), a fabric-wide prefix announced by a rack in each of 64 pods (both
areas), and eight prefixes a spine announces into both areas; three classes,
thresholds 0..4. Timed with HIP events on one stream, each after one untimed
launch, median of --reps (>= 10), all in one process:

  (a) areas2   the areas call over both areas
  (b) floor    one ospf_sweep_select_policy_dev per area over that area's own
               entries; the sum is the work floor
  (c) areas1   the areas call with area a0 alone, beside (b)'s a0 launch on the
               same table: what the multi-area kernel costs at A = 1

and, on a small fabric of --host-pods pods split the same way (the host path
runs one SPF per node and area on the CPU, which F100k does not finish in a
benchmark's time), wall-clock:

  (d) linkstate_device / linkstate_host   all_areas_select_policy on the
               device (sweeps resident) and with set_host_spf

Parity: for the racks of a sample of pods, the per-pod prefixes of their own
area must agree between (a) and (b) in metric, count, links and need (a rack
is in one area, and those prefixes have entries in that area only); (d)'s two
answers must be equal. No pass threshold on the times.

Usage: python scripts/bench_select_areas.py [--out profiles/r11/select_areas_f100k.json]
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

from openr_amd import topology as T  # noqa: E402
from openr_amd.adjdb import AdjDbStream  # noqa: E402
from openr_amd.engine import Engine, Sweep, select_policy_areas_dev  # noqa: E402
from openr_amd.linkstate import LinkState, all_areas_select_policy  # noqa: E402

HDR = ("metric", "count", "links", "need", "best", "areas")
POL = ("metric", "count", "nh", "links", "need", "best")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def area_streams(pods, planes):
    """the two areas' streams: fabrics of pods // 2 and pods - pods // 2 pods,
    the second with its pods renumbered behind the first's (the spines keep
    their names: they are the border)"""
    h0 = pods // 2
    st0 = T.fabric(pods=h0, planes=planes)
    st1 = T.fabric(pods=pods - h0, planes=planes)

    def moved(s):
        f = s.split("-")
        return s if f[0] == "1" else f"{f[0]}-{int(f[1]) + h0}-{f[2]}"

    V1 = int(st1.cols["db_name"].size)
    strings = [moved(s) for s in st1.strings[:V1]] + list(st1.strings[V1:])
    return [st0, AdjDbStream(strings, st1.cols)]


def union(names):
    g = sorted({n for ns in names for n in ns}, key=lambda s: s.encode())
    ix = {n: i for i, n in enumerate(g)}
    return g, [np.array([ix[n] for n in ns], np.uint32) for ns in names]


def table_of(names, seed):
    """entries (node name, area) per prefix with class rank and threshold"""
    rng = np.random.default_rng(seed)
    racks = {}
    for a, ns in enumerate(names):
        for nm in ns:
            if nm.startswith("3-"):
                racks.setdefault((int(nm.split("-")[1]), a), []).append(nm)
    table = []
    for (d, a) in sorted(racks):
        pick = rng.choice(len(racks[d, a]), size=min(4, len(racks[d, a])), replace=False)
        table.append([(racks[d, a][int(i)], a) for i in pick])
    keys = sorted(racks)
    wide = rng.choice(len(keys), size=min(64, len(keys)), replace=False)
    table.append([(racks[keys[int(i)]][int(rng.integers(len(racks[keys[int(i)]])))], keys[int(i)][1])
                  for i in wide])
    spines = [nm for nm in names[0] if nm.startswith("1-")]
    for i in rng.choice(len(spines), size=min(8, len(spines)), replace=False):
        table.append([(spines[int(i)], 0), (spines[int(i)], 1)])
    return [[(nm, a, int(rng.integers(3)), int(rng.integers(5))) for nm, a in ents]
            for ents in table]


def csr_of(table, key):
    """entries sorted by key(entry) -> (offsets, sorted entry lists)"""
    rows = [sorted(ents, key=key) for ents in table]
    off = np.zeros(len(rows) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, rows


class Area:
    def __init__(self, name, stream_):
        t0 = time.time()
        ls = LinkState(area=name)
        ls.apply(stream_)
        self.names, csr = ls.node_names(), ls.csr()
        self.eng = Engine()
        self.eng.load(csr)
        self.sw = Sweep(self.eng)
        self.sw.run()
        self.eng.sync()
        self.W = max(1, self.sw.max_nh_words)
        self.pos = np.zeros(self.eng.V, np.int64)
        self.pos[self.sw.roots] = np.arange(self.sw.n_roots)
        log(f"area {name}: V={self.eng.V} mode={self.sw.mode} W={self.W} in {time.time() - t0:.1f}s")

    def close(self):
        self.sw.close()
        self.eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--host-pods", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "select_areas_f100k.json"))
    args = ap.parse_args()
    if args.reps < 10:
        raise SystemExit("--reps: at least 10 timed launches")
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_areas.py needs an MI355X: no HIP device")
    stream = torch.cuda.Stream()

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    records = []

    def record(case, fn, **kw):
        timed(fn, 1)  # the untimed launch (row table upload, code load)
        ms = timed(fn, args.reps)
        rec = dict(case=case, ms=ms, ms_median=float(np.median(ms)), ms_min=float(min(ms)),
                   ms_max=float(max(ms)), **kw)
        records.append(rec)
        print(json.dumps({k: v for k, v in rec.items() if k != "ms"}), flush=True)
        return rec

    # ---- F100k in two areas
    areas = [Area(f"a{i}", st) for i, st in enumerate(area_streams(args.pods, args.planes))]
    torch.cuda.synchronize()
    names = [a.names for a in areas]
    gnames, gids = union(names)
    gix = {n: i for i, n in enumerate(gnames)}
    lix = [{n: i for i, n in enumerate(ns)} for ns in names]
    G, table = len(gnames), table_of(names, args.seed)
    P = len(table)
    off, rows = csr_of(table, lambda e: (gix[e[0]], e[1]))
    col = lambda f: np.array([f(e) for r in rows for e in r], np.uint32)  # noqa: E731
    t_node, t_area = col(lambda e: gix[e[0]]), col(lambda e: e[1])
    t_pref, t_mnh = col(lambda e: e[2]), col(lambda e: e[3])
    E = int(t_node.size)
    log(f"union: G={G} P={P} entries={E}")
    new = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device="cuda")  # noqa: E731
    hdr = {k: new(G, P) for k in HDR}
    nh = [new(a.eng.V, P, a.W) for a in areas]
    sws, Ws = [a.sw for a in areas], [a.W for a in areas]

    def call_a():
        select_policy_areas_dev(sws, gids, G, off, t_node, t_area, t_pref, t_mnh, Ws,
                                **{f"d_{k}": hdr[k].data_ptr() for k in HDR},
                                d_nh=[x.data_ptr() for x in nh], stream=stream.cuda_stream)

    ra = record("a_areas2", call_a, n_roots=G, n_prefixes=P, n_entries=E, nh_words=Ws)

    # ---- (b): each area alone over its own entries, by the policy kernel
    floor, pol, own = [], [], []
    for ai, a in enumerate(areas):
        mine = [[e for e in ents if e[1] == ai] for ents in table]
        o, r = csr_of(mine, lambda e: lix[ai][e[0]])
        c = lambda f: np.array([f(e) for rr in r for e in rr], np.uint32)  # noqa: E731
        cols = (o, c(lambda e: lix[ai][e[0]]), c(lambda e: e[2]), c(lambda e: e[3]))
        bufs = {k: new(a.sw.n_roots, P, a.W) if k == "nh" else new(a.sw.n_roots, P) for k in POL}
        own.append((mine, cols))
        pol.append(bufs)

        def call_b(a=a, cols=cols, bufs=bufs):
            a.sw.select_policy_dev(*cols, a.W, stream=stream.cuda_stream,
                                   **{f"d_{k}": bufs[k].data_ptr() for k in POL})

        floor.append(record(f"b_policy_a{ai}", call_b, n_roots=a.sw.n_roots, n_prefixes=P,
                            n_entries=int(cols[1].size), nh_words=a.W))

    # parity of (a) against (b): racks of sampled pods, their own area's pod prefixes
    ok, cells = True, 0
    rng = np.random.default_rng(args.seed)
    for ai, a in enumerate(areas):
        pfx = [p for p, ents in enumerate(table[:-9]) if ents[0][1] == ai]
        pick = rng.choice(len(pfx), size=min(6, len(pfx)), replace=False)
        pods = {table[pfx[int(i)]][0][0].split("-")[1] for i in pick}
        loc = np.array([i for i, nm in enumerate(a.names)
                        if nm.startswith("3-") and nm.split("-")[1] in pods])
        gl = torch.from_numpy(gids[ai][loc].astype(np.int64)).cuda()
        sl = torch.from_numpy(a.pos[loc]).cuda()
        pc = torch.tensor(pfx, device="cuda")
        for k in ("metric", "count", "links", "need"):
            ok &= bool(torch.equal(hdr[k][gl][:, pc], pol[ai][k][sl][:, pc]))
        cells += loc.size * len(pfx)
    log(f"parity of {cells} cells against the per-area policy kernel: {ok}")

    # ---- (c): the areas call with area a0 alone, on (b)'s a0 table
    a0, (mine0, cols0) = areas[0], own[0]
    hdr1 = {k: new(a0.eng.V, P) for k in HDR}
    nh1 = new(a0.eng.V, P, a0.W)
    ident = np.arange(a0.eng.V, dtype=np.uint32)

    def call_c():
        select_policy_areas_dev([a0.sw], [ident], a0.eng.V, cols0[0], cols0[1],
                                np.zeros_like(cols0[1]), cols0[2], cols0[3], [a0.W],
                                **{f"d_{k}": hdr1[k].data_ptr() for k in HDR},
                                d_nh=[nh1.data_ptr()], stream=stream.cuda_stream)

    rc = record("c_areas1_a0", call_c, n_roots=a0.eng.V, n_prefixes=P,
                n_entries=int(cols0[1].size), nh_words=a0.W)
    torch.cuda.synchronize()
    inv = torch.from_numpy(a0.pos).cuda()
    ok1 = all(bool(torch.equal(hdr1[k], pol[0][k][inv])) for k in ("metric", "count", "links", "need"))
    ok1 &= bool(torch.equal(nh1, pol[0]["nh"][inv]))
    log(f"parity of A = 1 against the policy kernel (every root, metric/count/links/need/nh): {ok1}")
    for a in areas:
        a.close()
    del hdr, nh, pol, hdr1, nh1

    # ---- (d): the LinkState call, device and host path, on a small fabric
    sts = area_streams(args.host_pods, args.planes)
    small = {}
    answers = {}
    for mode in ("device", "host"):
        lss = []
        for i, st in enumerate(sts):
            ls = LinkState(area=f"a{i}")
            ls.set_host_spf(mode == "host")
            ls.apply(st)
            lss.append(ls)
        tb = table_of([ls.node_names() for ls in lss], args.seed)
        prefixes = {f"p{p}": [(nm, f"a{a}", 10 - r, 0, 0, mn or None) for nm, a, r, mn in ents]
                    for p, ents in enumerate(tb)}
        t0 = time.time()
        first = all_areas_select_policy(lss, prefixes)
        t1 = time.time()
        again = all_areas_select_policy(lss, prefixes)
        t2 = time.time()
        assert first["on_device"] == (mode == "device")
        answers[mode] = again
        small[mode] = dict(first_ms=(t1 - t0) * 1e3, again_ms=(t2 - t1) * 1e3,
                           nodes=len(first["names"]), n_prefixes=len(tb))
        print(json.dumps(dict(case=f"d_linkstate_{mode}", **small[mode])), flush=True)
    okd = all(np.array_equal(answers["device"][k], answers["host"][k]) for k in HDR)
    okd &= all(np.array_equal(x, y) for x, y in zip(answers["device"]["nh"], answers["host"]["nh"]))
    log(f"parity of the LinkState call, device against host path: {okd}")

    fl = sum(r["ms_median"] for r in floor)
    summary = dict(areas2_ms=ra["ms_median"], floor_ms=fl, areas2_over_floor=ra["ms_median"] / fl,
                   areas1_ms=rc["ms_median"], policy_a0_ms=floor[0]["ms_median"],
                   areas1_over_policy=rc["ms_median"] / floor[0]["ms_median"],
                   linkstate_small=small, parity_areas2=ok, parity_areas1=ok1, parity_linkstate=okd)
    print(json.dumps(summary), flush=True)
    out = dict(topology=f"fabric pods={args.pods} planes={args.planes} in two areas sharing the spines",
               G=G, device=torch.cuda.get_device_name(0), cases=records, summary=summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not (ok and ok1 and okd):
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
