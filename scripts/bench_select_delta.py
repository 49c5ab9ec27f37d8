#!/usr/bin/env python3
"""The selection delta after one link event on the 100k-node fabric, one MI355X.

F100k all-sources sweep, then for the three tables of scripts/bench_select.py
((a) spines, (b) pods, (c) loopbacks): SelState.prime, one rack--fabric link
taken down with ospf_update_links, a new sweep, and SelState.update -- the
entries of the route DB that changed, selected and compared on the device.
Timed with HIP events around the (synchronous) calls, the median of --reps:
the first update after the event carries the changes; the repeats on the same
sweep report none and do the same device work (the kernel always selects,
stores and compares every entry). The baseline beside it is the full
ospf_sweep_select_dev of the same table in the same process.

Parity: two full selects (before / after the event) of 64 seeded roots,
diffed in numpy, against the records update returned for those roots.

Usage: python scripts/bench_select_delta.py [--out profiles/r07/select_delta_f100k.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_select import csr_table, log, tables  # noqa: E402
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import Engine, SelState, Sweep  # noqa: E402
from openr_amd.linkstate import LinkState  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parity-roots", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "select_delta_f100k.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_delta.py needs an MI355X: no HIP device")

    t0 = time.time()
    ls = LinkState()
    ls.apply(T.fabric(pods=args.pods, planes=args.planes))
    names, csr = ls.node_names(), ls.csr()
    V = len(names)
    log(f"graph: V={V} E={csr['col'].size} in {time.time() - t0:.1f}s")
    # the event: the first link of a rack in the middle (rack -- fabric switch)
    rack = [i for i, nm in enumerate(names) if nm.startswith("3-")][V // 3]
    e = int(csr["row_ptr"][rack])
    link = (int(csr["link_id"][e]), 0, int(csr["metric"][e]), int(csr["metric"][csr["twin"][e]]))
    if rack > int(csr["col"][e]):
        link = (link[0], 0, link[3], link[2])
    log(f"event: link {link[0]} {names[rack]} -- {names[int(csr['col'][e])]} down")

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = ev(), ev()
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    rng = np.random.default_rng(args.seed)
    parity_roots = np.sort(rng.choice(V, size=min(args.parity_roots, V), replace=False))
    records = []
    for tname, table in tables(names, args.seed).items():
        off, nodes = csr_table(table)
        P = len(table)
        eng = Engine()
        eng.load(csr, version=1)
        sw = Sweep(eng, hip_graph=False)
        sw.run()
        eng.sync()
        Wout, n = sw.max_nh_words, sw.n_roots
        pos = np.zeros(V, np.int64)
        pos[sw.roots] = np.arange(n)

        def full_select(sweep, keep):
            """the full select, timed; -> (ms, the parity roots' rows by node id)"""
            d_m = torch.empty((n, P), dtype=torch.int32, device="cuda")
            d_c = torch.empty((n, P), dtype=torch.int32, device="cuda")
            d_nh = torch.empty((n, P, Wout), dtype=torch.int32, device="cuda")
            p2 = np.zeros(V, np.int64)
            p2[sweep.roots] = np.arange(n)

            def call():
                sweep.select_dev(off, nodes, Wout, d_metric=d_m.data_ptr(), d_count=d_c.data_ptr(),
                                 d_nh=d_nh.data_ptr())
                torch.cuda.synchronize()

            timed(call, 1)
            ms = timed(call, args.reps)
            idx = torch.from_numpy(p2[keep]).cuda()
            rows = [t[idx].cpu().numpy().view(np.uint32) for t in (d_m, d_c, d_nh)]
            del d_m, d_c, d_nh
            torch.cuda.empty_cache()
            return ms, rows

        select_ms, before = full_select(sw, parity_roots)
        st = SelState(eng, off, nodes)
        prime_ms = timed(lambda: st.prime(sw), 1 + args.reps)[1:]
        state_bytes = st.device_bytes
        sw.close()
        eng.update_links([link], version=2)
        sw = Sweep(eng, hip_graph=False)
        sw.run()
        eng.sync()
        got = {}

        def first():
            cap = 1 << 16
            while True:
                try:
                    got["r"] = st.update(sw, cap=cap, cap_rebased=64, nh_words=Wout)
                    return
                except Exception as ex:  # SelStateOverflow: the complete counts, retry
                    if getattr(ex, "code", 0) != -4:
                        raise
                    cap = max(cap * 2, ex.n_changes)

        first_ms = timed(first, 1)[0]
        rec, nh, reb = got["r"]
        repeat_ms = timed(lambda: st.update(sw, cap=16, cap_rebased=16, nh_words=Wout), args.reps)
        _, after = full_select(sw, parity_roots)
        # parity on the seeded roots: numpy diff of the two full selects
        mask = (before[0] != after[0]) | (before[1] != after[1]) | (before[2] != after[2]).any(axis=2)
        want = {(int(parity_roots[i]), int(p)): (int(after[0][i, p]), int(after[1][i, p]),
                                                 tuple(after[2][i, p].tolist()))
                for i, p in np.argwhere(mask)}
        keep = set(parity_roots.tolist())
        have = {(int(r["root"]), int(r["prefix"])): (int(r["metric"]), int(r["count"]),
                                                     tuple(nh[i].tolist()))
                for i, r in enumerate(rec) if int(r["root"]) in keep}
        out = dict(table=tname, n_roots=n, n_prefixes=P, n_announcers=int(nodes.size), nh_words=Wout,
                   full_select_ms=select_ms, full_select_ms_median=float(np.median(select_ms)),
                   prime_ms=prime_ms, prime_ms_median=float(np.median(prime_ms)),
                   update_first_ms=first_ms, update_repeat_ms=repeat_ms,
                   update_ms_median=float(np.median(repeat_ms)),
                   n_changes=int(len(rec)), n_rebased=int(len(reb)),
                   change_bytes=int(len(rec) * (16 + 4 * Wout) + 4 * len(reb)),
                   full_select_bytes=int(n * P * 4 * (2 + Wout)), state_device_bytes=int(state_bytes),
                   update_over_full_select=float(np.median(repeat_ms) / np.median(select_ms)),
                   parity_roots=int(parity_roots.size), parity_changed=len(want),
                   parity_ok=bool(have == want))
        records.append(out)
        print(json.dumps(out), flush=True)
        st.close()
        sw.close()
        eng.close()
    res = dict(topology=f"fabric pods={args.pods} planes={args.planes}", V=V,
               device=torch.cuda.get_device_name(0), event="one rack--fabric link down",
               tables=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if not all(r["parity_ok"] for r in records):
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
