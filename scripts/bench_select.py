#!/usr/bin/env python3
"""Device-side anycast route selection on the 100k-node fabric, one MI355X.

One all-sources sweep (every root's dist and next-hop rows resident on the
device), then ospf_sweep_select_dev -- SpfSolver::getNextHopsWithMetric
(SpfSolver.cpp:1043-1089) for every root and every prefix of a table -- timed
with HIP events for three tables:

  (a) spines     one prefix announced by all 288 spines
  (b) pods       one aggregate per pod announced by the pod's 8 fabric switches
  (c) loopbacks  1,024 single-announcer prefixes + 64 prefixes of 16 random
                 racks (seeded)

Per table one JSON record: ms per select (table upload included), the useful
bytes (per root A * 4 * (1 + W_root) gathered + the outputs written) and the
rate they give, the same sweep's run time beside it, the parity of 64 seeded
roots against a numpy evaluation of Sweep.rows(), and the copy route for
comparison: Sweep.rows() + the numpy evaluation for 256 roots, scaled to all.

Usage: python scripts/bench_select.py [--out profiles/r07/select_f100k.json]
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
from openr_amd.engine import Engine, Sweep  # noqa: E402
from openr_amd.linkstate import LinkState  # noqa: E402

INF = 0xFFFFFFFF


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def tables(names, seed):
    """{name: list of announcer id lists} from topology.fabric's names
    (spines 1-plane-i, fabric switches 2-pod-plane, racks 3-pod-i)."""
    rng = np.random.default_rng(seed)
    spines = [i for i, nm in enumerate(names) if nm.startswith("1-")]
    racks = np.array([i for i, nm in enumerate(names) if nm.startswith("3-")])
    pods = {}
    for i, nm in enumerate(names):
        if nm.startswith("2-"):
            pods.setdefault(int(nm.split("-")[1]), []).append(i)
    loop = [[int(v)] for v in rng.choice(len(names), size=min(1024, len(names)), replace=False)]
    anyc = [sorted(rng.choice(racks, size=min(16, racks.size), replace=False).tolist())
            for _ in range(64)]
    return {"spines": [spines], "pods": [sorted(pods[d]) for d in sorted(pods)],
            "loopbacks": loop + anyc}


def csr_table(table):
    off = np.zeros(len(table) + 1, np.uint32)
    off[1:] = np.cumsum([len(a) for a in table])
    return off, np.array([x for a in table for x in a], np.uint32)


def numpy_select(dist, nh, table):
    """The reference loop over host rows: dist [n, V], nh [n, V, W] ->
    metric [n, P], count [n, P], nh [n, P, W]."""
    n, W = dist.shape[0], nh.shape[2]
    metric = np.full((n, len(table)), INF, np.uint32)
    count = np.zeros((n, len(table)), np.uint32)
    out = np.zeros((n, len(table), W), np.uint32)
    for p, ann in enumerate(table):
        if not ann:
            continue
        d = dist[:, ann]
        m = d.min(axis=1)
        tight = (d == m[:, None]) & (m != INF)[:, None]
        metric[:, p] = m
        count[:, p] = tight.sum(axis=1)
        out[:, p, :] = np.bitwise_or.reduce(np.where(tight[:, :, None], nh[:, ann, :], 0), axis=1)
    return metric, count, out


def rows_by_width(sw, eng_words, roots):
    """Sweep.rows() per width class (no padding copied) -> {W: (roots, dist, nh)}"""
    out = {}
    for W in sorted(set(eng_words[roots].tolist())):
        grp = roots[eng_words[roots] == W]
        dist, nh = sw.rows(grp, W)
        out[W] = (grp, dist, nh)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parity-roots", type=int, default=64)
    ap.add_argument("--copy-roots", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "select_f100k.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select.py needs an MI355X: no HIP device")

    t0 = time.time()
    ls = LinkState()
    ls.apply(T.fabric(pods=args.pods, planes=args.planes))
    names, csr = ls.node_names(), ls.csr()
    eng = Engine()
    eng.load(csr)
    V = eng.V
    deg = np.array([np.unique(csr["col"][csr["row_ptr"][r]:csr["row_ptr"][r + 1]]).size
                    for r in range(V)])
    words = np.maximum(1, (deg + 31) // 32).astype(np.int64)
    log(f"graph: V={V} E={csr['col'].size} in {time.time() - t0:.1f}s")

    sw = Sweep(eng)
    stream = torch.cuda.Stream()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = ev(), ev()
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    sw.run(stream.cuda_stream)
    eng.sync(stream.cuda_stream)
    sweep_ms = timed(lambda: sw.run(stream.cuda_stream), 3)
    eng.sync(stream.cuda_stream)
    torch.cuda.synchronize()
    Wout = sw.max_nh_words
    n = sw.n_roots
    pos = np.zeros(V, np.int64)
    pos[sw.roots] = np.arange(n)
    w_root = words[sw.roots]
    log(f"sweep: mode={sw.mode} n_roots={n} max_nh_words={Wout} run ms={sweep_ms}")

    rng = np.random.default_rng(args.seed)
    parity_roots = np.sort(rng.choice(V, size=min(args.parity_roots, V), replace=False)).astype(np.uint32)
    copy_roots = np.sort(rng.choice(V, size=min(args.copy_roots, V), replace=False)).astype(np.uint32)
    parity_rows = rows_by_width(sw, words, parity_roots)
    t1 = time.time()
    copy_rows = rows_by_width(sw, words, copy_roots)
    copy_rows_s = time.time() - t1

    records = []
    for tname, table in tables(names, args.seed).items():
        off, nodes = csr_table(table)
        P, A = len(table), int(nodes.size)
        d_m = torch.empty((n, P), dtype=torch.int32, device="cuda")
        d_c = torch.empty((n, P), dtype=torch.int32, device="cuda")
        d_nh = torch.empty((n, P, Wout), dtype=torch.int32, device="cuda")

        def call():
            sw.select_dev(off, nodes, Wout, d_metric=d_m.data_ptr(), d_count=d_c.data_ptr(),
                          d_nh=d_nh.data_ptr(), stream=stream.cuda_stream)

        timed(call, 1)  # warm-up (the row table's upload, code load)
        ms = timed(call, args.reps)
        read_b = int((A * 4 * (1 + w_root)).sum())
        write_b = n * P * 4 * (2 + Wout)
        best = float(np.median(ms))
        # parity: 64 seeded roots against numpy over Sweep.rows()
        ok, checked = True, 0
        for W, (grp, dist, nh) in parity_rows.items():
            em, ec, en = numpy_select(dist, nh, table)
            idx = torch.from_numpy(pos[grp]).cuda()
            gm = d_m[idx].cpu().numpy().view(np.uint32)
            gc = d_c[idx].cpu().numpy().view(np.uint32)
            gn = d_nh[idx].cpu().numpy().view(np.uint32)
            ok &= bool(np.array_equal(gm, em) and np.array_equal(gc, ec) and
                       np.array_equal(gn[:, :, :W], en) and not gn[:, :, W:].any())
            checked += grp.size
        # the copy route: rows to the host (timed above, once) + numpy per table
        t2 = time.time()
        for W, (grp, dist, nh) in copy_rows.items():
            numpy_select(dist, nh, table)
        copy_s = copy_rows_s + (time.time() - t2)
        copy_all_ms = copy_s * 1e3 * V / copy_roots.size
        rec = dict(table=tname, n_roots=n, n_prefixes=P, n_announcers=A, nh_words=Wout,
                   select_ms=ms, select_ms_median=best,
                   useful_bytes_read=read_b, useful_bytes_written=write_b,
                   useful_gb_per_s=(read_b + write_b) / best / 1e6,
                   sweep_run_ms=sweep_ms, select_over_sweep_run=best / float(np.median(sweep_ms)),
                   parity_roots=int(checked), parity_ok=ok,
                   copy_route_roots=int(copy_roots.size), copy_route_rows_s=copy_rows_s,
                   copy_route_s=copy_s, copy_route_all_roots_ms=copy_all_ms,
                   copy_route_over_select=copy_all_ms / best)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del d_m, d_c, d_nh
        torch.cuda.empty_cache()
    sw.close()
    eng.close()
    out = dict(topology=f"fabric pods={args.pods} planes={args.planes}", V=V, sweep_mode=sw.mode,
               device=torch.cuda.get_device_name(0), tables=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not all(r["parity_ok"] for r in records):
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
