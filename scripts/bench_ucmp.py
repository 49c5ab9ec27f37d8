#!/usr/bin/env python3
"""UCMP weights of every root and prefix on the 100k-node fabric, one MI355X.

The table: one weighted anycast prefix per pod (announced by four of the pod's
racks, weights 1..8, seeded) plus a fabric-wide one (one rack in each of 64
pods). LinkState.track_select keeps the selection resident; then

  device   LinkState.all_sources_ucmp(weights, algo): the S sums on the host,
           ospf_selstate_ucmp (timed alone too: engine_ms), and the [V, P]
           advertised weights and statuses copied back;
  host     LinkState.ucmp_host_loop on a seeded sample of roots --
           resolveUcmpWeights(getSpfResult(root), min-cost announcers) per root
           and prefix, the loop the call replaces (and degrades to) -- scaled
           to all V roots.

The sample's host answers are compared with the device's (ucmp_tracked). One
JSON record per algorithm on stdout; --out keeps them in a file.

Usage: python scripts/bench_ucmp.py [--out profiles/r08/ucmp_f100k.json]
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
from openr_amd.linkstate import LinkState  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def table(names, seed):
    """-> ({prefix: announcer names}, {prefix: weights}) from topology.fabric's
    names (racks 3-pod-i)."""
    rng = np.random.default_rng(seed)
    racks = {}
    for nm in names:
        if nm.startswith("3-"):
            racks.setdefault(int(nm.split("-")[1]), []).append(nm)
    prefixes, weights = {}, {}
    for pod in sorted(racks):
        ann = sorted(rng.choice(racks[pod], size=min(4, len(racks[pod])), replace=False).tolist())
        prefixes[f"pod{pod}"] = ann
        weights[f"pod{pod}"] = rng.integers(1, 9, size=len(ann)).tolist()
    pods = sorted(rng.choice(sorted(racks), size=min(64, len(racks)), replace=False).tolist())
    wide = [racks[d][int(rng.integers(len(racks[d])))] for d in pods]
    prefixes["fabric"] = wide
    weights["fabric"] = rng.integers(1, 9, size=len(wide)).tolist()
    return prefixes, weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sample", type=int, default=8, help="roots of the host loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "ucmp_f100k.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ucmp.py needs an MI355X: no HIP device")

    t0 = time.time()
    ls = LinkState()
    ls.apply(T.fabric(pods=args.pods, planes=args.planes))
    names = ls.node_names()
    V = len(names)
    prefixes, weights = table(names, args.seed)
    P = len(prefixes)
    log(f"graph: V={V} P={P} in {time.time() - t0:.1f}s")
    t0 = time.time()
    ls.track_select(prefixes)
    track_s = time.time() - t0
    log(f"track_select (sweep + selection): {track_s:.1f}s")

    rng = np.random.default_rng(args.seed)
    kinds = {k: [nm for nm in names if nm.startswith(k + "-")] for k in "123"}
    sample = [kinds["1"][0], kinds["2"][len(kinds["2"]) // 2]]
    sample += rng.choice(kinds["3"], size=max(0, args.sample - 2), replace=False).tolist()

    records = []
    for algo in ("prefix", "adj"):
        call_ms, engine_ms = [], []
        for _ in range(args.reps + 1):  # the first call allocates: not counted
            t1 = time.time()
            weight, status = ls.all_sources_ucmp(weights, algo)
            call_ms.append((time.time() - t1) * 1e3)
            engine_ms.append(ls.ucmp_info["engine_ms"])
            assert ls.ucmp_info["device"]
        rounds = ls.ucmp_info["rounds"]
        dev = ls.ucmp_tracked(sample)
        t1 = time.time()
        host = ls.ucmp_host_loop(weights, algo, sample)
        host_s = time.time() - t1
        ok = all(np.array_equal(a, b) for a, b in zip(dev, host))
        ids = [names.index(nm) for nm in sample]
        ok = ok and np.array_equal(weight[ids], dev[0]) and np.array_equal(status[ids], dev[1])
        rec = dict(algo=algo, V=V, n_prefixes=P, rounds=rounds,
                   device_engine_ms=engine_ms[1:], device_engine_ms_median=float(np.median(engine_ms[1:])),
                   device_call_ms=call_ms[1:], device_call_ms_median=float(np.median(call_ms[1:])),
                   status_counts=np.bincount(status.ravel(), minlength=4).tolist(),
                   host_loop_roots=len(sample), host_loop_s=host_s,
                   host_loop_ms_per_root=host_s * 1e3 / len(sample),
                   host_loop_all_roots_s=host_s * V / len(sample),
                   host_over_device_call=host_s * V / len(sample) * 1e3 / float(np.median(call_ms[1:])),
                   sample_parity_ok=bool(ok))
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del weight, status
    out = dict(topology=f"fabric pods={args.pods} planes={args.planes}", V=V,
               device=torch.cuda.get_device_name(0), track_select_s=track_s, sample=sample,
               algos=records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not all(r["sample_parity_ok"] for r in records):
        raise SystemExit("parity mismatch between the device and the host loop")


if __name__ == "__main__":
    main()
