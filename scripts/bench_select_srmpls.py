#!/usr/bin/env python3
"""SR_MPLS route selection over the all-sources sweep of the F100k fabric on one
MI355X: ospf_sweep_select_srmpls_dev beside ospf_sweep_select_policy_dev.

The anycast table of scripts/bench_select_policy.py (four racks per pod, then
one rack in each of 64 pods), three classes, thresholds, every second entry
with a prepend label, on the plain fabric's derive sweep. Timed in one process,
on one stream, >= 10 launches each after an untimed one:

  policy      ospf_sweep_select_policy_dev, all six outputs (the IP route)
  srmpls      ospf_sweep_select_srmpls_dev without dst_nh (six outputs)
  srmpls_nh   the same with dst_nh [n][A][W] -- the dense per-destination words,
              the expected cost (n x A x W x 4 bytes; skipped with the reason
              when the device cannot hold it)

and the ratios srmpls / policy, srmpls_nh / policy. Parity: a sample of roots
against tests/srmpls_ref.py (every output but the dense dst_nh).

Usage: python scripts/bench_select_srmpls.py [--out profiles/select_srmpls_f100k.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import selpolicy_ref as PR  # noqa: E402
import srmpls_ref as SR  # noqa: E402
from bench_select_policy import Rig, csr_table, log, table_of  # noqa: E402
from openr_amd import topology as T  # noqa: E402
from oracle import Oracle, parse_spf_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_srmpls_f100k.json"))
    args = ap.parse_args()
    if args.reps < 10:
        raise SystemExit("--reps: at least 10 timed launches")
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_srmpls.py needs an MI355X: no HIP device")

    rig = Rig(T.fabric(pods=args.pods, planes=args.planes))
    stream = torch.cuda.Stream()
    table = table_of(rig.names, args.seed)
    off, nodes = csr_table(table)
    n, P, W, A = rig.n, len(table), rig.W, int(nodes.size)
    rng = np.random.default_rng(args.seed + 1)
    pref, mnh = PR.random_policy(table, rng, classes=3, max_need=4)
    flags = [[(i + p) & 1 for i in range(len(a))] for p, a in enumerate(table)]
    cols = (off, nodes, PR.flat(pref), PR.flat(mnh))

    def timed(fn):
        fn()  # the untimed launch (row table upload, code load)
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    def dev(shape):
        return torch.full(shape, -1, dtype=torch.int32, device="cuda")

    pol = {k: dev((n, P, W) if k == "nh" else (n, P)) for k in PR.KEYS}
    sr = {k: dev((n, A) if k == "dst_links" else (n, P)) for k in SR.KEYS if k != "dst_nh"}
    records = []

    def record(name, ms, **extra):
        rec = dict(case=name, n_roots=n, n_prefixes=P, n_announcers=A, nh_words=W, ms=ms,
                   ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)),
                   **extra)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    r_pol = record("policy", timed(lambda: rig.sw.select_policy_dev(
        *cols, W, stream=stream.cuda_stream, **{f"d_{k}": t.data_ptr() for k, t in pol.items()})))
    pol = None  # its nh is n x P x W words: the room dst_nh needs
    torch.cuda.empty_cache()
    ptr = {f"d_{k}": t.data_ptr() for k, t in sr.items()}
    r_sr = record("srmpls", timed(lambda: rig.sw.select_srmpls_dev(
        *cols, SR.flat(flags), W, stream=stream.cuda_stream, **ptr)))
    nh_bytes = n * A * W * 4
    r_nh, skipped = None, None
    try:
        sr["dst_nh"] = torch.empty((n, A, W), dtype=torch.int32, device="cuda")
    except RuntimeError as e:  # the device cannot hold the dense words
        skipped = f"dst_nh of {nh_bytes / 1e9:.1f} GB not allocated: {str(e).splitlines()[0]}"
        log(skipped)
    else:
        ptr["d_dst_nh"] = sr["dst_nh"].data_ptr()
        ms = timed(lambda: rig.sw.select_srmpls_dev(
            *cols, SR.flat(flags), W, stream=stream.cuda_stream, **ptr))
        r_nh = record("srmpls_nh", ms, dst_nh_bytes=nh_bytes,
                      dst_nh_gb_per_s=nh_bytes / float(np.median(ms)) / 1e6)

    # parity of a sample of roots against the restatement
    t0 = time.time()
    prng = np.random.default_rng(args.seed)
    kinds = {k: [i for i, nm in enumerate(rig.names) if nm.startswith(k + "-")] for k in "123"}
    roots = sorted([kinds["1"][0], kinds["2"][len(kinds["2"]) // 2]] +
                   prng.choice(kinds["3"], size=max(0, args.sample - 2), replace=False).tolist() +
                   [int(nodes[0]), int(nodes[-1])])  # two announcing roots
    orc = Oracle(rig.st)
    spf = {rig.names[r]: parse_spf_text(orc.spf_text(rig.names[r], True)) for r in roots}
    want, facts = SR.expect(spf, rig.names, rig.csr, table, pref, mnh, flags, W, roots=roots,
                            with_nh=False)
    idx = torch.from_numpy(rig.pos[roots]).cuda()
    ok = True
    checked = [k for k in sr if k != "dst_nh"]  # the dense words are the GPU tests' to check
    for k in checked:
        t = sr[k]
        ok &= bool(np.array_equal(t[idx].cpu().numpy().view(np.uint32), want[k][roots]))
    log(f"parity of {len(roots)} roots: {ok} in {time.time() - t0:.1f}s; facts {facts}")

    summary = dict(srmpls_over_policy=r_sr["ms_median"] / r_pol["ms_median"],
                   srmpls_nh_over_policy=r_nh["ms_median"] / r_pol["ms_median"] if r_nh else None,
                   dst_nh_bytes=nh_bytes, dst_nh_skipped=skipped, parity_roots=len(roots),
                   parity_ok=ok, parity_outputs=sorted(checked))
    print(json.dumps(summary), flush=True)
    out = dict(topology=f"fabric pods={args.pods} planes={args.planes}", V=rig.eng.V,
               device=torch.cuda.get_device_name(0), cases=records, summary=summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    rig.close()
    if not ok:
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
