#!/usr/bin/env python3
"""Route selection under the best-route policy on the 100k-node fabric, one
MI355X: ospf_sweep_select_policy_dev beside ospf_sweep_select_dev.

The table is DESIGN.md section 6's 1,782-prefix one (one anycast prefix per pod
announced by four of its racks, plus a fabric-wide one announced by a rack in
each of 64 pods, seeded). Three launches are timed with HIP events on one
stream, each after one untimed launch, median of --reps (>= 10):

  (a) plain     ospf_sweep_select_dev: the yardstick
  (b) uniform   the policy kernel, every pref 0, no threshold, nothing drained
  (c) policy    the policy kernel, three classes, thresholds 0..4 and 5 % of
                the announcers drained (their own graph and sweep: the drained
                bit is the graph's)

The byte ratio printed beside the time ratio is computed from the table: (b)
reads what (a) gathers plus 4 B of pref per announcer and root and the root's
CSR row once (colx, w, didx: 10 B per entry), and writes three more words per
(root, prefix); (c) also reads 4 B of min_nexthop per announcer and root.
Parity: a sample of roots (a spine, a fabric switch, racks) against the four
steps restated over the CPU oracle's SPF (tests/selpolicy_ref.py), for all
three. The box's store-probe rate is recorded with them.

Usage: python scripts/bench_select_policy.py [--out profiles/r09/select_policy_f100k.json]
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

import selpolicy_ref as PR  # noqa: E402
from openr_amd import topology as T  # noqa: E402
from openr_amd.adjdb import AdjDbStream  # noqa: E402
from openr_amd.engine import Engine, Sweep  # noqa: E402
from openr_amd.linkstate import LinkState  # noqa: E402
from oracle import Oracle, parse_spf_text  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def table_of(names, seed):
    """announcer id lists: four racks per pod, then one rack in each of 64 pods"""
    rng = np.random.default_rng(seed)
    racks = {}
    for i, nm in enumerate(names):
        if nm.startswith("3-"):
            racks.setdefault(int(nm.split("-")[1]), []).append(i)
    table = [sorted(rng.choice(racks[d], size=min(4, len(racks[d])), replace=False).tolist())
             for d in sorted(racks)]
    pods = sorted(rng.choice(sorted(racks), size=min(64, len(racks)), replace=False).tolist())
    table.append(sorted(racks[d][int(rng.integers(len(racks[d])))] for d in pods))
    return table


def csr_table(table):
    off = np.zeros(len(table) + 1, np.uint32)
    off[1:] = np.cumsum([len(a) for a in table])
    return off, np.array([x for a in table for x in a], np.uint32)


class Rig:
    """one graph: LinkState (names, CSR), oracle, engine, sweep"""

    def __init__(self, stream_):
        t0 = time.time()
        self.st = stream_
        ls = LinkState()
        ls.apply(stream_)
        self.names, self.csr = ls.node_names(), ls.csr()
        self.eng = Engine()
        self.eng.load(self.csr)
        self.sw = Sweep(self.eng)
        self.sw.run()
        self.eng.sync()
        torch.cuda.synchronize()
        self.n, self.W = self.sw.n_roots, self.sw.max_nh_words
        self.pos = np.zeros(self.eng.V, np.int64)
        self.pos[self.sw.roots] = np.arange(self.n)
        log(f"graph + sweep: V={self.eng.V} mode={self.sw.mode} Wout={self.W} in {time.time() - t0:.1f}s")

    def close(self):
        self.sw.close()
        self.eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1781)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "select_policy_f100k.json"))
    args = ap.parse_args()
    if args.reps < 10:
        raise SystemExit("--reps: at least 10 timed launches")
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_policy.py needs an MI355X: no HIP device")

    plain_st = T.fabric(pods=args.pods, planes=args.planes)
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

    def sample_of(names):
        rng = np.random.default_rng(args.seed)
        kinds = {k: [i for i, nm in enumerate(names) if nm.startswith(k + "-")] for k in "123"}
        s = [kinds["1"][0], kinds["2"][len(kinds["2"]) // 2]]
        s += rng.choice(kinds["3"], size=max(0, args.sample - 2), replace=False).tolist()
        return sorted(int(x) for x in s)

    def parity(rig, bufs, table, pref, mnh, keys):
        """the sampled roots' device rows against the restatement"""
        t0 = time.time()
        roots = sample_of(rig.names)
        orc = Oracle(rig.st)
        spf = {rig.names[r]: parse_spf_text(orc.spf_text(rig.names[r], True)) for r in roots}
        want, _ = PR.expect(spf, rig.names, rig.csr, table, pref, mnh, rig.W, roots=roots)
        ok = True
        idx = torch.from_numpy(rig.pos[roots]).cuda()
        for k in keys:
            got = bufs[k][idx].cpu().numpy().view(np.uint32)
            ok &= bool(np.array_equal(got, want[k][roots]))
        log(f"parity of {len(roots)} roots: {ok} in {time.time() - t0:.1f}s")
        return ok, len(roots)

    records = []

    def record(name, rig, call, bufs, table, pref, mnh, keys, bytes_):
        timed(call, 1)  # the untimed launch (row table upload, code load)
        ms = timed(call, args.reps)
        ok, checked = parity(rig, bufs, table, pref, mnh, keys)
        rec = dict(case=name, n_roots=rig.n, n_prefixes=len(table),
                   n_announcers=int(sum(len(a) for a in table)), nh_words=rig.W, ms=ms,
                   ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)),
                   bytes=int(bytes_), gb_per_s=bytes_ / float(np.median(ms)) / 1e6,
                   parity_roots=checked, parity_ok=ok)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    # ---- (a), (b): the plain fabric
    rig = Rig(plain_st)
    table = table_of(rig.names, args.seed)
    off, nodes = csr_table(table)
    n, P, Wout, A = rig.n, len(table), rig.W, int(nodes.size)
    deg = np.diff(rig.csr["row_ptr"]).astype(np.int64)
    dn = np.array([np.unique(rig.csr["col"][rig.csr["row_ptr"][r]:rig.csr["row_ptr"][r + 1]]).size
                   for r in range(rig.eng.V)])
    w_root = np.maximum(1, (dn + 31) // 32)[rig.sw.roots]
    bytes_a = int((A * 4 * (1 + w_root)).sum()) + n * P * 4 * (2 + Wout)
    bytes_b = bytes_a + n * A * 4 + int(deg[rig.sw.roots].sum()) * 10 + n * P * 4 * 3
    bytes_c = bytes_b + n * A * 4
    probe = rig.eng.probe_store("stream", 1 << 20, 1024, reps=5)
    probe_gbs = 2 * 1024 * (1 << 20) * 4 / float(np.median(probe)) / 1e6
    log(f"store probe: {probe_gbs:.0f} GB/s")
    bufs = {k: torch.empty((n, P, Wout) if k == "nh" else (n, P), dtype=torch.int32, device="cuda")
            for k in PR.KEYS}
    ptr = {f"d_{k}": bufs[k].data_ptr() for k in PR.KEYS}
    upref, umnh = PR.uniform_policy(table)

    def call_a():
        rig.sw.select_dev(off, nodes, Wout, d_metric=ptr["d_metric"], d_count=ptr["d_count"],
                          d_nh=ptr["d_nh"], stream=stream.cuda_stream)

    def call_b():
        rig.sw.select_policy_dev(off, nodes, PR.flat(upref), None, Wout, stream=stream.cuda_stream,
                                 **ptr)

    for t in bufs.values():
        t.fill_(-1)
    ra = record("a_plain", rig, call_a, bufs, table, upref, umnh, ("metric", "count", "nh"), bytes_a)
    for t in bufs.values():
        t.fill_(-1)
    rb = record("b_uniform", rig, call_b, bufs, table, upref, umnh, PR.KEYS, bytes_b)
    rig.close()
    del rig

    # ---- (c): 5 % of the announcers drained, three classes, thresholds
    rng = np.random.default_rng(args.seed + 1)
    ann = np.unique(nodes)
    drained = rng.choice(ann, size=max(1, ann.size // 20), replace=False)
    cols = dict(plain_st.cols)
    ov = cols["db_overloaded"].copy()
    by_name = {plain_st.strings[s]: i for i, s in enumerate(cols["db_name"])}
    names0 = sorted(by_name)  # node ids are name ranks
    for v in drained.tolist():
        ov[by_name[names0[v]]] = 1
    cols["db_overloaded"] = ov
    rig = Rig(AdjDbStream(plain_st.strings, cols))
    assert rig.names == names0 and int(np.asarray(rig.csr["no_transit"]).sum()) == drained.size
    assert rig.n == n and rig.W == Wout
    pref, mnh = PR.random_policy(table, rng, classes=3, max_need=4)

    def call_c():
        rig.sw.select_policy_dev(off, nodes, PR.flat(pref), PR.flat(mnh), Wout,
                                 stream=stream.cuda_stream, **ptr)

    for t in bufs.values():
        t.fill_(-1)
    rc = record("c_policy", rig, call_c, bufs, table, pref, mnh, PR.KEYS, bytes_c)
    rig.close()

    spread = (ra["ms_max"] - ra["ms_min"]) / ra["ms_median"]
    summary = dict(b_over_a_time=rb["ms_median"] / ra["ms_median"], b_over_a_bytes=bytes_b / bytes_a,
                   c_over_a_time=rc["ms_median"] / ra["ms_median"], c_over_a_bytes=bytes_c / bytes_a,
                   a_spread=spread, store_probe_gb_per_s=probe_gbs, drained_announcers=int(drained.size))
    print(json.dumps(summary), flush=True)
    out = dict(topology=f"fabric pods={args.pods} planes={args.planes}", V=len(names0),
               device=torch.cuda.get_device_name(0), cases=records, summary=summary)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not all(r["parity_ok"] for r in records):
        raise SystemExit("parity mismatch")


if __name__ == "__main__":
    main()
