"""Python face of libopenr_spf_hip (include/openr_spf.h).

``Engine`` owns one ospf_ctx on a HIP device. ``run`` is the synchronous
host-buffer batch (the drop-in ``ospf_sssp_batch``); ``run_dev`` queues a
device-resident batch on a stream (raw device pointers, e.g. from torch
tensors' ``data_ptr()``) — that is what bench.py times.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _native as N


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ospf error {code}: {msg}")
        self.code = code


def csr_struct(csr: Dict[str, np.ndarray]):
    keep = {k: np.ascontiguousarray(v) for k, v in csr.items()}
    s = N.ospf_csr(int(keep["row_ptr"].size - 1), int(keep["col"].size),
                   keep["row_ptr"].ctypes.data, keep["col"].ctypes.data,
                   keep["metric"].ctypes.data, keep["link_id"].ctypes.data,
                   keep["twin"].ctypes.data, keep["edge_up"].ctypes.data,
                   keep["no_transit"].ctypes.data,
                   keep["link_rank"].ctypes.data if "link_rank" in keep else None)
    return s, keep


def select_table(offsets: Sequence[int], nodes: Sequence[int]):
    """(ospf_select_table, the arrays it points into) of a CSR prefix table."""
    off = np.ascontiguousarray(offsets, np.uint32)
    ids = np.ascontiguousarray(nodes, np.uint32)
    if off.size < 1:
        raise ValueError("offsets needs n_prefixes + 1 entries")
    t = N.ospf_select_table(int(off.size - 1), off.ctypes.data, ids.ctypes.data if ids.size else None)
    return t, (off, ids)


POLICY_OUTPUTS = ("metric", "count", "nh", "links", "need", "best")


def select_ptable(offsets: Sequence[int], nodes: Sequence[int], pref: Optional[Sequence[int]],
                  min_nexthop: Optional[Sequence[int]] = None):
    """(ospf_select_ptable, the arrays it points into): the CSR prefix table
    with a class rank (< 2^31, smaller wins) and optionally a minNexthop
    threshold (0 = unset) per announcer entry. pref None passes NULL."""
    off = np.ascontiguousarray(offsets, np.uint32)
    ids = np.ascontiguousarray(nodes, np.uint32)
    if off.size < 1:
        raise ValueError("offsets needs n_prefixes + 1 entries")
    pr = None if pref is None else np.ascontiguousarray(pref, np.uint32)
    mn = None if min_nexthop is None else np.ascontiguousarray(min_nexthop, np.uint32)
    for a in (pr, mn):
        if a is not None and a.size != ids.size:
            raise ValueError("pref / min_nexthop: one per announcer entry")
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    t = N.ospf_select_ptable(int(off.size - 1), off.ctypes.data, ptr(ids), ptr(pr), ptr(mn))
    return t, (off, ids, pr, mn)


def _policy_host_out(n: int, P: int, W: int, want: Sequence[str]):
    bad = set(want) - set(POLICY_OUTPUTS)
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    arrs = {k: np.zeros((n, P, W) if k == "nh" else (n, P), np.uint32) for k in want}
    o = N.ospf_select_pout(*[arrs[k].ctypes.data if k in arrs else None for k in POLICY_OUTPUTS])
    return o, arrs


SRMPLS_OUTPUTS = ("metric", "count", "links", "need", "best", "dst_links", "dst_nh")


def select_stable(offsets: Sequence[int], nodes: Sequence[int], pref: Optional[Sequence[int]],
                  min_nexthop: Optional[Sequence[int]] = None,
                  flags: Optional[Sequence[int]] = None):
    """(ospf_select_stable, the arrays it points into): select_ptable's table
    with a flag word per announcer entry (bit 0: the entry has a prepend
    label, OSPF_SEL_SELF_PREPEND); flags None passes NULL (all 0)."""
    pt, (off, ids, pr, mn) = select_ptable(offsets, nodes, pref, min_nexthop)
    fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
    if fl is not None and fl.size != ids.size:
        raise ValueError("flags: one per announcer entry")
    t = N.ospf_select_stable(pt.n_prefixes, pt.offsets, pt.nodes, pt.pref, pt.min_nexthop,
                             fl.ctypes.data if fl is not None and fl.size else None)
    return t, (off, ids, pr, mn, fl)


AREAS_OUTPUTS = ("metric", "count", "links", "need", "best", "areas", "nh")


def areas_table(sweeps: Sequence["Sweep"], gids: Sequence[Sequence[int]], n_global: int,
                offsets: Sequence[int], node: Sequence[int], area: Sequence[int],
                pref: Optional[Sequence[int]], min_nexthop: Optional[Sequence[int]] = None):
    """(ospf_areas_table, the arrays it points into): one sweep and one
    node id -> global id list per area (area-name order) and the CSR table of
    (global node, area) entries with a class rank and optionally a minNexthop
    threshold each. A sweep given as None passes NULL; pref None passes NULL."""
    A = len(sweeps)
    hs = (C.c_void_p * max(1, A))(*[None if s is None else s._h for s in sweeps])
    gs = [np.ascontiguousarray(g, np.uint32) for g in gids]
    gp = (C.c_void_p * max(1, A))(*[g.ctypes.data if g.size else None for g in gs])
    off = np.ascontiguousarray(offsets, np.uint32)
    cols = [None if c is None else np.ascontiguousarray(c, np.uint32)
            for c in (node, area, pref, min_nexthop)]
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    t = N.ospf_areas_table(A, C.cast(hs, C.c_void_p), C.cast(gp, C.c_void_p), int(n_global),
                           max(0, int(off.size) - 1), off.ctypes.data if off.size else None,
                           *[ptr(c) for c in cols])
    return t, (hs, gs, gp, off, cols)


def _areas_last_error(sweeps) -> str:
    s = sweeps[0] if len(sweeps) else None
    return "" if s is None else s._L.ospf_sweep_last_error(s._h).decode()


def select_policy_areas(sweeps: Sequence["Sweep"], gids: Sequence[Sequence[int]], n_global: int,
                        offsets: Sequence[int], node: Sequence[int], area: Sequence[int],
                        pref: Optional[Sequence[int]],
                        min_nexthop: Optional[Sequence[int]] = None,
                        nh_words: Optional[Sequence[int]] = None,
                        want: Sequence[str] = AREAS_OUTPUTS) -> Dict[str, object]:
    """ospf_areas_select_policy: the reference's best-route selection across
    several areas (one sweep per area, area-name order) for every node of the
    union and every prefix -> {metric, count, links, need, best, areas [G, P]
    u32 by global id, nh: a list of [V_a, P, W_a] u32 by each area's node id};
    only the outputs named in `want` are computed. best is the entry's
    position within its prefix."""
    bad = set(want) - set(AREAS_OUTPUTS)
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    L = N.engine()
    t, keep = areas_table(sweeps, gids, n_global, offsets, node, area, pref, min_nexthop)
    G, P, A = int(n_global), int(t.n_prefixes), len(sweeps)
    out: Dict[str, object] = {k: np.zeros((G, P), np.uint32) for k in want if k != "nh"}
    W = np.ascontiguousarray(
        nh_words if nh_words is not None else [max(1, s.max_nh_words) for s in sweeps], np.uint32)
    nhp = None
    if "nh" in want:
        out["nh"] = [np.zeros((len(gids[a]), P, int(W[a])), np.uint32) for a in range(A)]
        nhp = (C.c_void_p * max(1, A))(*[x.ctypes.data for x in out["nh"]])
    o = N.ospf_areas_pout(*[out[k].ctypes.data if k in out else None for k in AREAS_OUTPUTS[:6]],
                          C.cast(nhp, C.c_void_p) if nhp is not None else None, W.ctypes.data)
    rc = L.ospf_areas_select_policy(C.byref(t), C.byref(o))
    if rc != 0:
        raise EngineError(rc, _areas_last_error(sweeps))
    return out


def select_policy_areas_dev(sweeps: Sequence["Sweep"], gids: Sequence[Sequence[int]],
                            n_global: int, offsets: Sequence[int], node: Sequence[int],
                            area: Sequence[int], pref: Optional[Sequence[int]],
                            min_nexthop: Optional[Sequence[int]],
                            nh_words: Optional[Sequence[int]], *, d_metric: int = 0,
                            d_count: int = 0, d_links: int = 0, d_need: int = 0, d_best: int = 0,
                            d_areas: int = 0, d_nh: Optional[Sequence[int]] = None,
                            stream: int = 0) -> None:
    """ospf_areas_select_policy_dev: the same into device memory (raw pointers;
    0 = not wanted; d_nh one pointer per area), queued on `stream` after the
    uploads."""
    L = N.engine()
    t, keep = areas_table(sweeps, gids, n_global, offsets, node, area, pref, min_nexthop)
    A = len(sweeps)
    W = None if nh_words is None else np.ascontiguousarray(nh_words, np.uint32)
    nhp = None if d_nh is None else (C.c_void_p * max(1, A, len(d_nh)))(*[p or None for p in d_nh])
    o = N.ospf_areas_pout(d_metric or None, d_count or None, d_links or None, d_need or None,
                          d_best or None, d_areas or None,
                          C.cast(nhp, C.c_void_p) if nhp is not None else None,
                          W.ctypes.data if W is not None else None)
    rc = L.ospf_areas_select_policy_dev(C.byref(t), C.byref(o), stream or None)
    if rc != 0:
        raise EngineError(rc, _areas_last_error(sweeps))


# ospf_select_change / odl_select_change records
CHANGE_DTYPE = np.dtype([("root", np.uint32), ("prefix", np.uint32), ("metric", np.uint32),
                         ("count", np.uint32)])
# ospf_select_pchange records
PCHANGE_DTYPE = np.dtype([(k, np.uint32) for k in ("root", "prefix", "metric", "count", "links",
                                                   "need", "best", "installed")])


def decode_paths(recs: np.ndarray, status: np.ndarray, bad: int):
    """KSP2 records -> per row a list of paths (lists of link ids), None when
    `status & bad`."""
    out = []
    for rec, st in zip(recs, status):
        if int(st) & bad:
            out.append(None)
            continue
        paths, q = [], 1
        for _ in range(int(rec[0])):
            ln = int(rec[q])
            paths.append([int(x) for x in rec[q + 1:q + 1 + ln]])
            q += 1 + ln
        out.append(paths)
    return out


class Engine:
    def __init__(self, device: int = 0):
        self._L = N.engine()
        h = C.c_void_p()
        rc = self._L.ospf_open(device, C.byref(h))
        if rc != 0:
            raise EngineError(rc, f"ospf_open(device={device}) failed: no usable HIP device")
        self._h = h
        self.V = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.ospf_close(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(rc, self._L.ospf_last_error(self._h).decode())

    def load(self, csr: Dict[str, np.ndarray], version: int = 1) -> None:
        s, keep = csr_struct(csr)
        self._check(self._L.ospf_load_graph(self._h, C.byref(s), version))
        self.V = int(s.n_nodes)

    def info(self) -> N.ospf_graph_info:
        gi = N.ospf_graph_info()
        self._check(self._L.ospf_graph_info_get(self._h, C.byref(gi)))
        return gi

    def root_neighbors(self, root: int) -> np.ndarray:
        n = C.c_uint32()
        self._check(self._L.ospf_root_neighbors(self._h, root, None, 0, C.byref(n)))
        ids = np.zeros(max(n.value, 1), np.uint32)
        self._check(self._L.ospf_root_neighbors(self._h, root, ids.ctypes.data, n.value,
                                                C.byref(n)))
        return ids[: n.value]

    def nh_words(self, root: int) -> int:
        return max(1, (len(self.root_neighbors(root)) + 31) // 32)

    def plan_variant(self, nh_words: int, flags: int = 0) -> int:
        v = C.c_int()
        self._check(self._L.ospf_plan_variant(self._h, flags, nh_words, C.byref(v)))
        return v.value

    def plan(self, nh_words: int, flags: int = 0, max_ignored: int = 0,
             n_roots: int = 0xFFFFFFFF, max_root_neighbors: int = 0) -> dict:
        p = N.ospf_plan_info()
        self._check(self._L.ospf_plan_n(self._h, flags, nh_words, max_ignored, n_roots,
                                        max_root_neighbors, C.byref(p)))
        return dict(variant=p.variant, block=p.block, lds_bytes=p.lds_bytes, slices=p.slices)

    @property
    def spf_runs(self) -> int:
        return int(self._L.ospf_spf_runs(self._h))

    def run(self, roots: Sequence[int], nh_words: int, *, hop_count: bool = False,
            want_dist: bool = True, want_nh: bool = True, want_digest: bool = False,
            ignore: Optional[Sequence[Sequence[int]]] = None):
        """Synchronous batch. Returns dict with dist [n,V] u32, nh [n,V,W] u32,
        digest [n,3] u64 (only the requested ones)."""
        roots = np.ascontiguousarray(roots, np.uint32)
        n, V, W = roots.size, self.V, nh_words
        flags = (N.OSPF_HOP_COUNT if hop_count else 0) | \
            (N.OSPF_WANT_DIST if want_dist else 0) | (N.OSPF_WANT_NH if want_nh else 0) | \
            (N.OSPF_WANT_DIGEST if want_digest else 0)
        dist = np.zeros((n, V), np.uint32) if want_dist else None
        nh = np.zeros((n, V, W), np.uint32) if want_nh else None
        dig = np.zeros((n, 3), np.uint64) if want_digest else None
        ig_ref = None
        if ignore is not None:
            off = np.zeros(n + 1, np.uint32)
            off[1:] = np.cumsum([len(x) for x in ignore])
            ids = np.ascontiguousarray(np.concatenate(
                [np.sort(np.asarray(x, np.uint32)) for x in ignore]) if off[-1] else
                np.zeros(1, np.uint32), np.uint32)
            ig = N.ospf_ignore(off.ctypes.data, ids.ctypes.data)
            ig_ref = (C.byref(ig), off, ids)
        self._check(self._L.ospf_sssp_batch(
            self._h, roots.ctypes.data, n, ig_ref[0] if ig_ref else None, flags, W,
            dist.ctypes.data if dist is not None else None,
            nh.ctypes.data if nh is not None else None,
            dig.ctypes.data if dig is not None else None))
        out = {}
        if want_dist:
            out["dist"] = dist
        if want_nh:
            out["nh"] = nh
        if want_digest:
            out["digest"] = dig
        return out

    def run_dev(self, d_roots: int, n_roots: int, nh_words: int, *, flags: int,
                d_dist: int = 0, d_nh: int = 0, d_digest: int = 0, stream: int = 0,
                d_ign_off: int = 0, d_ign_ids: int = 0, max_ignored: int = 0,
                max_root_neighbors: int = 0) -> None:
        """Queue a device-resident batch (raw device pointers) on `stream`.
        max_root_neighbors: optional bound on the roots' distinct neighbour
        counts (sizes the multi-source BFS; 0 = 32 * nh_words)."""
        b = N.ospf_batch(d_roots, n_roots, d_ign_off or None, d_ign_ids or None, max_ignored,
                         flags, nh_words, max_root_neighbors, d_dist or None, d_nh or None,
                         d_digest or None)
        self._check(self._L.ospf_run_batch_dev(self._h, C.byref(b), stream or None))

    @property
    def lev_pitch(self) -> int:
        """Bytes per level row for levels_dev / nh_derive_dev (V rounded up to 16)."""
        return (self.V + 15) // 16 * 16

    def levels_dev(self, d_roots: int, n: int, d_lev: int, *, d_dist: int = 0,
                   d_lev_digest: int = 0, hop_count: bool = False, stream: int = 0,
                   lev_pitch: int = 0) -> None:
        """Derive phase 1 (ospf_levels_dev): dist rows [n][V] (optional), byte
        level rows [n][lev_pitch] and the distance part of each run's digest
        (optional, [n][3] u64) of the n device roots."""
        self._check(self._L.ospf_levels_dev(self._h, d_roots, n,
                                            N.OSPF_HOP_COUNT if hop_count else 0,
                                            d_dist or None, d_lev, lev_pitch or self.lev_pitch,
                                            d_lev_digest or None, stream or None))

    def nh_derive_dev(self, d_roots: int, n: int, nh_words: int, d_lev: int, d_pos: int,
                      d_nh: int, *, d_lev_digest: int = 0, d_digest: int = 0,
                      max_root_neighbors: int = 0, stream: int = 0, lev_pitch: int = 0) -> None:
        """Derive phase 2 (ospf_nh_derive_dev): next-hop rows [n][V][nh_words]
        (+ digests, completing d_lev_digest's parts) from level rows;
        d_pos[v] = level row of node v."""
        self._check(self._L.ospf_nh_derive_dev(self._h, d_roots, n, nh_words, max_root_neighbors,
                                               d_lev, lev_pitch or self.lev_pitch, d_pos,
                                               d_lev_digest or None, d_nh, d_digest or None,
                                               stream or None))

    def wderive_dev(self, d_roots: int, n: int, d_src: int, d_pos: int, d_dist: int, *,
                    src_pitch: int = 0, d_nh: int = 0, d_digest: int = 0,
                    max_root_neighbors: int = 0, hop_count: bool = False,
                    stream: int = 0) -> None:
        """Weighted derive (ospf_wderive_dev): dist rows [n][V], one-word
        next-hop rows [n][V] and digests of n leaf roots (<= 32 distinct
        neighbours) from their neighbours' distance rows
        (d_src + d_pos[v] * src_pitch words)."""
        self._check(self._L.ospf_wderive_dev(self._h, d_roots, n,
                                             N.OSPF_HOP_COUNT if hop_count else 0,
                                             max_root_neighbors, d_src, src_pitch or self.V,
                                             d_pos, d_dist, d_nh or None, d_digest or None,
                                             stream or None))

    def cover_prepare(self, leaf_mask) -> None:
        """ospf_cover_prepare: contracted graph of the cover (nodes outside the
        independent leaf set, leaf_mask[V] bool) for cover_dist_dev."""
        m = np.ascontiguousarray(leaf_mask, np.uint8)
        self._check(self._L.ospf_cover_prepare(self._h, m.ctypes.data))

    def cover_dist_dev(self, d_roots: int, n: int, d_dist: int, stream: int = 0) -> None:
        """ospf_cover_dist_dev: dist rows [n][V] of n cover roots (node ids)."""
        self._check(self._L.ospf_cover_dist_dev(self._h, d_roots, n, d_dist, stream or None))

    def wderive_wide_dev(self, d_roots: int, n: int, nh_words: int, d_src: int, d_pos: int,
                         d_nh: int, *, src_pitch: int = 0, d_digest: int = 0,
                         hop_count: bool = False, stream: int = 0) -> None:
        """ospf_wderive_wide_dev: next-hop rows [n][V][nh_words] (<= 4 words)
        + digests of n roots from their own and their neighbours' dist rows."""
        self._check(self._L.ospf_wderive_wide_dev(self._h, d_roots, n,
                                                  N.OSPF_HOP_COUNT if hop_count else 0, nh_words,
                                                  d_src, src_pitch or self.V, d_pos, d_nh,
                                                  d_digest or None, stream or None))

    def ksp2(self, src: int, dsts: Sequence[int], path_cap: int = 512):
        """getKthPaths(src, d, 1) and (src, d, 2) for every d (ospf_ksp2_run).
        Returns (k1, k2, status): per destination a list of paths (lists of
        link ids, src -> dst) or None where status says the engine's budget
        was exceeded, and the status words."""
        dsts = np.ascontiguousarray(dsts, np.uint32)
        n = dsts.size
        k1 = np.zeros((max(n, 1), path_cap), np.uint32)
        k2 = np.zeros_like(k1)
        st = np.zeros(max(n, 1), np.uint32)
        a = N.ospf_ksp2(src, dsts.ctypes.data, n, path_cap, k1.ctypes.data, k2.ctypes.data,
                        st.ctypes.data)
        self._check(self._L.ospf_ksp2_run(self._h, C.byref(a)))
        return (decode_paths(k1[:n], st[:n], N.OSPF_KSP_OVF1),
                decode_paths(k2[:n], st[:n], N.OSPF_KSP_OVF2 | N.OSPF_KSP_OVF1), st[:n])

    def ksp2_stats(self) -> dict:
        """ospf_ksp2_stats: k = 2 runs by the decremental kernel, runs sent to
        the full masked reruns, affected nodes summed (since open)."""
        out = np.zeros(3, np.uint64)
        self._check(self._L.ospf_ksp2_stats(self._h, out.ctypes.data))
        return {"decremental": int(out[0]), "full_reruns": int(out[1]), "affected": int(out[2])}

    def ksp2_dev(self, src: int, d_dsts: int, n: int, path_cap: int, d_k1: int, d_k2: int,
                 d_status: int, stream: int = 0) -> None:
        a = N.ospf_ksp2(src, d_dsts, n, path_cap, d_k1, d_k2, d_status)
        self._check(self._L.ospf_ksp2_dev(self._h, C.byref(a), stream or None))

    def update_links(self, updates, version: int) -> None:
        """updates: iterable of (link_id, up, metric_lo, metric_hi)."""
        ups = list(updates)
        arr = (N.ospf_link_update * max(len(ups), 1))(*[N.ospf_link_update(*u) for u in ups])
        self._check(self._L.ospf_update_links(self._h, arr, len(ups), version))

    def update_rows(self, csr: Dict[str, np.ndarray], rows, version: int) -> None:
        """ospf_update_rows: links added / removed in place; `csr` is the
        whole CSR after the change, `rows` the nodes whose rows changed."""
        s, keep = csr_struct(csr)
        r = np.ascontiguousarray(rows, np.uint32)
        self._check(self._L.ospf_update_rows(self._h, C.byref(s), r.ctypes.data if r.size else None,
                                             r.size, version))

    def update_nodes(self, nodes, no_transit, version: int) -> None:
        n = np.ascontiguousarray(nodes, np.uint32)
        t = np.ascontiguousarray(no_transit, np.uint8)
        self._check(self._L.ospf_update_nodes(self._h, n.ctypes.data, t.ctypes.data, n.size,
                                              version))

    def affected(self, d_dist: int, n_roots: int, changes, d_out: int, flags: int = 0,
                 stream: int = 0) -> None:
        """changes: iterable of ospf_change field tuples
        (kind, a, b, up0, w_ab0, w_ba0, up1, w_ab1, w_ba1)."""
        ch = list(changes)
        arr = (N.ospf_change * max(len(ch), 1))(*[N.ospf_change(*c) for c in ch])
        self._check(self._L.ospf_affected_roots(self._h, d_dist, n_roots, flags, arr, len(ch),
                                                d_out, stream or None))

    def repair(self, d_roots: int, n: int, nh_words: int, d_dist: int, d_nh: int, changes,
               d_status: int, flags: int = 0, stream: int = 0) -> None:
        """ospf_repair_runs: fix finished rows in place after a patch; d_status
        [n] u32 = 1 where the run must be re-run."""
        ch = list(changes)
        arr = (N.ospf_change * max(len(ch), 1))(*[N.ospf_change(*c) for c in ch])
        self._check(self._L.ospf_repair_runs(self._h, d_roots, n, flags, nh_words, d_dist, d_nh,
                                             arr, len(ch), d_status, stream or None))

    def sync(self, stream: int = 0) -> None:
        self._check(self._L.ospf_sync(self._h, stream or None))

    def links_mask(self, link_ids, version: int) -> None:
        ids = np.ascontiguousarray(link_ids, np.uint32)
        self._check(self._L.ospf_links_mask(self._h, ids.ctypes.data, ids.size, version))

    def links_unmask(self) -> None:
        self._check(self._L.ospf_links_unmask(self._h))

    def sweep(self, **kw) -> "Sweep":
        return Sweep(self, **kw)

    PROBES = {"stream": 0, "rows_chunk": 1, "rows_group": 2, "rows_walk": 3}

    def probe_store(self, pattern: str, V: int, rows: int, group: int = 48, ctiles: int = 6,
                    reps: int = 3) -> np.ndarray:
        """ospf_probe_store: ms per launch writing 2 * rows * V * 4 bytes with
        16-B non-temporal stores (box calibration for the roofline)."""
        out = np.zeros(reps, np.float32)
        self._check(self._L.ospf_probe_store(self._h, self.PROBES[pattern], V, rows, group,
                                             ctiles, reps, out.ctypes.data))
        return out


class Sweep:
    """All-sources sweep (ospf_sweep_*): runSpf for every node of the graph,
    or for part `part` of `n_parts` of the root partition; the library owns
    the path, the width classes, their streams, the row buffers and the HIP
    graph one run replays. ``run(stream)`` queues one sweep."""

    def __init__(self, engine: "Engine", *, hop_count: bool = False, mode: str = "auto",
                 part: int = 0, n_parts: int = 1, hip_graph: bool = True, defer: bool = False,
                 early_start: bool = False, _handle=None):
        self._L = N.engine()
        self.engine = engine
        if _handle is not None:  # a part of an ospf_msweep (owned by it)
            self._h, self._owned = _handle, False
        else:
            # defer: no eager run at create (hip_graph must be off): the
            # first run() is the first run (OSPF_SWEEP_DEFER)
            # early_start (with defer): the first run's serial prefix is
            # queued while the plan is built (OSPF_SWEEP_EARLY_START)
            o = N.ospf_sweep_opts((N.OSPF_HOP_COUNT if hop_count else 0) |
                                  (N.OSPF_SWEEP_DEFER if defer else 0) |
                                  (N.OSPF_SWEEP_EARLY_START if early_start else 0),
                                  N.SWEEP_MODES[mode],
                                  part, n_parts, int(hip_graph and not defer))
            h = C.c_void_p()
            rc = self._L.ospf_sweep_create(engine._h, C.byref(o), C.byref(h))
            if rc != 0:
                raise EngineError(rc, self._L.ospf_last_error(engine._h).decode())
            self._h, self._owned = h, True
        gi = N.ospf_sweep_info()
        self._check(self._L.ospf_sweep_get_info(self._h, C.byref(gi)))
        self.mode = N.SWEEP_MODE_NAMES[gi.mode]
        self.n_roots = int(gi.n_roots)
        self.n_rows = int(gi.n_rows)
        self.n_launches = int(gi.n_launches)
        self.hip_graph = bool(gi.hip_graph)
        self.max_nh_words = int(gi.max_nh_words)
        self.device_bytes = int(gi.device_bytes)
        self.step_compulsory_bytes = int(gi.step_compulsory_bytes)
        self.step_traversed_edges = int(gi.step_traversed_edges)
        r = np.zeros(max(1, self.n_roots), np.uint32)
        self._check(self._L.ospf_sweep_roots(self._h, r.ctypes.data))
        self.roots = r[: self.n_roots]

    def close(self):
        if getattr(self, "_h", None) and self._owned:
            self._L.ospf_sweep_destroy(self._h)
        self._h = None

    __del__ = close

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(rc, self._L.ospf_sweep_last_error(self._h).decode())

    def run(self, stream: int = 0) -> None:
        self._check(self._L.ospf_sweep_run(self._h, stream or None))

    def digests_dev(self, d_out: int, stream: int = 0) -> None:
        """Digests of the owned roots (roots order) into device memory [n][3] u64."""
        self._check(self._L.ospf_sweep_digests(self._h, d_out, stream or None))

    def poison(self, stream: int = 0) -> None:
        self._check(self._L.ospf_sweep_poison(self._h, stream or None))

    def row(self, root: int):
        """(device dist row pointer, device next-hop row pointer, next-hop words)."""
        d, nh, w = C.c_void_p(), C.c_void_p(), C.c_uint32()
        self._check(self._L.ospf_sweep_row(self._h, int(root), C.byref(d), C.byref(nh),
                                           C.byref(w)))
        return d.value, nh.value, int(w.value)

    def rows(self, roots: Sequence[int], nh_words: int = 0):
        """Host copies of owned roots' rows: dist [n, V] u32, nh [n, V, W] u32
        (W = nh_words or the widest of the roots)."""
        roots = np.ascontiguousarray(roots, np.uint32)
        V = self.engine.V
        W = nh_words or max([self.row(r)[2] for r in roots.tolist()] or [1])
        dist = np.zeros((roots.size, V), np.uint32)
        nh = np.zeros((roots.size, V, W), np.uint32)
        self._check(self._L.ospf_sweep_copy_rows(self._h, roots.ctypes.data, roots.size, W,
                                                 dist.ctypes.data, nh.ctypes.data))
        return dist, nh

    def select(self, offsets: Sequence[int], nodes: Sequence[int], nh_words: int = 0):
        """ospf_sweep_select: getNextHopsWithMetric for every owned root and
        every prefix of the CSR table (prefix p announced by
        nodes[offsets[p]:offsets[p + 1]], ids strictly ascending) ->
        (metric [n, P] u32, count [n, P] u32, nh [n, P, W] u32) in `roots`
        order, W = nh_words or the sweep's max_nh_words."""
        t, keep = select_table(offsets, nodes)
        n, P, W = self.n_roots, int(t.n_prefixes), nh_words or max(1, self.max_nh_words)
        metric = np.zeros((n, P), np.uint32)
        count = np.zeros((n, P), np.uint32)
        nh = np.zeros((n, P, W), np.uint32)
        self._check(self._L.ospf_sweep_select(self._h, C.byref(t), W, metric.ctypes.data,
                                              count.ctypes.data, nh.ctypes.data))
        return metric, count, nh

    def select_dev(self, offsets: Sequence[int], nodes: Sequence[int], nh_words: int, *,
                   d_metric: int = 0, d_count: int = 0, d_nh: int = 0, stream: int = 0) -> None:
        """ospf_sweep_select_dev: the same into device memory (raw pointers,
        [n, P] / [n, P] / [n, P, nh_words] u32; 0 = not wanted), queued on
        `stream` after the table's upload."""
        t, keep = select_table(offsets, nodes)
        self._check(self._L.ospf_sweep_select_dev(self._h, C.byref(t), nh_words, d_metric or None,
                                                  d_count or None, d_nh or None, stream or None))

    def select_policy(self, offsets: Sequence[int], nodes: Sequence[int],
                      pref: Optional[Sequence[int]],
                      min_nexthop: Optional[Sequence[int]] = None, nh_words: int = 0,
                      want: Sequence[str] = POLICY_OUTPUTS) -> Dict[str, np.ndarray]:
        """ospf_sweep_select_policy: the reference's best-route selection
        (reached announcers, best pref class, drain filter, minNexthop) for
        every owned root and every prefix -> {metric, count, links, need, best
        [n, P] u32, nh [n, P, W] u32} in `roots` order; only the outputs named
        in `want` are computed."""
        t, keep = select_ptable(offsets, nodes, pref, min_nexthop)
        W = nh_words or max(1, self.max_nh_words)
        o, arrs = _policy_host_out(self.n_roots, int(t.n_prefixes), W, want)
        self._check(self._L.ospf_sweep_select_policy(self._h, C.byref(t), W, C.byref(o)))
        return arrs

    def select_policy_dev(self, offsets: Sequence[int], nodes: Sequence[int],
                          pref: Optional[Sequence[int]],
                          min_nexthop: Optional[Sequence[int]], nh_words: int, *,
                          d_metric: int = 0, d_count: int = 0, d_nh: int = 0, d_links: int = 0,
                          d_need: int = 0, d_best: int = 0, stream: int = 0) -> None:
        """ospf_sweep_select_policy_dev: the same into device memory (raw
        pointers; 0 = not wanted), queued on `stream` after the table's upload."""
        t, keep = select_ptable(offsets, nodes, pref, min_nexthop)
        o = N.ospf_select_pout(d_metric or None, d_count or None, d_nh or None, d_links or None,
                               d_need or None, d_best or None)
        self._check(self._L.ospf_sweep_select_policy_dev(self._h, C.byref(t), nh_words,
                                                         C.byref(o), stream or None))

    def select_srmpls(self, offsets: Sequence[int], nodes: Sequence[int],
                      pref: Optional[Sequence[int]],
                      min_nexthop: Optional[Sequence[int]] = None,
                      flags: Optional[Sequence[int]] = None, nh_words: int = 0,
                      want: Sequence[str] = SRMPLS_OUTPUTS) -> Dict[str, np.ndarray]:
        """ospf_sweep_select_srmpls: select_policy's selection for prefixes
        forwarded as SR_MPLS, the next hops kept per destination (table entry)
        -> {metric, count, links, need, best [n, P] u32, dst_links [n, A] u32,
        dst_nh [n, A, W] u32} in `roots` order, A = offsets[-1]; flags: bit 0
        per entry = it has a prepend label (an announcing root with it routes
        to the other announcers). Only the outputs named in `want` are
        computed; dst_nh is the large one."""
        bad = set(want) - set(SRMPLS_OUTPUTS)
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}")
        t, keep = select_stable(offsets, nodes, pref, min_nexthop, flags)
        W = nh_words or max(1, self.max_nh_words)
        n, P, A = self.n_roots, int(t.n_prefixes), int(keep[1].size)
        shape = {"dst_links": (n, A), "dst_nh": (n, A, W)}
        arrs = {k: np.zeros(shape.get(k, (n, P)), np.uint32) for k in want}
        o = N.ospf_select_sout(*[arrs[k].ctypes.data if k in arrs else None
                                 for k in SRMPLS_OUTPUTS])
        self._check(self._L.ospf_sweep_select_srmpls(self._h, C.byref(t), W, C.byref(o)))
        return arrs

    def select_srmpls_dev(self, offsets: Sequence[int], nodes: Sequence[int],
                          pref: Optional[Sequence[int]], min_nexthop: Optional[Sequence[int]],
                          flags: Optional[Sequence[int]], nh_words: int, *, d_metric: int = 0,
                          d_count: int = 0, d_links: int = 0, d_need: int = 0, d_best: int = 0,
                          d_dst_links: int = 0, d_dst_nh: int = 0, stream: int = 0) -> None:
        """ospf_sweep_select_srmpls_dev: the same into device memory (raw
        pointers; 0 = not wanted), queued on `stream` after the table's upload."""
        t, keep = select_stable(offsets, nodes, pref, min_nexthop, flags)
        o = N.ospf_select_sout(d_metric or None, d_count or None, d_links or None, d_need or None,
                               d_best or None, d_dst_links or None, d_dst_nh or None)
        self._check(self._L.ospf_sweep_select_srmpls_dev(self._h, C.byref(t), nh_words,
                                                         C.byref(o), stream or None))

    def profile(self, reps: int = 3):
        """Every launch unit timed alone on its stream -> list of dicts."""
        cap = max(1, self.n_launches)
        arr = (N.ospf_sweep_launch * cap)()
        self._check(self._L.ospf_sweep_profile(self._h, reps, arr, cap))
        return [dict(name=a.name.decode(), kernel=a.kernel.decode(), n_roots=int(a.n_roots),
                     nh_words=int(a.nh_words), compulsory_bytes=int(a.compulsory_bytes),
                     ms_median=float(a.ms_median), ms_min=float(a.ms_min))
                for a in arr[: self.n_launches]]

    def graph_memsets(self):
        """Diagnostic: the captured graph's memset nodes -> (count, with a
        destination outside every live allocation, inside the sweep's own
        blocks); see ospf_sweep_graph_memsets."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._L.ospf_sweep_graph_memsets(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)


class SelStateOverflow(EngineError):
    """ospf_selstate_update's OSPF_E_RANGE (-4): more changes or rebased
    roots than the capacities; the state is unchanged. n_changes / n_rebased
    are the complete counts to retry with."""

    def __init__(self, msg: str, n_changes: int, n_rebased: int):
        super().__init__(-4, msg)
        self.n_changes = n_changes
        self.n_rebased = n_rebased


class UcmpOverflow(EngineError):
    """ospf_selstate_ucmp_copy's OSPF_E_RANGE (-4): more next-hop weights than
    the capacity; nothing was written. n_wt is the count to retry with."""

    def __init__(self, msg: str, n_wt: int):
        super().__init__(-4, msg)
        self.n_wt = n_wt


UCMP_ALGOS = {"adj": 2, "prefix": 3}  # OSPF_UCMP_ADJ / OSPF_UCMP_PREFIX
UCMP_OK, UCMP_NONE, UCMP_VOID, UCMP_OVERFLOW = 0, 1, 2, 3


class SelState:
    """ospf_selstate: the selection of one prefix table for every root, kept
    on the device in each root's own width, and the entries a later sweep
    changed (DecisionRouteDb::calculateUpdate for ospf_sweep_select's route
    DB). Bound to an Engine (not to a Sweep) and to one table. With `pref`
    (a class rank per announcer entry; optionally `min_nexthop`) a policy
    state: it holds Sweep.select_policy's selection and is driven by
    update_policy / copy_policy / set_policy instead of update."""

    def __init__(self, engine: "Engine", offsets: Sequence[int], nodes: Sequence[int],
                 pref: Optional[Sequence[int]] = None,
                 min_nexthop: Optional[Sequence[int]] = None):
        self._L = N.engine()
        self.engine = engine
        self.policy = pref is not None or min_nexthop is not None
        h = C.c_void_p()
        if self.policy:
            t, keep = select_ptable(offsets, nodes, pref, min_nexthop)
            rc = self._L.ospf_selstate_create_policy(engine._h, C.byref(t), C.byref(h))
        else:
            t, keep = select_table(offsets, nodes)
            rc = self._L.ospf_selstate_create(engine._h, C.byref(t), C.byref(h))
        if rc != 0:
            raise EngineError(rc, self._L.ospf_last_error(engine._h).decode())
        self.P = int(t.n_prefixes)
        self.n_entries = int(keep[1].size)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.ospf_selstate_destroy(self._h)
        self._h = None

    __del__ = close

    def _msg(self) -> str:
        return self._L.ospf_selstate_last_error(self._h).decode()

    @property
    def device_bytes(self) -> int:
        return int(self._L.ospf_selstate_device_bytes(self._h))

    def prime(self, sweep: "Sweep") -> None:
        """Store the sweep's selection as the baseline; reports nothing."""
        rc = self._L.ospf_selstate_prime(self._h, sweep._h)
        if rc != 0:
            raise EngineError(rc, self._msg())

    def update(self, sweep: "Sweep", cap: int = 1024, cap_rebased: int = 64, nh_words: int = 0,
               want_nh: bool = True):
        """Compare the sweep's selection with the stored one and commit it ->
        (changes [n] structured u32 root / prefix / metric / count with the NEW
        values, nh [n, W] u32 or None, rebased roots [m] u32). Raises
        SelStateOverflow (code -4, n_changes / n_rebased attached, state
        unchanged) when a list does not fit its capacity."""
        if cap < 0 or cap_rebased < 0 or nh_words < 0:
            raise ValueError("capacities and nh_words must be >= 0")
        W = nh_words or max(1, sweep.max_nh_words)
        rec = np.zeros(max(1, cap), CHANGE_DTYPE)
        nh = np.zeros((max(1, cap), W), np.uint32) if want_nh else None
        reb = np.zeros(max(1, cap_rebased), np.uint32)
        n, m = C.c_uint32(), C.c_uint32()
        rc = self._L.ospf_selstate_update(self._h, sweep._h, W, rec.ctypes.data,
                                          nh.ctypes.data if want_nh else None, cap, C.byref(n),
                                          reb.ctypes.data, cap_rebased, C.byref(m))
        if rc == -4:
            raise SelStateOverflow(self._msg(), int(n.value), int(m.value))
        if rc != 0:
            raise EngineError(rc, self._msg())
        return rec[: n.value], (nh[: n.value] if want_nh else None), reb[: m.value]

    def copy(self, roots: Sequence[int], nh_words: int):
        """The stored selection of `roots` (node ids), expanded like
        Sweep.select: (metric [n, P], count [n, P], nh [n, P, nh_words])."""
        roots = np.ascontiguousarray(roots, np.uint32)
        if nh_words < 1:
            raise ValueError("nh_words must be >= 1")
        metric = np.zeros((roots.size, self.P), np.uint32)
        count = np.zeros((roots.size, self.P), np.uint32)
        nh = np.zeros((roots.size, self.P, nh_words), np.uint32)
        rc = self._L.ospf_selstate_copy(self._h, roots.ctypes.data, roots.size, nh_words,
                                        metric.ctypes.data, count.ctypes.data, nh.ctypes.data)
        if rc != 0:
            raise EngineError(rc, self._msg())
        return metric, count, nh

    # ------------------------------------------------------------ policy
    def update_policy(self, sweep: "Sweep", cap: int = 1024, cap_rebased: int = 64,
                      nh_words: int = 0, want_nh: bool = True):
        """ospf_selstate_update_policy: update() for a policy state -> (changes
        [n] structured u32 root / prefix / metric / count / links / need / best
        / installed with the NEW values, nh [n, W] u32 or None, rebased roots
        [m] u32). Raises SelStateOverflow as update() does."""
        if cap < 0 or cap_rebased < 0 or nh_words < 0:
            raise ValueError("capacities and nh_words must be >= 0")
        W = nh_words or max(1, sweep.max_nh_words)
        rec = np.zeros(max(1, cap), PCHANGE_DTYPE)
        nh = np.zeros((max(1, cap), W), np.uint32) if want_nh else None
        reb = np.zeros(max(1, cap_rebased), np.uint32)
        n, m = C.c_uint32(), C.c_uint32()
        rc = self._L.ospf_selstate_update_policy(self._h, sweep._h, W, rec.ctypes.data,
                                                 nh.ctypes.data if want_nh else None, cap,
                                                 C.byref(n), reb.ctypes.data, cap_rebased,
                                                 C.byref(m))
        if rc == -4:
            raise SelStateOverflow(self._msg(), int(n.value), int(m.value))
        if rc != 0:
            raise EngineError(rc, self._msg())
        return rec[: n.value], (nh[: n.value] if want_nh else None), reb[: m.value]

    def copy_policy(self, roots: Sequence[int], nh_words: int,
                    want: Sequence[str] = POLICY_OUTPUTS) -> Dict[str, np.ndarray]:
        """ospf_selstate_copy_policy: the committed entries of `roots` (node
        ids) in Sweep.select_policy's layout; only the outputs in `want`."""
        roots = np.ascontiguousarray(roots, np.uint32)
        if nh_words < 1:
            raise ValueError("nh_words must be >= 1")
        o, arrs = _policy_host_out(roots.size, self.P, nh_words, want)
        rc = self._L.ospf_selstate_copy_policy(self._h, roots.ctypes.data, roots.size, nh_words,
                                               C.byref(o))
        if rc != 0:
            raise EngineError(rc, self._msg())
        return arrs

    def set_policy(self, pref: Optional[Sequence[int]],
                   min_nexthop: Optional[Sequence[int]] = None) -> None:
        """ospf_selstate_set_policy: replace the class ranks and thresholds
        (one per announcer entry). Nothing committed changes; the next
        update_policy reports what the new attributes changed."""
        pr = None if pref is None else np.ascontiguousarray(pref, np.uint32)
        mn = None if min_nexthop is None else np.ascontiguousarray(min_nexthop, np.uint32)
        for a in (pr, mn):
            if a is not None and a.size != self.n_entries:
                raise ValueError("pref / min_nexthop: one per announcer entry")
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        rc = self._L.ospf_selstate_set_policy(self._h, ptr(pr), ptr(mn))
        if rc != 0:
            raise EngineError(rc, self._msg())

    # ------------------------------------------------------------ UCMP
    @property
    def ucmp_slots(self) -> int:
        """Distinct-neighbour slots of the loaded graph: the length of
        ucmp()'s link_weight_sum (ospf_root_neighbors order, node after node)."""
        n = C.c_uint32()
        self._L.ospf_selstate_ucmp_info(self._h, None, C.byref(n))
        return int(n.value)

    def ucmp(self, algo: str, leaf_weight: Sequence[int],
             link_weight_sum: Optional[Sequence[int]] = None) -> int:
        """ospf_selstate_ucmp: resolve the UCMP weight and status of every
        (node, prefix) over the stored selection and keep them on the device
        -> gather rounds taken (the hop depth of the deepest selected path).
        algo 'adj' | 'prefix'; leaf_weight parallel to the table's nodes;
        link_weight_sum one i64 per distinct-neighbour slot ('adj' needs it)."""
        lw = np.ascontiguousarray(leaf_weight, np.int64)
        ls = None if link_weight_sum is None else np.ascontiguousarray(link_weight_sum, np.int64)
        rounds = C.c_uint32()
        rc = self._L.ospf_selstate_ucmp(self._h, UCMP_ALGOS[algo], lw.ctypes.data if lw.size else None,
                                        None if ls is None else ls.ctypes.data,
                                        0 if ls is None else ls.size, C.byref(rounds))
        if rc != 0:
            raise EngineError(rc, self._msg())
        return int(rounds.value)

    def ucmp_copy(self, roots: Sequence[int], cap: Optional[int] = None):
        """ospf_selstate_ucmp_copy: the per-link view of `roots` (node ids) ->
        (advertised [n, P] i64, status [n, P] u8, off [n * P + 1] u64, wt i64):
        entry (i, p)'s normalised next-hop weights are wt[off[i * P + p] :
        off[i * P + p + 1]], one per set next-hop bit in bit order. cap None:
        retried once with the count the engine reports; else UcmpOverflow
        (code -4, n_wt attached) when the weights do not fit."""
        roots = np.ascontiguousarray(roots, np.uint32)
        n = roots.size
        adv = np.zeros((n, self.P), np.int64)
        status = np.zeros((n, self.P), np.uint8)
        off = np.zeros(n * self.P + 1, np.uint64)
        need = C.c_uint64()
        room = 1024 if cap is None else cap
        while True:
            wt = np.zeros(max(1, room), np.int64)
            rc = self._L.ospf_selstate_ucmp_copy(self._h, roots.ctypes.data, n, adv.ctypes.data,
                                                 status.ctypes.data, off.ctypes.data, wt.ctypes.data,
                                                 room, C.byref(need))
            if rc == -4 and cap is None and int(need.value) > room:
                room = int(need.value)
                continue
            if rc == -4:
                raise UcmpOverflow(self._msg(), int(need.value))
            if rc != 0:
                raise EngineError(rc, self._msg())
            return adv, status, off, wt[: int(need.value)]


# ospf_areas_change records, with the derived `installed` column
ACHANGE_DTYPE = np.dtype([(k, np.uint32) for k in ("root", "prefix", "metric", "count", "links",
                                                   "need", "best", "areas")])
ACHANGE_OUT_DTYPE = np.dtype(ACHANGE_DTYPE.descr + [("installed", np.uint32)])


class AreaSelState:
    """ospf_areastate: select_policy_areas' selection of one table of (global
    node, area) entries for every node of the union of the areas, kept on the
    device in each root's own widths, and the cells a later sweep of some areas
    (or a change of the attributes) changed. Bound to the areas' Engines (the
    sweeps are read for them and their node counts only) and to one table.
    Roots are global ids."""

    def __init__(self, sweeps: Sequence["Sweep"], gids: Sequence[Sequence[int]], n_global: int,
                 offsets: Sequence[int], node: Sequence[int], area: Sequence[int],
                 pref: Optional[Sequence[int]], min_nexthop: Optional[Sequence[int]] = None):
        self._L = N.engine()
        t, keep = areas_table(sweeps, gids, n_global, offsets, node, area, pref, min_nexthop)
        h = C.c_void_p()
        rc = self._L.ospf_areastate_create(C.byref(t), C.byref(h))
        if rc != 0:
            s = sweeps[0] if len(sweeps) else None
            raise EngineError(rc, "" if s is None else
                              self._L.ospf_last_error(s.engine._h).decode())
        self.A, self.G, self.P = len(sweeps), int(n_global), int(t.n_prefixes)
        self.n_entries = 0 if keep[4][0] is None else int(keep[4][0].size)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.ospf_areastate_destroy(self._h)
        self._h = None

    __del__ = close

    def _msg(self) -> str:
        return self._L.ospf_areastate_last_error(self._h).decode()

    def _sweeps(self, sweeps):
        if len(sweeps) != self.A:
            raise ValueError("one sweep per area of the state")
        return (C.c_void_p * max(1, self.A))(*[None if s is None else s._h for s in sweeps])

    def device_bytes(self) -> int:
        return int(self._L.ospf_areastate_device_bytes(self._h))

    def prime(self, sweeps: Sequence["Sweep"]) -> None:
        """Store the sweeps' selection as the baseline; reports nothing."""
        rc = self._L.ospf_areastate_prime(self._h, self._sweeps(sweeps))
        if rc != 0:
            raise EngineError(rc, self._msg())

    def update(self, sweeps: Sequence["Sweep"], cap: int = 1024, cap_rebased: int = 64,
               nh_words: Optional[Sequence[int]] = None):
        """ospf_areastate_update: compare the sweeps' selection with the stored
        one and commit it -> (records [n] structured u32 root / prefix / metric
        / count / links / need / best / areas / installed with the NEW values,
        nh [n, sum(nh_words)] u32 with area a's words from column
        sum(nh_words[:a]), rebased roots [m] u32). Raises SelStateOverflow
        (code -4, n_changes / n_rebased attached, state unchanged) when a list
        does not fit its capacity."""
        if cap < 0 or cap_rebased < 0:
            raise ValueError("capacities must be >= 0")
        W = np.ascontiguousarray(
            nh_words if nh_words is not None else [max(1, s.max_nh_words) for s in sweeps],
            np.uint32)
        if W.size != self.A:
            raise ValueError("one nh_words per area")
        rec = np.zeros(max(1, cap), ACHANGE_DTYPE)
        nh = np.zeros((max(1, cap), int(W.sum())), np.uint32)
        reb = np.zeros(max(1, cap_rebased), np.uint32)
        n, m = C.c_uint32(), C.c_uint32()
        rc = self._L.ospf_areastate_update(self._h, self._sweeps(sweeps), W.ctypes.data,
                                           rec.ctypes.data, nh.ctypes.data, cap, C.byref(n),
                                           reb.ctypes.data, cap_rebased, C.byref(m))
        if rc == -4:
            raise SelStateOverflow(self._msg(), int(n.value), int(m.value))
        if rc != 0:
            raise EngineError(rc, self._msg())
        out = np.zeros(n.value, ACHANGE_OUT_DTYPE)
        for k in ACHANGE_DTYPE.names:
            out[k] = rec[k][: n.value]
        out["installed"] = (out["links"] > 0) & (out["need"] <= out["links"])
        return out, nh[: n.value], reb[: m.value]

    def copy(self, roots: Sequence[int], nh_words: Sequence[int]) -> Dict[str, object]:
        """ospf_areastate_copy: the committed cells of `roots` (global ids) ->
        select_policy_areas' keys, rows in `roots` order: the six columns
        [n, P], nh a list of [n, P, nh_words[a]] (zero where the area does not
        hold the root)."""
        roots = np.ascontiguousarray(roots, np.uint32)
        W = np.ascontiguousarray(nh_words, np.uint32)
        if W.size != self.A:
            raise ValueError("one nh_words per area")
        n = int(roots.size)
        out: Dict[str, object] = {k: np.zeros((n, self.P), np.uint32) for k in AREAS_OUTPUTS[:6]}
        out["nh"] = [np.zeros((n, self.P, int(w)), np.uint32) for w in W]
        nhp = (C.c_void_p * max(1, self.A))(*[x.ctypes.data for x in out["nh"]])
        o = N.ospf_areas_pout(*[out[k].ctypes.data for k in AREAS_OUTPUTS[:6]],
                              C.cast(nhp, C.c_void_p), W.ctypes.data)
        rc = self._L.ospf_areastate_copy(self._h, roots.ctypes.data, n, C.byref(o))
        if rc != 0:
            raise EngineError(rc, self._msg())
        return out

    def set_policy(self, pref: Optional[Sequence[int]],
                   min_nexthop: Optional[Sequence[int]] = None) -> None:
        """ospf_areastate_set_policy: replace the class ranks and thresholds
        (one per entry). Nothing committed changes; the next update reports
        what the new attributes changed."""
        pr = None if pref is None else np.ascontiguousarray(pref, np.uint32)
        mn = None if min_nexthop is None else np.ascontiguousarray(min_nexthop, np.uint32)
        for a in (pr, mn):
            if a is not None and a.size != self.n_entries:
                raise ValueError("pref / min_nexthop: one per entry")
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        rc = self._L.ospf_areastate_set_policy(self._h, ptr(pr), ptr(mn))
        if rc != 0:
            raise EngineError(rc, self._msg())


class Multi:
    """Several devices behind one handle (ospf_multi_*): the graph replicated,
    sweeps partitioned by device slot, digests gathered by peer copies."""

    def __init__(self, devices: Sequence[int]):
        self._L = N.engine()
        devs = np.ascontiguousarray(devices, np.int32)
        h = C.c_void_p()
        rc = self._L.ospf_multi_open(devs.ctypes.data, devs.size, C.byref(h))
        if rc != 0:
            raise EngineError(rc, f"ospf_multi_open({list(devices)}) failed")
        self._h = h
        self.n = int(self._L.ospf_multi_size(h))
        self.V = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.ospf_multi_close(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(rc, self._L.ospf_multi_last_error(self._h).decode())

    def load(self, csr: Dict[str, np.ndarray], version: int = 1) -> None:
        s, keep = csr_struct(csr)
        self._check(self._L.ospf_multi_load_graph(self._h, C.byref(s), version))
        self.V = int(s.n_nodes)


class MultiSweep:
    """ospf_msweep_*: one sweep part per device slot of a Multi."""

    def __init__(self, multi: Multi, *, hop_count: bool = False, mode: str = "auto",
                 hip_graph: bool = True):
        self._L = N.engine()
        self.multi = multi
        o = N.ospf_sweep_opts(N.OSPF_HOP_COUNT if hop_count else 0, N.SWEEP_MODES[mode], 0, 0,
                              int(hip_graph))
        h = C.c_void_p()
        rc = self._L.ospf_msweep_create(multi._h, C.byref(o), C.byref(h))
        if rc != 0:
            raise EngineError(rc, self._L.ospf_multi_last_error(multi._h).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.ospf_msweep_destroy(self._h)
            self._h = None

    __del__ = close

    def run(self) -> None:
        self.multi._check(self._L.ospf_msweep_run(self._h))

    def digests(self) -> np.ndarray:
        out = np.zeros((self.multi.V, 3), np.uint64)
        self.multi._check(self._L.ospf_msweep_digests(self._h, out.ctypes.data))
        return out

    def select(self, offsets: Sequence[int], nodes: Sequence[int], nh_words: int = 0):
        """ospf_msweep_select: every part selects for its own roots ->
        (metric [V, P], count [V, P], nh [V, P, W]) by node id, W = nh_words
        or the widest part's max_nh_words."""
        t, keep = select_table(offsets, nodes)
        if not nh_words:
            gi = N.ospf_sweep_info()
            for slot in range(self.multi.n):
                self._L.ospf_sweep_get_info(self._L.ospf_msweep_part(self._h, slot), C.byref(gi))
                nh_words = max(nh_words, int(gi.max_nh_words), 1)
        V, P = self.multi.V, int(t.n_prefixes)
        metric = np.zeros((V, P), np.uint32)
        count = np.zeros((V, P), np.uint32)
        nh = np.zeros((V, P, nh_words), np.uint32)
        self.multi._check(self._L.ospf_msweep_select(self._h, C.byref(t), nh_words,
                                                     metric.ctypes.data, count.ctypes.data,
                                                     nh.ctypes.data))
        return metric, count, nh

    def select_policy(self, offsets: Sequence[int], nodes: Sequence[int],
                      pref: Optional[Sequence[int]],
                      min_nexthop: Optional[Sequence[int]] = None, nh_words: int = 0,
                      want: Sequence[str] = POLICY_OUTPUTS) -> Dict[str, np.ndarray]:
        """ospf_msweep_select_policy: Sweep.select_policy on every part for its
        own roots -> the same arrays by node id ([V, P], nh [V, P, W])."""
        t, keep = select_ptable(offsets, nodes, pref, min_nexthop)
        if not nh_words:
            gi = N.ospf_sweep_info()
            for slot in range(self.multi.n):
                self._L.ospf_sweep_get_info(self._L.ospf_msweep_part(self._h, slot), C.byref(gi))
                nh_words = max(nh_words, int(gi.max_nh_words), 1)
        o, arrs = _policy_host_out(self.multi.V, int(t.n_prefixes), nh_words, want)
        self.multi._check(self._L.ospf_msweep_select_policy(self._h, C.byref(t), nh_words,
                                                            C.byref(o)))
        return arrs

    @property
    def gather_backend(self) -> str:
        """'rccl' (one ncclAllGather of the parts' digests) or 'peer'."""
        return "rccl" if self._L.ospf_msweep_gather_backend(self._h) else "peer"

    def owner(self, root: int) -> int:
        s = C.c_uint32()
        self.multi._check(self._L.ospf_msweep_owner(self._h, int(root), C.byref(s)))
        return int(s.value)

    def part_roots(self, slot: int) -> np.ndarray:
        h = self._L.ospf_msweep_part(self._h, slot)
        gi = N.ospf_sweep_info()
        self._L.ospf_sweep_get_info(h, C.byref(gi))
        r = np.zeros(max(1, gi.n_roots), np.uint32)
        self._L.ospf_sweep_roots(h, r.ctypes.data)
        return r[: gi.n_roots]
