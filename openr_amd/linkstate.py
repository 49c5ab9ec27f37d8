"""Python face of the GPU-backed LinkState mirror (libopenr_decision).

Method names follow openr/decision/LinkState.h (getSpfResult, getKthPaths,
getMetricFromAToB, linksFromNode, isNodeOverloaded, updateAdjacencyDatabase,
deleteAdjacencyDatabase); the snake_case helpers below are what the parity
tests drive.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .adjdb import AdjDbStream, change_array, changes_to_list


class LinkStateError(RuntimeError):
    pass


def parse_ucmp_text(t: str) -> Dict[str, Tuple[int, Dict[str, Tuple[str, int]]]]:
    """odl/orc UCMP text -> {node: (advertised weight, {iface: (next hop, weight)})}."""
    out = {}
    for ln in t.splitlines():
        node, w, hops = ln.split("\t")
        hp = {}
        for h in filter(None, hops.split(",")):
            iface, rest = h.split("=", 1)
            nh, hw = rest.rsplit(":", 1)
            hp[iface] = (nh, int(hw))
        out[node] = (int(w), hp)
    return out


UCMP_ALGOS = {"adj": 2, "prefix": 3}  # SP_UCMP_{ADJ,PREFIX}_WEIGHT_PROPAGATION

# odl_route_db_bin records (include/openr_decision.h)
RDB_MAGIC = 0x4244524F
RDB_HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("bytes", "<u8"),
                       ("n_nodes", "<u4"), ("n_routes", "<u4"), ("n_nhs", "<u4"),
                       ("n_labels", "<u4"), ("off_nodes", "<u8"), ("off_routes", "<u8"),
                       ("off_nhs", "<u8"), ("off_labels", "<u8"), ("off_strings", "<u8"),
                       ("str_bytes", "<u8")])
RDB_NODE = np.dtype([("name", "<u4"), ("found", "<u4"), ("first_route", "<u4"),
                     ("n_unicast", "<u4"), ("n_mpls", "<u4"), ("pad", "<u4")])
RDB_ROUTE = np.dtype([("kind", "<u4"), ("key", "<u4"), ("igp_cost", "<u4"),
                      ("has_weight", "<u4"), ("ucmp_weight", "<i8"), ("first_nh", "<u4"),
                      ("n_nh", "<u4")])
RDB_NH = np.dtype([("if_name", "<u4"), ("neighbor", "<u4"), ("metric", "<i4"),
                   ("weight", "<i4"), ("op", "<u4"), ("first_label", "<u4"),
                   ("n_labels", "<u4"), ("pad", "<u4")])
_OPS = {0: "", 1: "PHP", 2: "SWAP", 3: "PUSH", 4: "POP"}


def decode_route_db_bin(buf: bytes):
    """odl_route_db_bin buffer -> route_dbs' dict (same shape as the text)."""
    hd = np.frombuffer(buf, RDB_HEADER, 1)[0]
    if int(hd["magic"]) != RDB_MAGIC or int(hd["version"]) != 1 or int(hd["bytes"]) != len(buf):
        raise ValueError("not an odl route-db buffer")
    nodes = np.frombuffer(buf, RDB_NODE, int(hd["n_nodes"]), int(hd["off_nodes"]))
    routes = np.frombuffer(buf, RDB_ROUTE, int(hd["n_routes"]), int(hd["off_routes"]))
    nhs = np.frombuffer(buf, RDB_NH, int(hd["n_nhs"]), int(hd["off_nhs"]))
    labels = np.frombuffer(buf, "<i4", int(hd["n_labels"]), int(hd["off_labels"])).tolist()
    so = int(hd["off_strings"])
    strs = buf[so: so + int(hd["str_bytes"])]
    cache = {}

    def sget(o):
        o = int(o)
        v = cache.get(o)
        if v is None:
            v = cache[o] = strs[o: strs.index(b"\0", o)].decode()
        return v

    out = {}
    for nd in nodes:
        me = sget(nd["name"])
        if not nd["found"]:
            out[me] = None
            continue
        db = {"routes": {}}
        r0 = int(nd["first_route"])
        for r in routes[r0: r0 + int(nd["n_unicast"]) + int(nd["n_mpls"])]:
            if r["kind"] == 0:
                key = sget(r["key"])
                db["routes"][key] = (int(r["igp_cost"]),
                                     int(r["ucmp_weight"]) if r["has_weight"] else None)
                kk = ("U", key)
            else:
                kk = ("M", str(int(np.int32(np.uint32(r["key"])))))
            f0 = int(r["first_nh"])
            if r["n_nh"]:
                db[kk] = {(sget(x["if_name"]), sget(x["neighbor"]), int(x["metric"]),
                           _OPS[int(x["op"])],
                           tuple(labels[int(x["first_label"]): int(x["first_label"]) + int(x["n_labels"])]),
                           int(x["weight"]))
                          for x in nhs[f0: f0 + int(r["n_nh"])]}
        out[me] = db
    return out


def _parse_spf(t: str) -> Dict[str, Tuple[int, tuple, tuple]]:
    out = {}
    for ln in t.splitlines():
        name, metric, nh, pl = ln.split("\t")
        out[name] = (int(metric), tuple(x for x in nh.split(",") if x),
                     tuple(x for x in pl.split(";") if x))
    return out


def root_neighbor_ids(csr: Dict[str, np.ndarray], root: int) -> np.ndarray:
    """Distinct neighbours of `root` in ascending id order: the bit order of
    every next-hop mask of that root (ospf_root_neighbors)."""
    row = csr["col"][int(csr["row_ptr"][root]): int(csr["row_ptr"][root + 1])]
    return np.unique(row[row != root])


def decode_next_hops(csr: Dict[str, np.ndarray], names: Sequence[str], root, words) -> List[str]:
    """(root id or name, mask words) -> next-hop node names, ascending id."""
    rid = names.index(root) if isinstance(root, str) else int(root)
    nb = root_neighbor_ids(csr, rid)
    bits = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")
    on = np.nonzero(bits)[0]
    if on.size and int(on[-1]) >= nb.size:
        raise ValueError(f"mask bit {int(on[-1])} beyond the {nb.size} neighbours of node {rid}")
    return [names[int(nb[k])] for k in on]


def encode_next_hops(csr: Dict[str, np.ndarray], names: Sequence[str], root, hops: Sequence[str],
                     nh_words: int) -> np.ndarray:
    """Inverse of decode_next_hops: next-hop names -> nh_words mask words."""
    rid = names.index(root) if isinstance(root, str) else int(root)
    nb = root_neighbor_ids(csr, rid)
    out = np.zeros(nh_words, np.uint32)
    for h in hops:
        k = int(np.searchsorted(nb, names.index(h)))
        if k >= nb.size or int(nb[k]) != names.index(h):
            raise ValueError(f"{h} is no neighbour of node {rid}")
        out[k // 32] |= np.uint32(1 << (k % 32))
    return out


_FWDS = {"ip": 0, "sr_mpls": 1}
_ALGOS = {"ecmp": 0, "ksp2": 1, "ucmp_adj": 2, "ucmp_prefix": 3}
_TXT_OPS = {"0": "", "1": "PHP", "2": "SWAP", "3": "PUSH", "4": "POP"}


def _prefix_lines(prefixes) -> List[str]:
    """{prefix: [(node, fwd, algo, weight, prepend[, area[, min_nexthop[,
    metrics[, type]]]])]} -> the text ABI's
    "prefix\tnode:fwd:algo:weight:prepend[%pp/sp/d][!type][@area][#n],..."
    lines (metrics = (path_preference, source_preference, distance), type
    None | "bgp" | "bgpmv")"""
    lines = []
    for p, ents in prefixes.items():
        es = []
        for ent in ents:
            node, fwd, algo, weight, prepend = ent[:5]
            area = ent[5] if len(ent) > 5 else None
            mn = ent[6] if len(ent) > 6 else None
            met = ent[7] if len(ent) > 7 else None
            typ = ent[8] if len(ent) > 8 else None
            x = (f"{node}:{_FWDS[fwd]}:{_ALGOS[algo]}:{int(weight)}:"
                 f"{'' if prepend is None else int(prepend)}")
            if met is not None:
                x += "%" + "/".join(str(int(v)) for v in met)
            if typ:
                x += f"!{typ}"
            if area:
                x += f"@{area}"
            if mn is not None:
                x += f"#{int(mn)}"
            es.append(x)
        lines.append(f"{p}\t{','.join(es)}")
    return lines


def _parse_route_text(t: str, mes, with_area: bool):
    out = {me: {"routes": {}} for me in mes}
    for ln in t.splitlines():
        f = ln.split("\t")
        me, kind = f[0], f[1]
        if kind == "NONE":
            out[me] = None
        elif kind == "R":
            out[me]["routes"][f[2]] = (int(f[3]), None if f[4] == "-" else int(f[4]))
            if len(f) > 6:  # best-route selection on: (best, selected) as (node, area)
                sel = tuple(tuple(x.rsplit("@", 1)) for x in f[6].split(",") if x)
                out[me].setdefault("best", {})[f[2]] = (tuple(f[5].rsplit("@", 1)), sel)
        else:
            key, ifn, nbr, metric, op, labels, w = f[2:9]
            nh = (ifn, nbr, int(metric), _TXT_OPS[op], tuple(int(x) for x in labels.split(",") if x),
                  int(w))
            if with_area:
                nh += (f[9],)
            out[me].setdefault((kind, key), set()).add(nh)
    return out


def route_dbs_multi(areas: Sequence["LinkState"], mes: Sequence[str], prefixes,
                    node_labels: bool = True, adj_labels: bool = True, ucmp: bool = False,
                    best_route_selection: bool = False):
    """SpfSolver::buildRouteDb over several areas (odl_route_db_multi_text):
    one LinkState per area; prefix entries may carry (.., area, min_nexthop).
    Same result shape as LinkState.route_dbs(binary=False) with the next
    hop's area as a 7th tuple field."""
    L = N.decision()
    hs = (C.c_void_p * len(areas))(*[a._h for a in areas])
    lines = _prefix_lines(prefixes)
    flags = int(node_labels) | (2 if adj_labels else 0) | (4 if ucmp else 0) | \
        (8 if best_route_selection else 0)
    p = L.odl_route_db_multi_text(hs, len(areas), "\n".join(mes).encode(), len(mes),
                                  "\n".join(lines).encode(), len(lines), flags)
    if not p:
        raise LinkStateError(areas[0]._err())
    return _parse_route_text(areas[0]._take(p), mes, with_area=True)


def all_areas_select_policy(areas: Sequence["LinkState"], prefixes: Dict[str, Sequence[tuple]],
                            use_link_metric: bool = True) -> dict:
    """The reference's route selection across several areas, one LinkState
    each, for every node of the union of the areas and every prefix
    (odl_areas_select_policy; createRouteForPrefix, SpfSolver.cpp:197-458),
    selected on the device from the areas' all-sources sweeps, or by the same
    steps on the host when an area is in host mode or degraded. prefixes:
    {prefix: [(node name, area name, path_pref, source_pref, distance,
    min_nexthop_or_None), ...]}. Returns a dict: names (global id -> node name,
    the union by name bytes), area_names (the areas by name: bit i of `areas`
    and nh[i] belong to area_names[i]), metric / count / links / need / best /
    areas [G, P] u32 by global id (best: the entry's position among the kept
    entries of its prefix in (node, area) order), nh a list of [V_a, P, W_a]
    u32 by that area's node id, installed [G, P] bool, on_device."""
    L = N.decision()
    A = len(areas)
    hs = (C.c_void_p * max(1, A))(*[a._h for a in areas])
    unset = -(1 << 63)
    lines, attrs = [], []
    for ents in prefixes.values():
        f = []
        for nm, ar, pp, sp, dist, mn in ents:
            for x in (nm, ar):
                if not x or "\n" in x or "\t" in x:
                    raise ValueError("names must be non-empty, without tabs and newlines")
            f += [nm, ar]
            attrs.append((int(pp), int(sp), int(dist), unset if mn is None else int(mn)))
        lines.append("\t".join(f))
    at = np.ascontiguousarray(attrs, np.int64).reshape(-1, 4)
    args = (hs, A, "\n".join(lines).encode(), len(lines), at.ctypes.data if at.size else None,
            at.shape[0], int(use_link_metric))
    G = C.c_uint32(0)
    order = np.zeros(max(1, A), np.uint32)
    words = np.zeros(max(1, A), np.uint32)
    if L.odl_areas_select_policy(*args, C.byref(G), order.ctypes.data, words.ctypes.data,
                                 *([None] * 10)) != 0:
        raise LinkStateError(areas[0]._err())
    P, g = len(lines), int(G.value)
    out = {k: np.zeros((g, P), np.uint32)
           for k in ("metric", "count", "links", "need", "best", "areas")}
    by_name = [areas[int(i)] for i in order[:A]]
    nh = [np.zeros((a.num_nodes(), P, int(w)), np.uint32) for a, w in zip(by_name, words)]
    nhp = (C.c_void_p * max(1, A))(*[x.ctypes.data for x in nh])
    inst = np.zeros((g, P), np.uint8)
    names = C.c_void_p()
    dev = C.c_int(0)
    if L.odl_areas_select_policy(*args, C.byref(G), order.ctypes.data, words.ctypes.data,
                                 C.byref(names), *[out[k].ctypes.data for k in
                                                   ("metric", "count", "links", "need", "best",
                                                    "areas")],
                                 nhp, inst.ctypes.data, C.byref(dev)) != 0:
        raise LinkStateError(areas[0]._err())
    txt = areas[0]._take(names)
    out["names"] = txt.split("\n")[:-1] if txt else []
    out["area_names"] = [a.area for a in by_name]
    out["nh"] = nh
    out["installed"] = inst.astype(bool)
    out["on_device"] = bool(dev.value)
    return out


def _areas_lines(prefixes):
    """{prefix: [(node, area, path_pref, source_pref, distance, min_nexthop or
    None)]} -> (lines of tab-separated name pairs, [n, 4] i64 attributes)"""
    unset = -(1 << 63)
    lines, attrs = [], []
    for ents in prefixes.values():
        f = []
        for nm, ar, pp, sp, dist, mn in ents:
            for x in (nm, ar):
                if not x or "\n" in x or "\t" in x:
                    raise ValueError("names must be non-empty, without tabs and newlines")
            f += [nm, ar]
            attrs.append((int(pp), int(sp), int(dist), unset if mn is None else int(mn)))
        lines.append("\t".join(f))
    return lines, np.ascontiguousarray(attrs, np.int64).reshape(-1, 4)


class AreasTracker:
    """odl::LinkState::AreasTracker: all_areas_select_policy's selection kept
    resident (on the device: ospf_areastate_*) and only the cells an event in
    some area or a change of the attributes altered. `areas`: one LinkState per
    area (kept alive by the tracker); `prefixes` as all_areas_select_policy
    takes them."""

    def __init__(self, areas: Sequence["LinkState"], prefixes: Dict[str, Sequence[tuple]],
                 use_link_metric: bool = True):
        self._L = N.decision()
        self.areas = list(areas)
        self._by_name = sorted(self.areas, key=lambda a: a.area.encode())
        self.area_names = [a.area for a in self._by_name]
        lines, at = _areas_lines(prefixes)
        self.P = len(lines)
        self._entries = [[(e[0], e[1]) for e in ents] for ents in prefixes.values()]
        A = len(self.areas)
        hs = (C.c_void_p * max(1, A))(*[a._h for a in self.areas])
        h = C.c_void_p()
        if not self.areas or self._L.odl_areas_track(
                hs, A, "\n".join(lines).encode(), len(lines), at.ctypes.data if at.size else None,
                at.shape[0], int(use_link_metric), C.byref(h)) != 0:
            raise LinkStateError(self.areas[0]._err() if self.areas else "no areas")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.odl_areas_untrack(self._h)
        self._h = None

    __del__ = close

    def _err(self):
        return self.areas[0]._err()

    def delta(self) -> dict:
        """odl_areas_delta -> dict(changes = structured array root / prefix /
        metric / count / links / need / best / areas / installed with the NEW
        values (root: global id), nh [n, sum(words)] u32 (the areas' words one
        after the other, areas by name), words per area, rebased global ids,
        full, on_device)."""
        from .engine import ACHANGE_DTYPE, ACHANGE_OUT_DTYPE
        A = len(self.areas)
        n, m, full, dev = C.c_uint32(), C.c_uint32(), C.c_int32(), C.c_int32()
        words = np.zeros(max(1, A), np.uint32)
        pc, pn, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self._L.odl_areas_delta(self._h, C.byref(n), C.byref(m), words.ctypes.data,
                                   C.byref(full), C.byref(dev), C.byref(pc), C.byref(pn),
                                   C.byref(pr)) != 0:
            raise LinkStateError(self._err())
        try:
            def take(p, count, dtype):
                if not count:
                    return np.zeros(0, dtype)
                nbytes = count * np.dtype(dtype).itemsize
                return np.frombuffer(C.string_at(p, nbytes), dtype).copy()
            W = int(words[:A].sum())
            rec = take(pc, n.value, ACHANGE_DTYPE)
            nh = take(pn, n.value * W, np.uint32).reshape(n.value, W)
            rebased = take(pr, m.value, np.uint32)
        finally:
            for p in (pc, pn, pr):
                self._L.odl_free_buf(p)
        changes = np.zeros(rec.size, ACHANGE_OUT_DTYPE)
        for k in ACHANGE_DTYPE.names:
            changes[k] = rec[k]
        changes["installed"] = (rec["links"] > 0) & (rec["need"] <= rec["links"])
        return {"changes": changes, "nh": nh, "words": words[:A].copy(), "rebased": rebased,
                "full": bool(full.value), "on_device": bool(dev.value)}

    def tracked(self, nodes: Sequence[str]) -> dict:
        """odl_areas_tracked: the committed cells of some global nodes (names)
        -> metric / count / links / need / best / areas [n, P] u32, nh a list
        (areas by name) of [n, P, words[a]] u32 in `nodes` order, installed,
        words, area_names."""
        A, n, P = len(self.areas), len(nodes), self.P
        order = np.zeros(max(1, A), np.uint32)
        words = np.zeros(max(1, A), np.uint32)
        if self._L.odl_areas_tracked(self._h, b"", 0, order.ctypes.data, words.ctypes.data,
                                     *([None] * 8)) != 0:
            raise LinkStateError(self._err())
        out = {k: np.zeros((n, P), np.uint32)
               for k in ("metric", "count", "links", "need", "best", "areas")}
        nh = [np.zeros((n, P, int(w)), np.uint32) for w in words[:A]]
        nhp = (C.c_void_p * max(1, A))(*[x.ctypes.data for x in nh])
        inst = np.zeros((n, P), np.uint8)
        if self._L.odl_areas_tracked(self._h, "\n".join(nodes).encode(), n, order.ctypes.data,
                                     words.ctypes.data,
                                     *[out[k].ctypes.data for k in
                                       ("metric", "count", "links", "need", "best", "areas")],
                                     nhp, inst.ctypes.data) != 0:
            raise LinkStateError(self._err())
        out["nh"] = nh
        out["installed"] = inst.astype(bool)
        out["words"] = words[:A].copy()
        out["area_names"] = list(self.area_names)
        return out

    def set_policy(self, prefixes: Dict[str, Sequence[tuple]]) -> None:
        """odl_areas_set_attrs: the same (node, area) entries with new
        attributes; the next delta() reports what they changed."""
        if [[(e[0], e[1]) for e in ents] for ents in prefixes.values()] != self._entries:
            raise ValueError("set_policy: the (node, area) entries differ from the tracked table")
        _, at = _areas_lines(prefixes)
        if self._L.odl_areas_set_attrs(self._h, at.ctypes.data if at.size else None,
                                       at.shape[0]) != 0:
            raise LinkStateError(self._err())


class LinkState:
    """odl::LinkState over the MI355X SPF engine (device `device`)."""

    def __init__(self, area: str = "0", device: int = 0, stream: Optional[AdjDbStream] = None,
                 devices: Optional[Sequence[int]] = None):
        self._L = N.decision()
        self.area = area
        h = C.c_void_p()
        if devices is not None and len(devices) > 1:
            devs = np.ascontiguousarray(devices, np.int32)
            rc = self._L.odl_create_multi(area.encode(), devs.ctypes.data, devs.size, C.byref(h))
        else:
            rc = self._L.odl_create(area.encode(), device if devices is None else devices[0],
                                    C.byref(h))
        if rc != 0:
            raise LinkStateError("odl_create failed")
        self._h = h
        if stream is not None:
            self.apply(stream)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.odl_destroy(self._h)
            self._h = None

    # ------------------------------------------------------------ plumbing
    def _err(self) -> str:
        return self._L.odl_last_error(self._h).decode()

    def _take(self, p) -> str:
        if not p:
            raise LinkStateError(self._err())
        s = C.cast(p, C.c_char_p).value.decode()
        self._L.odl_free(p)
        return s

    # ------------------------------------------------------------ ingest
    def apply(self, stream: AdjDbStream, first: int = 0, count: Optional[int] = None,
              hold_up_ttl: int = 0, hold_down_ttl: int = 0):
        """updateAdjacencyDatabase per record (LinkState.cpp:584-726), with its
        hold TTLs (0: Decision's own call, Decision.cpp:756)."""
        count = stream.n_dbs - first if count is None else count
        ch = change_array(count)
        if hold_up_ttl or hold_down_ttl:
            rc = self._L.odl_apply_hold(self._h, C.addressof(stream.struct), first, count,
                                        C.addressof(ch), hold_up_ttl, hold_down_ttl)
        else:
            rc = self._L.odl_apply(self._h, C.addressof(stream.struct), first, count,
                                   C.addressof(ch))
        if rc != 0:
            raise LinkStateError(self._err())
        return changes_to_list(ch, count)

    def decrement_holds(self) -> bool:
        """LinkState::decrementHolds (LinkState.cpp:520-535): True when a hold
        expired (topology changed)."""
        rc = self._L.odl_decrement_holds(self._h)
        if rc < 0:
            raise LinkStateError(self._err())
        return bool(rc)

    decrementHolds = decrement_holds

    def has_holds(self) -> bool:
        return self._L.odl_has_holds(self._h) == 1

    hasHolds = has_holds

    updateAdjacencyDatabases = apply

    # ------------------------------------------------------------ queries
    def spf_text(self, root: str, use_link_metric: bool = True) -> str:
        return self._take(self._L.odl_spf_text(self._h, root.encode(), int(use_link_metric)))

    def spf(self, root: str, use_link_metric: bool = True):
        return _parse_spf(self.spf_text(root, use_link_metric))

    getSpfResult = spf

    def kth_paths(self, src: str, dst: str, k: int) -> List[List[str]]:
        t = self._take(self._L.odl_kth_paths_text(self._h, src.encode(), dst.encode(), k))
        return [ln.split(",") for ln in t.splitlines()]

    getKthPaths = kth_paths

    def ksp2_text(self, src: str, dsts: Sequence[str]) -> str:
        return self._take(self._L.odl_ksp2_text(self._h, src.encode(),
                                                "\n".join(dsts).encode(), len(dsts)))

    def route(self, me: str, announcers: Sequence[str], algo: str = "ecmp"):
        """Route next-hops built in C++ (odl::SpfSolver): algo 'ecmp',
        'ksp2' or 'label'. Returns a set of (ifName, metric, labels)."""
        code = {"ecmp": 0, "ksp2": 1, "label": 2}[algo]
        t = self._take(self._L.odl_route_text(self._h, me.encode(),
                                              "\n".join(announcers).encode(),
                                              len(announcers), code))
        out = set()
        for ln in t.splitlines():
            ifn, nbr, metric, op, labels = ln.split("\t")
            out.add((ifn, int(metric), tuple(int(x) for x in labels.split(",") if x)))
        return out or None

    def route_dbs(self, mes: Sequence[str], prefixes: Dict[str, Sequence],
                  node_labels: bool = True, adj_labels: bool = True, ucmp: bool = False,
                  binary: bool = True, best_route_selection: bool = False):
        """SpfSolver::buildRouteDb (odl::SpfSolver, C++) for every node in
        `mes`, over SPF results from one batched engine launch.

        prefixes: {prefix: [entry, ...]}, entry = (node, fwd, algo, weight,
        prepend) with fwd 'ip' | 'sr_mpls', algo 'ecmp' | 'ksp2' | 'ucmp_adj'
        | 'ucmp_prefix', weight 0 = unset, prepend None or a label.
        Returns {me: None | {"routes": {prefix: (igp_cost, weight|None)},
        (kind, key): set of (ifName, neighbor, metric, op, labels, weight)}}
        with kind 'U' (prefix) or 'M' (MPLS label) and op 'PHP' | 'SWAP' |
        'PUSH' | 'POP' | ''."""
        lines = _prefix_lines(prefixes)
        flags = int(node_labels) | (2 if adj_labels else 0) | (4 if ucmp else 0) | \
            (8 if best_route_selection else 0)
        if binary and not best_route_selection:  # odl_route_db_bin: records + strings, no text
            return decode_route_db_bin(self.route_db_bin_raw(mes, lines, flags))
        t = self._take(self._L.odl_route_db_text(
            self._h, "\n".join(mes).encode(), len(mes), "\n".join(lines).encode(),
            len(lines), flags))
        return _parse_route_text(t, mes, with_area=False)

    def route_db_bin_raw(self, mes: Sequence[str], prefix_lines: Sequence[str], flags: int) -> bytes:
        """odl_route_db_bin as raw bytes (prefix_lines in the text ABI's
        "prefix\tentries" form): what a C / C++ caller gets, before decoding."""
        buf, nb = C.c_void_p(), C.c_uint64()
        rc = self._L.odl_route_db_bin(self._h, "\n".join(mes).encode(), len(mes),
                                      "\n".join(prefix_lines).encode(), len(prefix_lines), flags,
                                      C.byref(buf), C.byref(nb))
        if rc != 0:
            raise LinkStateError(self._err())
        try:
            return C.string_at(buf.value, nb.value)
        finally:
            self._L.odl_free_buf(buf)

    @staticmethod
    def path_a_in_b(a: Sequence[str], b: Sequence[str]) -> bool:
        """LinkState::pathAInPathB (LinkState.h:477-492) in C++ over link keys."""
        L = N.decision()
        r = L.odl_path_a_in_b("\n".join(a).encode(), len(a), "\n".join(b).encode(), len(b))
        if r < 0:
            raise ValueError(f"malformed link key in {a} / {b}")
        return bool(r)

    def route_db(self, me: str, prefixes: Dict[str, Sequence], **kw):
        """route_dbs for one node."""
        return self.route_dbs([me], prefixes, **kw)[me]

    def ucmp(self, root: str, leaves: Dict[str, int], algo: str = "adj",
             use_link_metric: bool = True):
        """resolveUcmpWeights(getSpfResult(root), leaves, algo) (C++ over the
        GPU SPF result) -> {node: (weight, {iface: (next hop, weight)})}."""
        items = "\n".join(f"{k}\t{v}" for k, v in leaves.items())
        t = self._take(self._L.odl_ucmp_text(self._h, root.encode(), items.encode(),
                                             len(leaves), UCMP_ALGOS[algo],
                                             int(use_link_metric)))
        return parse_ucmp_text(t)

    def links(self, node: str):
        out = []
        for ln in self._take(self._L.odl_links_text(self._h, node.encode())).splitlines():
            key, m, up = ln.split("\t")
            out.append((key, int(m), up == "1"))
        return out

    linksFromNode = links

    def link_keys(self) -> List[str]:
        """Link keys of the current snapshot in link id order (ids of csr()
        and of the engine's KSP2 records)."""
        return self._take(self._L.odl_link_keys_text(self._h)).splitlines()

    def metric(self, a: str, b: str, use_link_metric: bool = True) -> Optional[int]:
        v = self._L.odl_metric_a_to_b(self._h, a.encode(), b.encode(), int(use_link_metric))
        if v == -2:
            raise LinkStateError(self._err())
        return None if v < 0 else v

    getMetricFromAToB = metric

    def is_overloaded(self, node: str) -> bool:
        return bool(self._L.odl_is_overloaded(self._h, node.encode()))

    isNodeOverloaded = is_overloaded

    @property
    def spf_runs(self) -> int:
        return int(self._L.odl_spf_runs(self._h))

    def set_incremental(self, on: bool = True) -> None:
        """Keep memoised SPF results a metric / up / overload-only update
        cannot affect (odl_set_incremental; off = the reference's behaviour)."""
        self._L.odl_set_incremental(self._h, int(on))

    def apply_kvs(self, key_vals, expired=(), my_node: Optional[str] = None):
        """Decision::processPublication's LinkState part (odl_apply_kvs):
        key_vals = [(key, compact-thrift AdjacencyDatabase bytes or None)] in
        keyVals iteration order, then expired keys. Change records as tuples
        (topology, link attributes, node label, added links)."""
        n, ne = len(key_vals), len(expired)
        keys = (C.c_char_p * max(n, 1))(*[k.encode() for k, _ in key_vals])
        bufs = [v for _, v in key_vals]
        vals = (C.c_void_p * max(n, 1))(*[(C.cast(C.c_char_p(v), C.c_void_p).value if v is not None
                                            else None) for v in bufs])
        lens = (C.c_uint64 * max(n, 1))(*[len(v) if v is not None else 0 for v in bufs])
        exp = (C.c_char_p * max(ne, 1))(*[k.encode() for k in expired])
        ch = change_array(n + ne)
        if self._L.odl_apply_kvs(self._h, n, keys, vals, lens, ne, exp,
                                 my_node.encode() if my_node is not None else None, ch) != 0:
            raise LinkStateError(self._err())
        self.decode_errors = [i for i in range(n + ne) if ch[i].decode_error]
        return changes_to_list(ch, n + ne)

    def apply_publication(self, buf: bytes, my_node: Optional[str] = None):
        """A whole compact-thrift thrift::Publication (odl_apply_publication).
        Values that fail to decode skip their own key only: their record
        indices are left in self.decode_errors, the reason in
        last_decode_error()."""
        nout = C.c_uint32(0)
        cap = 64
        me = my_node.encode() if my_node is not None else None
        while True:
            ch = change_array(cap)
            rc = self._L.odl_apply_publication(self._h, buf, len(buf), me, ch, cap, C.byref(nout))
            if rc == -2 and int(nout.value) > cap:  # ODL_E_SMALL: nothing applied
                cap = int(nout.value)
                continue
            if rc != 0:
                raise LinkStateError(self._err())
            break
        n = int(nout.value)
        self.decode_errors = [i for i in range(n) if ch[i].decode_error]
        return changes_to_list(ch, n)

    def counters(self) -> dict:
        """The path's fb303 counters (odl_get_counters): decision.spf_runs,
        spf_ms / ucmp_ms / route_build_ms as sums + sample counts (AVG =
        sum / samples), ucmp_runs, and the device errors survived."""
        c = N.odl_counters()
        self._L.odl_get_counters(self._h, C.byref(c))
        return {k: getattr(c, k) for k, _ in c._fields_}

    def set_degrade(self, on: bool = True) -> None:
        """Degrade to the host path on device errors (odl_set_degrade)."""
        self._L.odl_set_degrade(self._h, int(on))

    def last_engine_error(self) -> str:
        return (self._L.odl_last_engine_error(self._h) or b"").decode()

    def inject_engine_error(self, after: int = 1) -> None:
        """Test hook: the after-th engine call from now fails (OSPF_E_DEVICE)."""
        if self._L.odl_inject_engine_error(self._h, after) != 0:
            raise LinkStateError(self._err())

    def last_decode_error(self):
        """(message of the last value that failed to decode or "", count so far)."""
        k = C.c_uint64(0)
        msg = self._L.odl_last_decode_error(self._h, C.byref(k))
        return (msg or b"").decode(), int(k.value)

    def set_host_spf(self, on: bool = True) -> None:
        """Run every SPF / KSP2 / digest of this LinkState on the host with the
        reference's algorithm, the engine never opened (odl_set_host_spf): a
        GPU-free run of the ingest / patch / memo logic, for sanitizer builds
        and CPU tests. Off by default."""
        self._L.odl_set_host_spf(self._h, int(on))

    def incremental_stats(self) -> Dict[str, int]:
        out = (C.c_uint64 * 3)()
        self._L.odl_incremental_stats(self._h, out)
        return {"patches": int(out[0]), "kept": int(out[1]), "dropped": int(out[2])}

    @property
    def node_patches(self) -> int:
        """nodes added / removed in place (odl_node_patches)"""
        return int(self._L.odl_node_patches(self._h))

    def shard_stats(self) -> Dict[str, int]:
        """multi-device LinkState: root batches / KSP2 prefetches split across
        the device slots and their per-slot launches (odl_shard_stats)"""
        out = (C.c_uint64 * 4)()
        self._L.odl_shard_stats(self._h, out)
        return {"spf_batches": int(out[0]), "spf_launches": int(out[1]),
                "ksp2_runs": int(out[2]), "ksp2_launches": int(out[3])}

    def topology_stats(self) -> Dict[str, int]:
        """{snapshots, loads, link_patches, rows_patched}: links added /
        removed between known nodes patch the CSR and the device graph in
        place (odl_topology_stats)."""
        out = (C.c_uint64 * 4)()
        self._L.odl_topology_stats(self._h, out)
        return {"snapshots": int(out[0]), "loads": int(out[1]), "link_patches": int(out[2]),
                "rows_patched": int(out[3])}

    def num_nodes(self) -> int:
        return int(self._L.odl_num_nodes(self._h))

    def num_links(self) -> int:
        return int(self._L.odl_num_links(self._h))

    # ------------------------------------------------------------ batches
    def digests(self, roots: Sequence[str], use_link_metric: bool = True) -> np.ndarray:
        out = np.zeros((len(roots), 3), np.uint64)
        if self._L.odl_spf_digests(self._h, "\n".join(roots).encode(), len(roots),
                                   int(use_link_metric), out.ctypes.data) != 0:
            raise LinkStateError(self._err())
        return out

    def all_sources_digests(self, use_link_metric: bool = True) -> np.ndarray:
        """Digests of every node (node id order) from one all-sources sweep."""
        out = np.zeros((self.num_nodes(), 3), np.uint64)
        if self._L.odl_all_sources_digests(self._h, int(use_link_metric), out.ctypes.data) != 0:
            raise LinkStateError(self._err())
        return out

    def all_sources_select(self, prefixes: Dict[str, Sequence[str]],
                           use_link_metric: bool = True, nh_words: int = 0):
        """SpfSolver::getNextHopsWithMetric for every node and every prefix
        (odl_all_sources_select), selected on the device from the all-sources
        sweep's rows. prefixes: {prefix: announcer node names}; unknown names
        and duplicates are dropped. Returns (metric [V, P] u32, count [V, P]
        u32, nh [V, P, W] u32) by node id (node_names() order), columns in the
        dict's order; metric 0xFFFFFFFF / count 0 where the node reaches no
        announcer; decode nh with next_hop_names()."""
        lines = ["\t".join(a) for a in prefixes.values()]
        for ln in lines:
            if "\n" in ln:
                raise ValueError("node names must not contain newlines")
        txt = "\n".join(lines).encode()
        need = C.c_uint32(0)
        if self._L.odl_all_sources_select(self._h, txt, len(lines), int(use_link_metric), 0,
                                          C.byref(need), None, None, None) != 0:
            raise LinkStateError(self._err())
        V, P, W = self.num_nodes(), len(lines), nh_words or int(need.value)
        metric = np.zeros((V, P), np.uint32)
        count = np.zeros((V, P), np.uint32)
        nh = np.zeros((V, P, W), np.uint32)
        if self._L.odl_all_sources_select(self._h, txt, P, int(use_link_metric), W, None,
                                          metric.ctypes.data, count.ctypes.data,
                                          nh.ctypes.data) != 0:
            raise LinkStateError(self._err())
        return metric, count, nh

    def all_sources_select_policy(self, prefixes: Dict[str, Sequence[tuple]],
                                  use_link_metric: bool = True, nh_words: int = 0) -> dict:
        """The reference's route selection for every node and every prefix
        (odl_all_sources_select_policy; createRouteForPrefix, SpfSolver.cpp:
        197-458): unreached announcers dropped, the best (path preference,
        source preference, distance) class kept, drained announcers filtered
        unless all are, then the minimum. prefixes: {prefix: [(name,
        path_pref, source_pref, distance, min_nexthop_or_None), ...]}; for a
        name given twice the first counts, unknown names are dropped. Returns
        a dict by node id (node_names() order), columns in the dict's order:
        metric / count / links / need / best [V, P] u32, nh [V, P, W] u32 and
        installed [V, P] bool (links > 0 and need <= links)."""
        lines, at = self._policy_lines(prefixes)
        txt = "\n".join(lines).encode()
        args = (self._h, txt, len(lines), at.ctypes.data if at.size else None, at.shape[0],
                int(use_link_metric))
        need = C.c_uint32(0)
        if self._L.odl_all_sources_select_policy(*args, 0, C.byref(need), None, None, None, None,
                                                 None, None, None) != 0:
            raise LinkStateError(self._err())
        V, P, W = self.num_nodes(), len(lines), nh_words or int(need.value)
        out = {k: np.zeros((V, P), np.uint32) for k in ("metric", "count", "links", "need", "best")}
        out["nh"] = np.zeros((V, P, W), np.uint32)
        inst = np.zeros((V, P), np.uint8)
        if self._L.odl_all_sources_select_policy(
                *args, W, None, out["metric"].ctypes.data, out["count"].ctypes.data,
                out["nh"].ctypes.data, out["links"].ctypes.data, out["need"].ctypes.data,
                out["best"].ctypes.data, inst.ctypes.data) != 0:
            raise LinkStateError(self._err())
        out["installed"] = inst.astype(bool)
        return out

    def all_sources_select_srmpls(self, prefixes: Dict[str, Sequence[tuple]],
                                  use_link_metric: bool = True, nh_words: int = 0) -> dict:
        """all_sources_select_policy for prefixes forwarded as SR_MPLS
        (odl_all_sources_select_srmpls; selectBestPathsSpf with perDestination,
        SpfSolver.cpp:772-845): the next hops are kept per destination.
        prefixes: {prefix: [(name, path_pref, source_pref, distance,
        min_nexthop_or_None, has_prepend), ...]}; a node whose own entry has a
        prepend label routes to the other announcers. Returns a dict by node id:
        metric / count / links / need / best [V, P] u32, installed [V, P] bool,
        entry_offsets [P + 1] (the kept entries of each prefix: unknown names
        dropped, ascending by node id; A = entry_offsets[-1]), dst_links [V, A]
        u32 and dst_nh [V, A, W] u32 per kept entry. links counts (link,
        destination) pairs."""
        lines, at4 = self._policy_lines({k: [a[:5] for a in v] for k, v in prefixes.items()})
        flag = np.array([int(bool(a[5])) for v in prefixes.values() for a in v], np.int64)
        at = np.ascontiguousarray(np.concatenate([at4, flag.reshape(-1, 1)], axis=1), np.int64)
        txt = "\n".join(lines).encode()
        args = (self._h, txt, len(lines), at.ctypes.data if at.size else None, at.shape[0],
                int(use_link_metric))
        need = C.c_uint32(0)
        if self._L.odl_all_sources_select_srmpls(*args, 0, C.byref(need), *[None] * 9) != 0:
            raise LinkStateError(self._err())
        V, P, W = self.num_nodes(), len(lines), nh_words or int(need.value)
        cap = at.shape[0]  # the kept entries are at most the names given
        out = {k: np.zeros((V, P), np.uint32) for k in ("metric", "count", "links", "need", "best")}
        off = np.zeros(P + 1, np.uint32)
        dl = np.zeros(V * cap, np.uint32)
        dn = np.zeros(V * cap * W, np.uint32)
        inst = np.zeros((V, P), np.uint8)
        if self._L.odl_all_sources_select_srmpls(
                *args, W, None, off.ctypes.data, out["metric"].ctypes.data,
                out["count"].ctypes.data, out["links"].ctypes.data, out["need"].ctypes.data,
                out["best"].ctypes.data, dl.ctypes.data, dn.ctypes.data, inst.ctypes.data) != 0:
            raise LinkStateError(self._err())
        A = int(off[-1])
        out["entry_offsets"] = off
        out["dst_links"] = dl[:V * A].reshape(V, A)
        out["dst_nh"] = dn[:V * A * W].reshape(V, A, W)
        out["installed"] = inst.astype(bool)
        return out

    @staticmethod
    def _policy_lines(prefixes: Dict[str, Sequence[tuple]]):
        """{prefix: [(name, path_pref, source_pref, distance, min_nexthop_or_None)]}
        -> (tab-separated name lines, attribute sets [n, 4] i64)"""
        unset = -(1 << 63)
        lines, attrs = [], []
        for ann in prefixes.values():
            for nm, pp, sp, dist, mn in ann:
                if not nm or "\n" in nm or "\t" in nm:
                    raise ValueError("node names must be non-empty, without tabs and newlines")
                attrs.append((int(pp), int(sp), int(dist), unset if mn is None else int(mn)))
            lines.append("\t".join(a[0] for a in ann))
        return lines, np.ascontiguousarray(attrs, np.int64).reshape(-1, 4)

    def track_select_policy(self, prefixes: Dict[str, Sequence[tuple]],
                            use_link_metric: bool = True) -> None:
        """odl_track_select_policy: bind the LinkState to a prefix table with
        attributes (all_sources_select_policy's form) and store the policy
        selection as the baseline of policy_delta, on the device."""
        lines, at = self._policy_lines(prefixes)
        if self._L.odl_track_select_policy(self._h, "\n".join(lines).encode(), len(lines),
                                           at.ctypes.data if at.size else None, at.shape[0],
                                           int(use_link_metric)) != 0:
            raise LinkStateError(self._err())
        self._tracked_prefixes = len(lines)

    def set_tracked_policy(self, prefixes: Dict[str, Sequence[tuple]]) -> None:
        """odl_set_tracked_attrs: new attributes for the tracked table (the
        same announcer names per prefix, in track_select_policy's order); the
        next policy_delta reports what they changed."""
        _, at = self._policy_lines(prefixes)
        if self._L.odl_set_tracked_attrs(self._h, at.ctypes.data if at.size else None,
                                         at.shape[0]) != 0:
            raise LinkStateError(self._err())

    def policy_delta(self) -> dict:
        """odl_policy_delta: select_delta over the policy selection -> dict(
        changes = structured array root / prefix / metric / count / links /
        need / best / installed with the NEW values, nh [n, W] u32, rebased
        node ids, full)."""
        n, m, W, full = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        pc, pn, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self._L.odl_policy_delta(self._h, C.byref(n), C.byref(m), C.byref(W), C.byref(full),
                                    C.byref(pc), C.byref(pn), C.byref(pr)) != 0:
            raise LinkStateError(self._err())
        try:
            def take(p, count, dtype):
                if not count:
                    return np.zeros(0, dtype)
                nbytes = count * np.dtype(dtype).itemsize
                return np.frombuffer(C.string_at(p, nbytes), dtype).copy()
            from .engine import PCHANGE_DTYPE
            changes = take(pc, n.value, PCHANGE_DTYPE)
            nh = take(pn, n.value * W.value, np.uint32).reshape(n.value, W.value)
            rebased = take(pr, m.value, np.uint32)
        finally:
            for p in (pc, pn, pr):
                self._L.odl_free_buf(p)
        return {"changes": changes, "nh": nh, "rebased": rebased, "full": bool(full.value)}

    def policy_tracked(self, nodes: Sequence[str], nh_words: int = 0) -> dict:
        """odl_policy_tracked: the baseline of some nodes (names) in
        all_sources_select_policy's layout (rows = nodes)."""
        if not hasattr(self, "_tracked_prefixes"):
            raise LinkStateError("policy_tracked: no tracked table (track_select_policy)")
        P, W = self._tracked_prefixes, nh_words
        if not W:
            need = C.c_uint32(0)
            if self._L.odl_all_sources_select(self._h, b"", 0, 1, 0, C.byref(need), None, None,
                                              None) != 0:
                raise LinkStateError(self._err())
            W = int(need.value)
        n = len(nodes)
        out = {k: np.zeros((n, P), np.uint32) for k in ("metric", "count", "links", "need", "best")}
        out["nh"] = np.zeros((n, P, W), np.uint32)
        inst = np.zeros((n, P), np.uint8)
        if self._L.odl_policy_tracked(self._h, "\n".join(nodes).encode(), n, W,
                                      out["metric"].ctypes.data, out["count"].ctypes.data,
                                      out["nh"].ctypes.data, out["links"].ctypes.data,
                                      out["need"].ctypes.data, out["best"].ctypes.data,
                                      inst.ctypes.data) != 0:
            raise LinkStateError(self._err())
        out["installed"] = inst.astype(bool)
        return out

    @staticmethod
    def _prefix_lines(prefixes: Dict[str, Sequence[str]]) -> List[str]:
        lines = ["\t".join(a) for a in prefixes.values()]
        for ln in lines:
            if "\n" in ln:
                raise ValueError("node names must not contain newlines")
        return lines

    def track_select(self, prefixes: Dict[str, Sequence[str]], use_link_metric: bool = True) -> None:
        """odl_track_select: bind the LinkState to a prefix table (as
        all_sources_select takes it) and store the current selection as the
        baseline of select_delta, on the device."""
        lines = self._prefix_lines(prefixes)
        if self._L.odl_track_select(self._h, "\n".join(lines).encode(), len(lines),
                                    int(use_link_metric)) != 0:
            raise LinkStateError(self._err())
        self._tracked_prefixes = len(lines)

    def select_delta(self) -> dict:
        """odl_select_delta: what changed in the tracked selection since the
        last call (DecisionRouteDb::calculateUpdate) -> dict(changes =
        structured array root / prefix / metric / count by node id with the
        NEW values, nh = [n, W] u32 next-hop words, rebased = node ids whose
        neighbour list changed (read them with select_tracked), full = True
        when the node names changed and everything is to be read anew)."""
        n, m, W, full = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        pc, pn, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self._L.odl_select_delta(self._h, C.byref(n), C.byref(m), C.byref(W), C.byref(full),
                                    C.byref(pc), C.byref(pn), C.byref(pr)) != 0:
            raise LinkStateError(self._err())
        try:
            def take(p, count, dtype):
                if not count:
                    return np.zeros(0, dtype)
                nbytes = count * np.dtype(dtype).itemsize
                return np.frombuffer(C.string_at(p, nbytes), dtype).copy()
            from .engine import CHANGE_DTYPE
            changes = take(pc, n.value, CHANGE_DTYPE)
            nh = take(pn, n.value * W.value, np.uint32).reshape(n.value, W.value)
            rebased = take(pr, m.value, np.uint32)
        finally:
            for p in (pc, pn, pr):
                self._L.odl_free_buf(p)
        return {"changes": changes, "nh": nh, "rebased": rebased, "full": bool(full.value)}

    def select_tracked(self, nodes: Sequence[str], nh_words: int = 0):
        """odl_select_tracked: the baseline of some nodes (names) ->
        (metric [n, P], count [n, P], nh [n, P, W])."""
        if not hasattr(self, "_tracked_prefixes"):
            raise LinkStateError("select_tracked: no tracked table (track_select)")
        P = self._tracked_prefixes
        W = nh_words
        if not W:
            need = C.c_uint32(0)
            if self._L.odl_all_sources_select(self._h, b"", 0, 1, 0, C.byref(need), None, None,
                                              None) != 0:
                raise LinkStateError(self._err())
            W = int(need.value)
        metric = np.zeros((len(nodes), P), np.uint32)
        count = np.zeros((len(nodes), P), np.uint32)
        nh = np.zeros((len(nodes), P, W), np.uint32)
        if self._L.odl_select_tracked(self._h, "\n".join(nodes).encode(), len(nodes), W,
                                      metric.ctypes.data, count.ctypes.data, nh.ctypes.data) != 0:
            raise LinkStateError(self._err())
        return metric, count, nh

    def _leaf_weights(self, weights) -> np.ndarray:
        lists = list(weights.values()) if isinstance(weights, dict) else list(weights)
        if len(lists) != getattr(self, "_tracked_prefixes", -1):
            raise LinkStateError("UCMP: one weight list per tracked prefix (track_select)")
        return np.ascontiguousarray([int(w) for ws in lists for w in ws], np.int64)

    def all_sources_ucmp(self, weights, algo: str = "prefix"):
        """odl_all_sources_ucmp: getNodeUcmpResult -> resolveUcmpWeights for
        every node and every prefix of the tracked table, on the device over
        the resident selection. weights: {prefix: [weight per announcer name]}
        (or a list of lists) parallel to track_select's prefixes; algo 'adj' |
        'prefix'. Returns (weight [V, P] i64, status [V, P] u8) by node id:
        status 0 OK, 1 no announcer reached, 2 a zero-weight announcer among the
        min-cost ones, 3 overflow. self.ucmp_info = dict(rounds, device,
        engine_ms) of the call. The tracked selection must be current
        (track_select / select_delta since the last change)."""
        lw = self._leaf_weights(weights)
        V, P = self.num_nodes(), self._tracked_prefixes
        weight = np.zeros((V, P), np.int64)
        status = np.zeros((V, P), np.uint8)
        rounds, dev, ms = C.c_uint32(), C.c_int32(), C.c_double()
        if self._L.odl_all_sources_ucmp(self._h, UCMP_ALGOS[algo], lw.ctypes.data if lw.size else None,
                                        lw.size, weight.ctypes.data, status.ctypes.data,
                                        C.byref(rounds), C.byref(dev), C.byref(ms)) != 0:
            raise LinkStateError(self._err())
        self.ucmp_info = dict(rounds=int(rounds.value), device=bool(dev.value), engine_ms=float(ms.value))
        return weight, status

    def _ucmp_view(self, call, n: int):
        P = self._tracked_prefixes
        weight = np.zeros((n, P), np.int64)
        status = np.zeros((n, P), np.uint8)
        off = np.zeros(n * P + 1, np.uint64)
        pw, nw = C.c_void_p(), C.c_uint64()
        if call(weight.ctypes.data, status.ctypes.data, off.ctypes.data, C.byref(pw), C.byref(nw)) != 0:
            raise LinkStateError(self._err())
        try:
            wt = (np.frombuffer(C.string_at(pw, nw.value * 8), np.int64).copy() if nw.value
                  else np.zeros(0, np.int64))
        finally:
            self._L.odl_free_buf(pw)
        return weight, status, off, wt

    def ucmp_tracked(self, nodes: Sequence[str]):
        """odl_ucmp_tracked: the per-link view of some nodes (names) from the
        last all_sources_ucmp -> (weight [n, P], status [n, P], off [n * P + 1],
        wt): entry (i, p)'s next-hop weights are wt[off[i * P + p] : off[i * P +
        p + 1]], one per selected next hop in the node's distinct-neighbour
        order (next_hop_names of select_tracked's mask), divided by their gcd."""
        txt = "\n".join(nodes).encode()
        return self._ucmp_view(lambda *o: self._L.odl_ucmp_tracked(self._h, txt, len(nodes), *o),
                               len(nodes))

    def ucmp_host_loop(self, weights, algo: str, nodes: Sequence[str]):
        """odl_ucmp_host_loop: resolveUcmpWeights(getSpfResult(node), min-cost
        announcers) per node and prefix, for some nodes -- the loop
        all_sources_ucmp degrades to; same outputs as ucmp_tracked."""
        lw = self._leaf_weights(weights)
        txt = "\n".join(nodes).encode()
        return self._ucmp_view(
            lambda *o: self._L.odl_ucmp_host_loop(self._h, UCMP_ALGOS[algo],
                                                  lw.ctypes.data if lw.size else None, lw.size, txt,
                                                  len(nodes), *o), len(nodes))

    def next_hop_names(self, root, words, csr: Optional[Dict[str, np.ndarray]] = None,
                       names: Optional[Sequence[str]] = None) -> List[str]:
        """Names of the next hops in one (root, prefix) mask of
        all_sources_select: bit k of `words` = the root's k-th distinct
        neighbour in ascending id order. root: node id or name; csr / names:
        csr() / node_names() when the caller already holds them."""
        csr = self.csr() if csr is None else csr
        names = self.node_names() if names is None else names
        return decode_next_hops(csr, names, root, words)

    def prefetch_all(self, use_link_metric: bool = True) -> None:
        if self._L.odl_all_sources_prefetch(self._h, int(use_link_metric)) != 0:
            raise LinkStateError(self._err())

    def sweep_stats(self) -> Dict[str, int]:
        out = (C.c_uint64 * 5)()
        self._L.odl_sweep_stats(self._h, out)
        return {"sweeps": int(out[0]), "rows_copied": int(out[1]),
                "mode": N.SWEEP_MODE_NAMES.get(int(out[2]), str(out[2])),
                "devices": int(out[3]), "hip_graph": int(out[4])}

    def prefetch(self, roots: Sequence[str], use_link_metric: bool = True) -> None:
        if self._L.odl_spf_prefetch(self._h, "\n".join(roots).encode(), len(roots),
                                    int(use_link_metric)) != 0:
            raise LinkStateError(self._err())

    # ------------------------------------------------------------ snapshot
    def csr(self) -> Dict[str, np.ndarray]:
        V, E = C.c_uint32(), C.c_uint32()
        if self._L.odl_csr_size(self._h, C.byref(V), C.byref(E)) != 0:
            raise LinkStateError(self._err())
        V, E = V.value, E.value
        a = dict(row_ptr=np.zeros(V + 1, np.uint32), col=np.zeros(E, np.uint32),
                 metric=np.zeros(E, np.uint32), link_id=np.zeros(E, np.uint32),
                 twin=np.zeros(E, np.uint32), edge_up=np.zeros(E, np.uint8),
                 no_transit=np.zeros(V, np.uint8), link_rank=np.zeros(E, np.uint32))
        ptrs = [a[k].ctypes.data if a[k].size else None for k in
                ("row_ptr", "col", "metric", "link_id", "twin", "edge_up", "no_transit",
                 "link_rank")]
        if self._L.odl_csr_export(self._h, *ptrs) != 0:
            raise LinkStateError(self._err())
        return a

    def node_names(self) -> List[str]:
        n = self.num_nodes()
        return [self._L.odl_node_name(self._h, i).decode() for i in range(n)]

    def node_id(self, name: str) -> int:
        return int(self._L.odl_node_id(self._h, name.encode()))
