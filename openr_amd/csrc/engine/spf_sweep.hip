// spf_sweep.hip — all-sources sweeps (include/openr_spf.h, "sweeps").
//
// A sweep is runSpf (openr/decision/LinkState.cpp:836-911) for every node of
// the graph, or for one part of a root partition: the reference's
// all-sources use is Decision::getDecisionRouteDb(node) per node
// (openr/decision/Decision.cpp:309) and `breeze decision routes --nodes all`
// (openr/py/openr/cli/commands/decision.py:26-48). The sweep owns what a
// caller would otherwise orchestrate: the path (derive / weighted cover /
// weighted derive / batch), root order and width classes, the row buffers,
// one HIP stream per concurrent launch and the HIP graph a run replays.
//
// This file: the sweep's plumbing (streams, events, rows), the root partition
// and the leaf set, run and capture, and the ospf_sweep_* ABI. What a sweep
// launches is planned in sweep_units.hip (batch, LDS), sweep_plan_derive.hip
// and sweep_plan_weighted.hip; the multi-device context is spf_multi.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "sweep_impl.h"

using namespace ospf_int;
using namespace ospf_int::sweep;

namespace {

__global__ void gather_digest_kernel(const ospf_digest* __restrict__ src,
                                     const uint32_t* __restrict__ idx, uint32_t n,
                                     ospf_digest* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}

// Empty dispatch queued before each launch unit by ospf_sweep_profile: in a
// rocprofv3 kernel trace or counter collection its dispatches cut the
// profile phase into units (scripts/sweep_unit_stats.py).
__global__ void sweep_unit_mark_kernel(uint32_t unit) { (void)unit; }

}  // namespace

// ---------------------------------------------------------------- host graph facts
std::vector<uint32_t> ospf_int::sweep::closure(const Facts& f, const std::vector<uint32_t>& roots) {
  std::vector<uint8_t> mark(f.V, 0);
  // (serial: on host threads the marks of shared neighbours -- a pod's
  // fabric switches, marked by all its racks -- contended, 0.8 -> 2.4 ms)
  for (uint32_t r : roots) {
    mark[r] = 1;
    for (uint32_t k = (*f.dn_off)[r]; k < (*f.dn_off)[r + 1]; ++k) mark[(*f.dn)[k]] = 1;
  }
  std::vector<uint32_t> out;
  for (uint32_t v = 0; v < f.V; ++v)
    if (mark[v]) out.push_back(v);
  return out;
}

namespace {

// [lo, hi) of part p's contiguous share of m items (sizes differ by <= 1)
std::pair<size_t, size_t> part_slice(size_t m, uint32_t parts, uint32_t p) {
  const size_t q = m / parts, r = m % parts;
  const size_t lo = p * q + std::min<size_t>(p, r);
  return {lo, lo + q + (p < r ? 1 : 0)};
}

// The roots of part p: every width class ordered by the node's largest
// neighbour (stable in id order), cut into contiguous slices. On a fabric
// the racks and fabric switches of a pod share their largest neighbour (a
// fabric switch / a rack of the same pod), the spines of a plane too (the
// plane's fabric switch in the last pod by name), so parts are pod and plane
// blocks and a part's closure adds little. Returns the class-major order.
std::vector<uint32_t> partition(const Facts& f, uint32_t parts, uint32_t p) {
  std::vector<uint32_t> all(f.V);
  std::iota(all.begin(), all.end(), 0u);
  if (parts <= 1) return all;
  std::vector<uint32_t> out;
  for (uint32_t cap : classes_by(all, [&](uint32_t v) { return f.cap(v); })) {
    std::vector<uint32_t> cls;
    for (uint32_t v = 0; v < f.V; ++v)
      if (f.cap(v) == cap) cls.push_back(v);
    locality_order(cls, [&](uint32_t v) { return f.last(v); });
    const auto sl = part_slice(cls.size(), parts, p);
    out.insert(out.end(), cls.begin() + sl.first, cls.begin() + sl.second);
  }
  return out;
}

}  // namespace

// Independent set of nodes with <= 32 distinct neighbours, greedy in
// (distinct neighbours, id) order: the lexicographically first maximal
// independent set of the candidates under that priority (what Luby rounds
// with a fixed priority also produce). Links of any state count.
std::vector<uint8_t> ospf_int::sweep::leaf_set(const Facts& f, uint32_t max_nbrs) {
  // candidates in (distinct neighbours, id) order: a counting sort
  std::vector<uint32_t> cnt(max_nbrs + 2, 0u);
  for (uint32_t v = 0; v < f.V; ++v)
    if (f.nbrs(v) <= max_nbrs) ++cnt[f.nbrs(v) + 1];
  for (uint32_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];
  std::vector<uint32_t> cand(cnt.back());
  for (uint32_t v = 0; v < f.V; ++v)
    if (f.nbrs(v) <= max_nbrs) cand[cnt[f.nbrs(v)]++] = v;
  std::vector<uint8_t> leaf(f.V, 0), blocked(f.V, 0);
  for (uint32_t v : cand) {
    if (blocked[v]) continue;
    leaf[v] = 1;
    for (uint32_t k = (*f.dn_off)[v]; k < (*f.dn_off)[v + 1]; ++k) blocked[(*f.dn)[k]] = 1;
  }
  return leaf;
}

// ---------------------------------------------------------------- plumbing
int ospf_int::sweep::sfail(ospf_sweep* s, int code, const std::string& m) {
  s->err = m;
  if (s->c) s->c->err = m;
  return code;
}

int ospf_int::sweep::new_stream(ospf_sweep* s) {
  hipStream_t st;
  if (!s->c->stream_pool.empty()) {
    st = s->c->stream_pool.back();
    s->c->stream_pool.pop_back();
  } else {
    SCHK(s, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  s->streams.push_back(st);
  return (int)s->streams.size() - 1;
}

int ospf_int::sweep::new_event(ospf_sweep* s) {
  hipEvent_t e;
  if (!s->c->event_pool.empty()) {
    e = s->c->event_pool.back();
    s->c->event_pool.pop_back();
  } else {
    SCHK(s, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  s->events.push_back(e);
  return (int)s->events.size() - 1;
}

// Row pitch (u32 words) of the sweep's dist / one-word next-hop rows: V
// rounded up to 32 words (128-B aligned rows) when V is a multiple of 4 (the
// 16-B store path); OSPF_SWEEP_ROW_PITCH=V keeps the packed pitch (A/B knob)
uint32_t ospf_int::sweep::row_pitch(uint32_t V) {
  if (V & 3u) return V;
  if (const char* e = knob_str(Knob::OSPF_SWEEP_ROW_PITCH))
    if (e[0] == 'V') return V;
  return (V + 31u) / 32u * 32u;
}

// CSR bytes one distance-only scan reads: neighbour ids + row offsets
uint64_t ospf_int::sweep::scan_bytes(const ospf_ctx* c, bool weighted) {
  return (uint64_t)(weighted ? 8 : 4) * c->info.n_edges + 4ull * (c->info.n_nodes + 1);
}

// owned root r's digest is slot `slot` of dig_all; its rows are (d, nh, W)
void ospf_int::sweep::own(ospf_sweep* s, uint32_t r, uint32_t slot, const uint32_t* d,
                          const uint32_t* nh, uint32_t W) {
  s->roots.push_back(r);
  s->own_slot.push_back(slot);
  s->row_dist[r] = d;
  s->row_nh[r] = nh;
  s->row_w[r] = W;
}

// ---------------------------------------------------------------- run
namespace {

// one unit of a run on its stream: its waits, the launch, its event
int launch_unit(ospf_sweep* s, ospf_sweep::Unit& u) {
  hipStream_t st = s->streams[u.stream];
  for (int e : u.wait)
    if (!(e == 0 && u.stream == 0)) SCHK(s, hipStreamWaitEvent(st, s->events[e], 0));
  const int rc = u.fn(st);
  if (rc != OSPF_OK) return sfail(s, rc, std::string(u.name) + ": " + ospf_last_error(s->c));
  if (u.record >= 0) SCHK(s, hipEventRecord(s->events[u.record], st));
  return OSPF_OK;
}

}  // namespace

// OSPF_SWEEP_EARLY_START: queue the units planned so far (the first run's
// start: after the null stream's prior work, as run_eager orders it)
int ospf_int::sweep::start_early(ospf_sweep* s) {
  if (!s->early) return OSPF_OK;
  if (!s->early_on) {
    SCHK(s, hipEventRecord(s->ev_in, nullptr));
    SCHK(s, hipStreamWaitEvent(s->streams[0], s->ev_in, 0));
    SCHK(s, hipEventRecord(s->events[0], s->streams[0]));
    s->early_on = true;
  }
  for (; s->started < s->units.size(); ++s->started) {
    const int rc = launch_unit(s, s->units[s->started]);
    if (rc) return rc;
  }
  return OSPF_OK;
}

namespace {

// queue one run's launches; the run starts when `origin` (the main stream)
// reaches this point and ends when main has waited for every other stream
int enqueue(ospf_sweep* s) {
  hipStream_t main = s->streams[0];
  // (units an early start queued are skipped, once)
  const size_t first = s->early_on ? s->started : 0;
  if (!s->early_on) SCHK(s, hipEventRecord(s->events[0], main));
  s->early_on = false;
  s->started = 0;
  for (size_t i = first; i < s->units.size(); ++i) {
    const int rc = launch_unit(s, s->units[i]);
    if (rc) return rc;
  }
  for (size_t i = 1; i < s->streams.size(); ++i) {
    SCHK(s, hipEventRecord(s->ev_done[i], s->streams[i]));
    SCHK(s, hipStreamWaitEvent(main, s->ev_done[i], 0));
  }
  return OSPF_OK;
}

int run_eager(ospf_sweep* s, hipStream_t caller) {
  if (!s->early_on) {  // (an early start ordered it after the null stream)
    SCHK(s, hipEventRecord(s->ev_in, caller));
    SCHK(s, hipStreamWaitEvent(s->streams[0], s->ev_in, 0));
  }
  const int rc = enqueue(s);
  if (rc) return rc;
  SCHK(s, hipEventRecord(s->ev_out, s->streams[0]));
  SCHK(s, hipStreamWaitEvent(caller, s->ev_out, 0));
  return OSPF_OK;
}

// The leaf launch (derive mode) timed in both block orders on the rows of
// the eager run (its own digests are zeroed by the launch, rows rewritten
// identically), the faster kept for the HIP graph and every later run.
// OSPF_LEAF_GROUP_MAJOR fixes the order; OSPF_LEAF_NO_AUTO keeps chunk-major.
int pick_leaf_order(ospf_sweep* s) {
  if (knob_set(Knob::OSPF_LEAF_GROUP_MAJOR) || knob_flag(Knob::OSPF_LEAF_NO_AUTO)) return OSPF_OK;
  ospf_sweep::Unit* u = nullptr;
  for (auto& x : s->units)
    if (x.name == "leaf") u = &x;
  if (!u || u->n_roots < 4096) return OSPF_OK;
  hipStream_t st = s->streams[u->stream];
  hipEvent_t a, b;
  SCHK(s, hipEventCreate(&a));
  SCHK(s, hipEventCreate(&b));
  float best[2] = {1e30f, 1e30f};
  int rc = OSPF_OK;
  for (int rep = 0; rep < 2 && rc == OSPF_OK; ++rep)
    for (int ord = 0; ord < 2 && rc == OSPF_OK; ++ord) {
      s->leaf_order = ord;
      if (hipEventRecord(a, st) != hipSuccess) rc = OSPF_E_DEVICE;
      if (rc == OSPF_OK) rc = u->fn(st);
      if (rc == OSPF_OK && (hipEventRecord(b, st) != hipSuccess || hipEventSynchronize(b) != hipSuccess))
        rc = OSPF_E_DEVICE;
      float t = 0;
      if (rc == OSPF_OK && hipEventElapsedTime(&t, a, b) == hipSuccess) best[ord] = std::min(best[ord], t);
    }
  hipEventDestroy(a);
  hipEventDestroy(b);
  if (rc) return sfail(s, rc, "sweep: leaf order probe: " + std::string(ospf_last_error(s->c)));
  s->leaf_order = best[1] < best[0] ? 1 : 0;
  if (knob_flag(Knob::OSPF_SWEEP_TIMING))
    fprintf(stderr, "sweep_create leaf order %s (chunk-major %.3f ms, group-major %.3f ms)\n",
            s->leaf_order ? "group-major" : "chunk-major", best[0], best[1]);
  return ospf_sync(s->c, st);
}

void release(ospf_sweep* s) {
  if (s->c) hipSetDevice(s->c->device);
  for (hipStream_t st : s->streams)
    if (st) hipStreamSynchronize(st);
  if (s->exec) hipGraphExecDestroy(s->exec);
  if (s->graph) hipGraphDestroy(s->graph);
  // blocks, streams (with their scratch) and events go to the ctx's pools
  // for the next sweep (ospf_close frees them)
  constexpr size_t kPoolCap = 160ull << 30;
  for (size_t i = 0; i < s->allocs.size(); ++i) {
    if (s->c && i < s->alloc_bytes.size() && s->c->sweep_pool_bytes + s->alloc_bytes[i] <= kPoolCap) {
      s->c->sweep_pool.emplace(s->alloc_bytes[i], s->allocs[i]);
      s->c->sweep_pool_bytes += s->alloc_bytes[i];
    } else {
      hipFree(s->allocs[i]);
    }
  }
  for (hipEvent_t e : s->events)
    if (e) (s->c ? (void)s->c->event_pool.push_back(e) : (void)hipEventDestroy(e));
  for (hipEvent_t e : s->ev_done)
    if (e) hipEventDestroy(e);
  if (s->ev_in) hipEventDestroy(s->ev_in);
  if (s->ev_out) hipEventDestroy(s->ev_out);
  if (s->sel_ev) {
    hipEventSynchronize(s->sel_ev);
    hipEventDestroy(s->sel_ev);
  }
  if (s->d_sel_tab) hipFree(s->d_sel_tab);
  s->sel_ev = nullptr;
  s->d_sel_tab = nullptr;
  s->d_sel_rows = nullptr;  // one of allocs
  s->sel_tab_words = 0;
  if (s->pol_ev) {
    hipEventSynchronize(s->pol_ev);
    hipEventDestroy(s->pol_ev);
  }
  if (s->d_pol_tab) hipFree(s->d_pol_tab);
  s->pol_ev = nullptr;
  s->d_pol_tab = nullptr;
  s->d_pol_roots = nullptr;  // one of allocs
  s->pol_tab_words = 0;
  if (s->areas_ev) {
    hipEventSynchronize(s->areas_ev);
    hipEventDestroy(s->areas_ev);
  }
  if (s->d_areas_blob) hipFree(s->d_areas_blob);
  s->areas_ev = nullptr;
  s->d_areas_blob = nullptr;
  s->d_area_rows = nullptr;  // one of allocs
  s->areas_blob_bytes = 0;
  for (hipStream_t st : s->streams) {
    if (!st) continue;
    if (s->c) {
      s->c->stream_pool.push_back(st);
    } else {
      hipStreamDestroy(st);
    }
  }
  // idempotent: a sweep released by ospf_close is released again (a no-op)
  // by its own destroy
  s->allocs.clear();
  s->alloc_bytes.clear();
  s->streams.clear();
  s->events.clear();
  s->ev_done.clear();
  s->ev_in = s->ev_out = nullptr;
  s->exec = nullptr;
  s->graph = nullptr;
}

// ---------------------------------------------------------------- select
uint32_t max_row_words(const ospf_sweep* s) {
  uint32_t mw = 0;
  for (uint32_t r : s->roots) mw = std::max(mw, s->row_w[r]);
  return mw;
}

// the table's contract (ospf_select_table): null on success, else what is wrong
const char* select_table_error(const ospf_select_table* t, uint32_t V) {
  if (!t) return "select: null table";
  const uint32_t P = t->n_prefixes;
  if (!P) return nullptr;
  if (!t->offsets) return "select: null offsets";
  for (uint32_t p = 0; p < P; ++p)
    if (t->offsets[p] > t->offsets[p + 1]) return "select: offsets not monotone";
  if (t->offsets[P] && !t->nodes) return "select: null nodes";
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t k = t->offsets[p]; k < t->offsets[p + 1]; ++k) {
      if (t->nodes[k] >= V) return "select: announcer id outside the graph";
      if (k > t->offsets[p] && t->nodes[k - 1] >= t->nodes[k])
        return "select: announcers of a prefix not strictly ascending";
    }
  return nullptr;
}

}  // namespace

const char* ospf_int::sweep::select_table_check(const ospf_select_table* t, uint32_t V) {
  return select_table_error(t, V);
}

// the owned roots' rows as a device table (s->d_sel_rows), uploaded once per sweep
int ospf_int::sweep::select_rows(ospf_sweep* s) {
  if (s->d_sel_rows) return OSPF_OK;
  const uint32_t n = (uint32_t)s->roots.size();
  std::vector<ospf_int::SelRow> h(n);  // the host row vectors, owned-roots order
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = s->roots[i];
    h[i] = ospf_int::SelRow{s->row_dist[r], s->row_nh[r], s->row_w[r], 0u};
  }
  ospf_int::SelRow* d = nullptr;
  const int rc = upload(s, &d, h);
  if (rc) return rc;
  s->d_sel_rows = d;
  return OSPF_OK;
}

// ospf_sweep_select_dev without the fault-injection hook (the host and
// multi-device calls hook once themselves)
int ospf_int::sweep::select_queue(ospf_sweep* s, const ospf_select_table* t, uint32_t nh_words, uint32_t* d_metric,
                 uint32_t* d_count, uint32_t* d_nh, void* stream) {
  if (!s->ran) return sfail(s, OSPF_E_INVAL, "sweep: select before the first run");
  if (const char* bad = select_table_error(t, s->V)) return sfail(s, OSPF_E_INVAL, bad);
  if (nh_words < max_row_words(s))
    return sfail(s, OSPF_E_INVAL, "sweep: nh_words below a root's next-hop words");
  const uint32_t n = (uint32_t)s->roots.size(), P = t->n_prefixes;
  if (!n || !P || (!d_metric && !d_count && !d_nh)) return OSPF_OK;
  SCHK(s, hipSetDevice(s->c->device));
  if (const int rc = select_rows(s)) return rc;
  // the prefix table's device copy: the buffer is the last call's, free once
  // that call's kernel is done
  const size_t A = t->offsets[P], words = (size_t)P + 1 + A;
  if (s->sel_ev) SCHK(s, hipEventSynchronize(s->sel_ev));
  if (words > s->sel_tab_words) {
    if (s->d_sel_tab) SCHK(s, hipFree(s->d_sel_tab));
    s->d_sel_tab = nullptr;
    s->sel_tab_words = 0;
    void* q = nullptr;
    if (hipMalloc(&q, words * 4) != hipSuccess) {
      (void)hipGetLastError();
      return sfail(s, OSPF_E_NOMEM, "select: hipMalloc of the prefix table");
    }
    s->d_sel_tab = (uint32_t*)q;
    s->sel_tab_words = words;
  }
  SCHK(s, hipMemcpy(s->d_sel_tab, t->offsets, ((size_t)P + 1) * 4, hipMemcpyHostToDevice));
  if (A) SCHK(s, hipMemcpy(s->d_sel_tab + P + 1, t->nodes, A * 4, hipMemcpyHostToDevice));
  if (!s->sel_ev) SCHK(s, hipEventCreateWithFlags(&s->sel_ev, hipEventDisableTiming));
  const int rc = ospf_int::select_launch(s->c, s->d_sel_rows, n, s->d_sel_tab, s->d_sel_tab + P + 1,
                                         P, nh_words, d_metric, d_count, d_nh, stream);
  if (rc) return sfail(s, rc, s->c->err);
  SCHK(s, hipEventRecord(s->sel_ev, (hipStream_t)stream));
  return OSPF_OK;
}

extern "C" {

int ospf_sweep_create(ospf_ctx* c, const ospf_sweep_opts* o, ospf_sweep** out) {
  if (!c || !o || !out) return OSPF_E_INVAL;
  *out = nullptr;
  if (ospf_int::injected(c)) return OSPF_E_DEVICE;
  if (!c->loaded) return fail(c, OSPF_E_NOGRAPH, "no graph loaded");
  if (c->mask.on) return fail(c, OSPF_E_INVAL, "sweep: links are masked (ospf_links_unmask)");
  const uint32_t parts = std::max(1u, o->n_parts);
  if (o->part >= parts) return fail(c, OSPF_E_INVAL, "sweep: part >= n_parts");
  if (o->mode > OSPF_SWEEP_WMULTI) return fail(c, OSPF_E_INVAL, "sweep: unknown mode");
  if (o->flags & ~(OSPF_HOP_COUNT | OSPF_SWEEP_DEFER | OSPF_SWEEP_EARLY_START))
    return fail(c, OSPF_E_INVAL,
                "sweep: flags = 0 or OSPF_HOP_COUNT, | OSPF_SWEEP_DEFER (| OSPF_SWEEP_EARLY_START)");
  const bool defer = (o->flags & OSPF_SWEEP_DEFER) != 0;
  if ((o->flags & OSPF_SWEEP_EARLY_START) && !defer)
    return fail(c, OSPF_E_INVAL, "sweep: OSPF_SWEEP_EARLY_START needs OSPF_SWEEP_DEFER");
  if (defer && o->hip_graph)
    return fail(c, OSPF_E_INVAL, "sweep: OSPF_SWEEP_DEFER needs hip_graph = 0 (the capture "
                                 "follows the first run)");
  const bool hop = o->flags & OSPF_HOP_COUNT;
  if (!hop && c->dist_bound >= 0xFFFFFFFFull)
    return fail(c, OSPF_E_RANGE, "u32 distance overflow possible (sum of per-node max metrics)");
  ospf_sweep* s = new (std::nothrow) ospf_sweep();
  if (!s) return OSPF_E_NOMEM;
  s->c = c;
  c->live_sweeps.push_back(s);
  c->release_sweep = [](ospf_sweep* x) {  // ospf_close: release now, detach
    release(x);
    x->c = nullptr;
  };
  s->opts = *o;
  s->early = (o->flags & OSPF_SWEEP_EARLY_START) && !knob_flag(Knob::OSPF_SWEEP_NO_EARLY);
  s->gen = c->graph_gen;
  s->V = c->info.n_nodes;
  const uint32_t V = s->V;
  s->row_dist.assign(V, nullptr);
  s->row_nh.assign(V, nullptr);
  s->row_w.assign(V, 0);
  auto bail = [&](int rc) {
    const std::string m = s->err.empty() ? std::string(ospf_last_error(c)) : s->err;
    auto& lsw = c->live_sweeps;
    lsw.erase(std::remove(lsw.begin(), lsw.end(), s), lsw.end());
    release(s);
    delete s;
    c->err = m;
    return rc;
  };
  const bool tm = knob_flag(Knob::OSPF_SWEEP_TIMING);
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!tm) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "sweep_create %s %.2f ms\n", what,
            std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
  };
  if (hipSetDevice(c->device) != hipSuccess) return bail(fail(c, OSPF_E_DEVICE, "hipSetDevice"));
  if (new_stream(s) < 0 || new_event(s) < 0) return bail(OSPF_E_DEVICE);
  if (hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming) != hipSuccess)
    return bail(fail(c, OSPF_E_DEVICE, "hipEventCreate"));
  Facts f;
  f.V = V;
  f.dn_off = &c->h_dn_off;
  f.dn = &c->h_dn;
  const std::vector<uint32_t> mine = partition(f, parts, o->part);
  // path
  const bool unit = hop || c->info.unit_metric;
  const bool derive_ok = unit && c->max_dn <= 2048 && c->depth_bound <= 123;
  // small graphs: every root's next hops in <= 4 words and the graph in LDS
  const uint32_t max_w = std::max(1u, (c->max_dn + 31) / 32);
  const bool lds_ok = unit && max_w <= 4 && ospf_lds_sweep_fits(c, o->flags & OSPF_HOP_COUNT, max_w) &&
                      !knob_flag(Knob::OSPF_SWEEP_NOLDS);
  // the cover and multi-root paths derive the next hops of roots with > 128
  // neighbours from a u16 slot table of their link metrics
  // (wderive_lanes_kernel: metrics <= 0xFFFE): decided here, not by the
  // unit's first launch. The rule is graph-wide, so it also turns away cover
  // plans whose wide roots would all have taken their next hops from the
  // seeds' Dial; AUTO then takes the weighted-derive sweep.
  const bool lanes_ok = hop || max_w <= 4 || c->info.max_metric <= 0xFFFEu;
  std::vector<uint8_t> leaf;
  bool any_leaf = false;
  uint32_t mode = o->mode;
  if (mode == OSPF_SWEEP_AUTO || mode == OSPF_SWEEP_WCOVER || mode == OSPF_SWEEP_WDERIVE ||
      mode == OSPF_SWEEP_WMULTI) {
    if (!(mode == OSPF_SWEEP_AUTO && derive_ok)) {
      leaf = leaf_set(f);
      for (uint8_t x : leaf) any_leaf |= x != 0;
    }
  }
  if (mode == OSPF_SWEEP_AUTO) {
    if (lds_ok) {
      mode = OSPF_SWEEP_LDS;
    } else if (derive_ok) {
      mode = OSPF_SWEEP_DERIVE;
    } else if (!hop && any_leaf && lanes_ok && ospf_cover_prepare(c, leaf.data()) == OSPF_OK) {
      mode = OSPF_SWEEP_WCOVER;
    } else if (any_leaf) {
      mode = OSPF_SWEEP_WDERIVE;
    } else {
      mode = OSPF_SWEEP_BATCH;
    }
  } else if (mode == OSPF_SWEEP_DERIVE && !derive_ok) {
    return bail(fail(c, OSPF_E_RANGE, "sweep: derive needs unit metric or hop count, a depth "
                                      "bound <= 123 and <= 2048 distinct neighbours per node"));
  } else if (mode == OSPF_SWEEP_LDS && !lds_ok) {
    return bail(fail(c, OSPF_E_RANGE, "sweep: lds needs unit metric or hop count, <= 128 "
                                      "distinct neighbours per node and the graph in LDS"));
  } else if (mode == OSPF_SWEEP_WCOVER) {
    if (hop) return bail(fail(c, OSPF_E_INVAL, "sweep: the cover path runs link metrics"));
    if (!lanes_ok)
      return bail(fail(c, OSPF_E_RANGE, "sweep: the cover path needs metrics <= 65534 when a "
                                        "node has more than 128 distinct neighbours"));
    const int rc = ospf_cover_prepare(c, leaf.data());
    if (rc) return bail(rc);
  } else if (mode == OSPF_SWEEP_WMULTI && !lanes_ok) {
    return bail(fail(c, OSPF_E_RANGE, "sweep: wmulti needs metrics <= 65534 when a node has "
                                      "more than 128 distinct neighbours"));
  }
  s->mode = mode;
  lap("partition + leaf set + cover prepare");
  int rc = OSPF_OK;
  switch (mode) {
    case OSPF_SWEEP_DERIVE: rc = plan_derive(s, f, mine); break;
    case OSPF_SWEEP_WCOVER: rc = plan_wcover(s, f, mine, leaf); break;
    case OSPF_SWEEP_WDERIVE: rc = plan_wderive(s, f, mine, leaf); break;
    case OSPF_SWEEP_WMULTI: rc = plan_wmulti(s, f, mine, leaf); break;
    case OSPF_SWEEP_LDS: rc = plan_lds(s, f, mine); break;
    default: rc = plan_batch(s, f, mine, !unit); break;
  }
  if (rc) return bail(rc);
  lap("plan");
  if (upload(s, &s->d_own_slot, s->own_slot)) return bail(OSPF_E_NOMEM);
  s->ev_done.assign(s->streams.size(), nullptr);
  for (size_t i = 1; i < s->streams.size(); ++i)
    if (hipEventCreateWithFlags(&s->ev_done[i], hipEventDisableTiming) != hipSuccess)
      return bail(fail(c, OSPF_E_DEVICE, "hipEventCreate"));
  lap("slots + events");
  if (defer) {  // the caller's first ospf_sweep_run is the first run
    *out = s;
    return OSPF_OK;
  }
  // one eager run: sizes every stream's scratch (nothing may allocate inside
  // a capture) and surfaces launch errors here
  const uint64_t runs0 = c->spf_runs;
  if ((rc = run_eager(s, s->streams[0]))) return bail(rc);
  if (hipStreamSynchronize(s->streams[0]) != hipSuccess)
    return bail(fail(c, OSPF_E_DEVICE, "sweep: first run failed"));
  if ((rc = ospf_sync(c, s->streams[0]))) return bail(rc);
  s->ran = true;
  if ((rc = pick_leaf_order(s))) return bail(rc);
  // the graph's seed BFS launches levels 1 .. the depth the eager run reached
  // (deterministic for this graph version; a deeper level would set error
  // bit 8 in the rows kernel) instead of the transit-depth bound (10 at
  // F100k, where the seeds' BFS ends at 4: 14 empty level launches).
  // OSPF_SWEEP_FULL_DEPTH keeps the bound.
  if (s->d_lv_maxd && !knob_flag(Knob::OSPF_SWEEP_FULL_DEPTH)) {
    uint32_t dm = 0;
    if (hipMemcpy(&dm, s->d_lv_maxd, 4, hipMemcpyDeviceToHost) != hipSuccess)
      return bail(fail(c, OSPF_E_DEVICE, "sweep: seed BFS depth readback"));
    if (dm >= 1 && dm < c->depth_bound) s->lv_cap = dm;
  }
  if (o->hip_graph) {
    hipStream_t m = s->streams[0];
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    bool ok = hipStreamBeginCapture(m, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
      const int erc = enqueue(s);
      ok = hipStreamEndCapture(m, &g) == hipSuccess && erc == OSPF_OK && g;
    }
    ok = ok && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess;
    if (ok) {
      s->graph = g;
      s->exec = ex;
    } else {
      if (ex) hipGraphExecDestroy(ex);
      if (g) hipGraphDestroy(g);
      (void)hipGetLastError();
      s->err.clear();
    }
  }
  c->spf_runs = runs0;
  *out = s;
  return OSPF_OK;
}

int ospf_sweep_destroy(ospf_sweep* s) {
  if (!s) return OSPF_E_INVAL;
  if (s->c) {
    auto& ls = s->c->live_sweeps;
    ls.erase(std::remove(ls.begin(), ls.end(), s), ls.end());
  }
  release(s);
  delete s;
  return OSPF_OK;
}

const char* ospf_sweep_last_error(const ospf_sweep* s) {
  return s ? s->err.c_str() : "null sweep";
}

int ospf_sweep_get_info(const ospf_sweep* s, ospf_sweep_info* info) {
  if (!s || !info) return OSPF_E_INVAL;
  info->mode = s->mode;
  info->n_roots = (uint32_t)s->roots.size();
  info->n_rows = s->n_rows;
  info->n_launches = (uint32_t)s->units.size();
  info->hip_graph = s->exec ? 1u : 0u;
  uint32_t mw = 0;
  for (uint32_t r : s->roots) mw = std::max(mw, s->row_w[r]);
  info->max_nh_words = mw;
  info->device_bytes = s->device_bytes;
  info->step_compulsory_bytes = s->step_comp;
  info->step_traversed_edges = s->trav_edges;
  return OSPF_OK;
}

int ospf_sweep_roots(const ospf_sweep* s, uint32_t* roots) {
  if (!s || (!roots && !s->roots.empty())) return OSPF_E_INVAL;
  std::copy(s->roots.begin(), s->roots.end(), roots);
  return OSPF_OK;
}

int ospf_sweep_run(ospf_sweep* s, void* stream) {
  if (!s) return OSPF_E_INVAL;
  ospf_ctx* c = s->c;
  if (ospf_int::injected(c)) return sfail(s, OSPF_E_DEVICE, c->err);
  if (c->graph_gen != s->gen || c->mask.on)
    return sfail(s, OSPF_E_NOGRAPH, "sweep: the graph changed since the sweep was created");
  SCHK(s, hipSetDevice(c->device));
  const uint64_t runs0 = c->spf_runs;
  if (s->exec) {
    SCHK(s, hipGraphLaunch(s->exec, (hipStream_t)stream));
  } else {
    const int rc = run_eager(s, (hipStream_t)stream);
    if (rc) return rc;
  }
  s->ran = true;
  c->spf_runs = runs0 + s->roots.size();
  return OSPF_OK;
}

int ospf_sweep_digests(ospf_sweep* s, ospf_digest* d_out, void* stream) {
  if (!s || (!d_out && !s->roots.empty())) return OSPF_E_INVAL;
  const uint32_t n = (uint32_t)s->roots.size();
  if (!n) return OSPF_OK;
  // a deferred sweep (OSPF_SWEEP_DEFER) has no rows or digests before its run
  if (!s->ran) return sfail(s, OSPF_E_INVAL, "sweep: digests before the first run");
  SCHK(s, hipSetDevice(s->c->device));
  hipLaunchKernelGGL(gather_digest_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, s->dig_all, s->d_own_slot, n, d_out);
  SCHK(s, hipGetLastError());
  return OSPF_OK;
}

int ospf_sweep_digests_host(ospf_sweep* s, ospf_digest* out) {
  if (!s || (!out && !s->roots.empty())) return OSPF_E_INVAL;
  const size_t n = s->roots.size();
  if (!n) return OSPF_OK;
  SCHK(s, hipSetDevice(s->c->device));
  ospf_digest* d = nullptr;
  SCHK(s, hipMalloc(&d, n * sizeof(ospf_digest)));
  int rc = ospf_sweep_digests(s, d, nullptr);
  hipError_t e = hipSuccess;
  if (rc == OSPF_OK) e = hipMemcpy(out, d, n * sizeof(ospf_digest), hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return sfail(s, OSPF_E_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
  return rc;
}

int ospf_sweep_poison(ospf_sweep* s, void* stream) {
  if (!s) return OSPF_E_INVAL;
  SCHK(s, hipSetDevice(s->c->device));
  // a kernel, not hipMemsetAsync: see ospf::zero_async
  auto fill = [&](void* p, size_t words) {
    return ospf::zero_by_memset() ? hipMemsetAsync(p, 0xFF, words * 4u, (hipStream_t)stream)
                                  : ospf::launch_fill32((uint32_t*)p, words, 0xFFFFFFFFu,
                                                        (hipStream_t)stream);
  };
  SCHK(s, fill(s->dig_all, (size_t)std::max(1u, s->n_dig) * 6u));
  for (auto& a : s->dig_aux) SCHK(s, fill(a.first, std::max<size_t>(1, a.second) * 6u));
  return OSPF_OK;
}

int ospf_sweep_graph_memsets(const ospf_sweep* s, uint32_t* n_memset, uint32_t* n_dead,
                             uint32_t* n_own) {
  if (!s || !n_memset || !n_dead || !n_own) return OSPF_E_INVAL;
  *n_memset = *n_dead = *n_own = 0;
  if (!s->graph) return OSPF_OK;
  size_t nn = 0;
  if (hipGraphGetNodes(s->graph, nullptr, &nn) != hipSuccess) return OSPF_E_DEVICE;
  std::vector<hipGraphNode_t> nodes(nn);
  if (nn && hipGraphGetNodes(s->graph, nodes.data(), &nn) != hipSuccess) return OSPF_E_DEVICE;
  for (hipGraphNode_t g : nodes) {
    hipGraphNodeType ty;
    if (hipGraphNodeGetType(g, &ty) != hipSuccess) return OSPF_E_DEVICE;
    if (ty != hipGraphNodeTypeMemset) continue;
    hipMemsetParams p{};
    if (hipGraphMemsetNodeGetParams(g, &p) != hipSuccess) return OSPF_E_DEVICE;
    ++*n_memset;
    const char* dst = static_cast<const char*>(p.dst);
    const size_t bytes = (size_t)p.elementSize * p.width * std::max<size_t>(1, p.height);
    // live allocation around [dst, dst + bytes)?
    hipDeviceptr_t base = nullptr;
    size_t sz = 0;
    if (hipMemGetAddressRange(&base, &sz, (hipDeviceptr_t)dst) != hipSuccess ||
        dst + bytes > static_cast<const char*>(base) + sz) {
      ++*n_dead;
      (void)hipGetLastError();
    }
    for (size_t i = 0; i < s->allocs.size() && i < s->alloc_bytes.size(); ++i) {
      const char* a = static_cast<const char*>(s->allocs[i]);
      if (dst >= a && dst + bytes <= a + s->alloc_bytes[i]) {
        ++*n_own;
        break;
      }
    }
  }
  return OSPF_OK;
}

int ospf_sweep_row(const ospf_sweep* s, uint32_t root, const uint32_t** d_dist,
                   const uint32_t** d_nh, uint32_t* nh_words) {
  if (!s || root >= s->V || !s->ran) return OSPF_E_INVAL;  // no rows before the first run
  if (!s->row_dist[root]) return OSPF_E_RANGE;
  if (d_dist) *d_dist = s->row_dist[root];
  if (d_nh) *d_nh = s->row_nh[root];
  if (nh_words) *nh_words = s->row_w[root];
  return OSPF_OK;
}

int ospf_sweep_copy_rows(ospf_sweep* s, const uint32_t* roots, uint32_t n, uint32_t nh_words,
                         uint32_t* dist_out, uint32_t* nh_out) {
  if (!s || (n && !roots)) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  if (!s->ran) return sfail(s, OSPF_E_INVAL, "sweep: rows before the first run");
  const uint32_t V = s->V;
  for (uint32_t i = 0; i < n; ++i) {
    if (roots[i] >= V || !s->row_dist[roots[i]])
      return sfail(s, OSPF_E_RANGE, "sweep: root " + std::to_string(roots[i]) + " not owned");
    if (nh_out && s->row_w[roots[i]] > nh_words)
      return sfail(s, OSPF_E_INVAL, "sweep: nh_words below a root's next-hop words");
  }
  SCHK(s, hipSetDevice(s->c->device));
  SCHK(s, hipDeviceSynchronize());
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i], W = s->row_w[r];
    if (dist_out)
      SCHK(s, hipMemcpy(dist_out + (size_t)i * V, s->row_dist[r], (size_t)V * 4,
                        hipMemcpyDeviceToHost));
    if (nh_out) {
      uint32_t* dst = nh_out + (size_t)i * V * nh_words;
      if (W == nh_words) {
        SCHK(s, hipMemcpy(dst, s->row_nh[r], (size_t)V * W * 4, hipMemcpyDeviceToHost));
      } else {
        std::memset(dst, 0, (size_t)V * nh_words * 4);
        SCHK(s, hipMemcpy2D(dst, (size_t)nh_words * 4, s->row_nh[r], (size_t)W * 4, (size_t)W * 4,
                            V, hipMemcpyDeviceToHost));
      }
    }
  }
  return OSPF_OK;
}

int ospf_sweep_select_dev(ospf_sweep* s, const ospf_select_table* t, uint32_t nh_words,
                          uint32_t* d_metric, uint32_t* d_count, uint32_t* d_nh, void* stream) {
  if (!s || !t) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  return select_queue(s, t, nh_words, d_metric, d_count, d_nh, stream);
}

int ospf_sweep_select(ospf_sweep* s, const ospf_select_table* t, uint32_t nh_words,
                      uint32_t* metric, uint32_t* count, uint32_t* nh) {
  if (!s || !t) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  const size_t cells = s->roots.size() * (size_t)t->n_prefixes;
  SelectOut d;
  if (cells && s->ran) {
    SCHK(s, hipSetDevice(s->c->device));
    SCHK(s, hipDeviceSynchronize());  // the rows, whichever streams ran the sweep
    if (!d.alloc(cells, std::max(1u, nh_words), metric, count, nh)) {
      (void)hipGetLastError();
      return sfail(s, OSPF_E_NOMEM, "select: hipMalloc of the outputs");
    }
  }
  const int rc = select_queue(s, t, nh_words, d.m, d.k, d.nh, nullptr);
  if (rc || !cells) return rc;
  if (d.m) SCHK(s, hipMemcpy(metric, d.m, cells * 4, hipMemcpyDeviceToHost));
  if (d.k) SCHK(s, hipMemcpy(count, d.k, cells * 4, hipMemcpyDeviceToHost));
  if (d.nh) SCHK(s, hipMemcpy(nh, d.nh, cells * nh_words * 4, hipMemcpyDeviceToHost));
  return OSPF_OK;
}

int ospf_sweep_profile(ospf_sweep* s, uint32_t reps, ospf_sweep_launch* out, uint32_t cap) {
  if (!s || (cap && !out)) return OSPF_E_INVAL;
  if (!s->ran) return sfail(s, OSPF_E_INVAL, "sweep: profile needs one run first");
  ospf_ctx* c = s->c;
  if (c->graph_gen != s->gen) return sfail(s, OSPF_E_NOGRAPH, "sweep: the graph changed");
  reps = std::max(1u, reps);
  SCHK(s, hipSetDevice(c->device));
  SCHK(s, hipDeviceSynchronize());
  const uint64_t runs0 = c->spf_runs;
  hipEvent_t a, b;
  SCHK(s, hipEventCreate(&a));
  SCHK(s, hipEventCreate(&b));
  for (size_t i = 0; i < s->units.size() && i < cap; ++i) {
    auto& u = s->units[i];
    hipStream_t st = s->streams[u.stream];
    std::vector<double> ms;
    hipLaunchKernelGGL(sweep_unit_mark_kernel, dim3(1), dim3(64), 0, st, (uint32_t)i);
    SCHK(s, hipGetLastError());
    for (uint32_t k = 0; k <= reps; ++k) {
      SCHK(s, hipEventRecord(a, st));
      const int rc = u.fn(st);
      if (rc) return sfail(s, rc, u.name + ": " + ospf_last_error(c));
      SCHK(s, hipEventRecord(b, st));
      SCHK(s, hipEventSynchronize(b));
      float t = 0;
      SCHK(s, hipEventElapsedTime(&t, a, b));
      if (k) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    ospf_sweep_launch& L = out[i];
    std::memset(&L, 0, sizeof(L));
    std::snprintf(L.name, sizeof(L.name), "%s", u.name.c_str());
    std::snprintf(L.kernel, sizeof(L.kernel), "%s", u.kernel.c_str());
    L.n_roots = u.n_roots;
    L.nh_words = u.W;
    L.compulsory_bytes = u.comp;
    L.ms_median = ms[ms.size() / 2];
    L.ms_min = ms.front();
  }
  hipLaunchKernelGGL(sweep_unit_mark_kernel, dim3(1), dim3(64), 0, s->streams[0],
                     (uint32_t)s->units.size());
  SCHK(s, hipStreamSynchronize(s->streams[0]));
  hipEventDestroy(a);
  hipEventDestroy(b);
  c->spf_runs = runs0;
  return ospf_sync(c, nullptr);
}

}  // extern "C"
