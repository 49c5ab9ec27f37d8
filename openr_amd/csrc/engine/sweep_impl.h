// sweep_impl.h — the sweep object and what its translation units share:
// spf_sweep.hip (plumbing, run, capture, the ospf_sweep_* ABI), sweep_units.hip
// (unit helpers, the batch and LDS planners), sweep_plan_derive.hip,
// sweep_plan_weighted.hip and spf_multi.hip (ospf_multi_* / ospf_msweep_*).
// Not a public header.
#pragma once

#include <functional>

#include "spf_internal.h"

// ---------------------------------------------------------------- the sweep
struct ospf_sweep {
  ospf_ctx* c = nullptr;
  ospf_sweep_opts opts{};
  uint32_t mode = 0;
  uint64_t gen = 0;
  std::string err;
  uint32_t V = 0;
  std::vector<uint32_t> roots;          // owned roots, digest order
  std::vector<uint32_t> own_slot;       // digest slot of roots[i] in dig_all
  // row of each owned root: device pointers, by node id (null: not owned)
  std::vector<const uint32_t*> row_dist, row_nh;
  std::vector<uint32_t> row_w;
  std::vector<void*> allocs;            // device allocations
  std::vector<size_t> alloc_bytes;      // their sizes (returned to the ctx's pool)
  uint64_t device_bytes = 0;
  ospf_digest* dig_all = nullptr;       // every digest a run writes
  uint32_t n_dig = 0;
  std::vector<std::pair<ospf_digest*, size_t>> dig_aux;  // intermediate digests (poisoned too)
  uint32_t* d_own_slot = nullptr;
  uint32_t n_rows = 0;
  uint64_t trav_edges = 0;  // edges scanned by the run's traversal kernels (TEPS)
  uint64_t step_comp = 0;
  // launches. A unit's fn outlives the planner that built it: it captures by
  // value only -- device pointers, scalars, the context, the sweep and small
  // POD plans -- never a reference or pointer to a planner's host state.
  struct Unit {
    std::string name, kernel;
    int stream = 0;            // index into streams (0 = main)
    std::vector<int> wait;     // events waited for before the launch
    int record = -1;           // event recorded after it
    std::function<int(hipStream_t)> fn;
    uint32_t n_roots = 0, W = 0;
    uint64_t comp = 0;
  };
  std::vector<Unit> units;
  std::vector<hipStream_t> streams;     // [0] = main
  std::vector<hipEvent_t> events;       // [0] = run start
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  std::vector<hipEvent_t> ev_done;      // per non-main stream
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool ran = false;
  // OSPF_SWEEP_EARLY_START: units [0, started) of the first run already
  // queued by the plan (after ev_in on the null stream and events[0])
  bool early = false, early_on = false;
  size_t started = 0;
  // block order of the leaf launch (0 chunk-major, 1 group-major): picked at
  // create by timing both -- which order stores faster depends on where the
  // allocation's rows fall in the memory channels (the probe's two patterns
  // swap places from one allocation to the next)
  int leaf_order = 0;
  // the seed BFS's deepest level in the first run (device word), and the
  // level launches the HIP graph captures (0: the graph's transit-depth bound)
  uint32_t* d_lv_maxd = nullptr;
  uint32_t lv_cap = 0;
  // ospf_sweep_select*: the owned roots' rows as a device table (uploaded on
  // first use), the last prefix table's device copy (offsets, then nodes;
  // grown on demand) and the event after the last launch that reads it
  ospf_int::SelRow* d_sel_rows = nullptr;
  uint32_t* d_sel_tab = nullptr;
  size_t sel_tab_words = 0;
  hipEvent_t sel_ev = nullptr;
  // ospf_sweep_select_policy*: the owned roots' node ids on the device
  // (uploaded on first use), the last policy table's device copy (offsets,
  // nodes, pref, min_nexthop; grown on demand) and the event after the last
  // launch that reads it
  uint32_t* d_pol_roots = nullptr;
  uint32_t* d_pol_tab = nullptr;
  size_t pol_tab_words = 0;
  hipEvent_t pol_ev = nullptr;
  // ospf_areas_select_policy*: every node's rows as a device table BY NODE ID
  // (uploaded on first use; the sweep owns every root), and -- on area 0's
  // sweep -- the last call's device block (per-area pointers, global -> local
  // ids, the table; grown on demand) with the event after the launch that
  // reads it
  ospf_int::SelRow* d_area_rows = nullptr;
  void* d_areas_blob = nullptr;
  size_t areas_blob_bytes = 0;
  hipEvent_t areas_ev = nullptr;
};

namespace ospf_int {
namespace sweep {

using Unit = ospf_sweep::Unit;

constexpr uint32_t kNone = 0xFFFFFFFFu;

// ---------------------------------------------------------------- host graph facts
// distinct neighbours (ascending id, links of any state) come from the
// context's host copy (ospf_load_graph: dn_off / dn)
struct Facts {
  uint32_t V = 0;
  const std::vector<uint32_t>* dn_off = nullptr;
  const std::vector<uint32_t>* dn = nullptr;
  uint32_t nbrs(uint32_t v) const { return (*dn_off)[v + 1] - (*dn_off)[v]; }
  // smallest / largest neighbour id (V / 0 for an isolated node)
  uint64_t first(uint32_t v) const { return nbrs(v) ? (*dn)[(*dn_off)[v]] : V; }
  uint64_t last(uint32_t v) const { return nbrs(v) ? (*dn)[(*dn_off)[v + 1] - 1] : 0; }
  // launch class: 8, 16 or 32 x next-hop words (distinct neighbours)
  uint32_t cap(uint32_t v) const {
    const uint32_t k = nbrs(v);
    return k <= 8 ? 8u : k <= 16 ? 16u : 32u * std::max(1u, (k + 31) / 32);
  }
  uint32_t words(uint32_t v) const { return std::max(1u, (nbrs(v) + 31) / 32); }
  // a and b have the same distinct neighbours
  bool same_nbrs(uint32_t a, uint32_t b) const {
    return nbrs(a) == nbrs(b) && std::equal(dn->begin() + (*dn_off)[a], dn->begin() + (*dn_off)[a + 1],
                                            dn->begin() + (*dn_off)[b]);
  }
};

// stable order of `v` by key(v)
template <class K>
void locality_order(std::vector<uint32_t>& v, K key) {
  std::stable_sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
}

// the distinct key(r) over `roots`, ascending: the launch classes of these
// roots under Facts::cap / Facts::words
template <class K>
std::vector<uint32_t> classes_by(const std::vector<uint32_t>& roots, K key) {
  std::vector<uint32_t> k;
  for (uint32_t r : roots) k.push_back(key(r));
  std::sort(k.begin(), k.end());
  k.erase(std::unique(k.begin(), k.end()), k.end());
  return k;
}

// sorted ids of `roots` and all their neighbours
std::vector<uint32_t> closure(const Facts& f, const std::vector<uint32_t>& roots);
// Independent set of nodes with <= max_nbrs distinct neighbours, greedy in
// (distinct neighbours, id) order
std::vector<uint8_t> leaf_set(const Facts& f, uint32_t max_nbrs = 32);

// ---------------------------------------------------------------- plumbing
int sfail(ospf_sweep* s, int code, const std::string& m);

#define SCHK(sw, call)                                                                \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess)                                                             \
      return ospf_int::sweep::sfail(sw, OSPF_E_DEVICE,                                \
                                    std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class T>
int dalloc(ospf_sweep* s, T** p, size_t count) {
  void* q = nullptr;
  const size_t want = std::max<size_t>(count, 1) * sizeof(T);
  // a block of a destroyed sweep, at most 1/8 larger (+ 1 MB), else new
  ospf_ctx* c = s->c;
  size_t bytes = (want + 255) & ~(size_t)255;
  auto it = c->sweep_pool.lower_bound(bytes);
  if (it != c->sweep_pool.end() && it->first <= bytes + bytes / 8 + (1u << 20)) {
    q = it->second;
    bytes = it->first;
    c->sweep_pool_bytes -= bytes;
    c->sweep_pool.erase(it);
  } else {
    const hipError_t e = ospf_int::dev_malloc(c, &q, bytes);  // frees the pool on failure
    if (e != hipSuccess)
      return sfail(s, OSPF_E_NOMEM, "sweep: hipMalloc " + std::to_string(bytes) + " B: " +
                                        hipGetErrorString(e));
  }
  s->allocs.push_back(q);
  s->alloc_bytes.push_back(bytes);
  s->device_bytes += bytes;
  *p = (T*)q;
  return OSPF_OK;
}

// dalloc without an error message (a caller that retries smaller)
template <class T>
int dalloc_try(ospf_sweep* s, T** p, size_t count) {
  const std::string keep = s->err, keep_c = s->c ? s->c->err : std::string();
  const int rc = dalloc(s, p, count);
  if (rc) {
    s->err = keep;
    if (s->c) s->c->err = keep_c;
  }
  return rc;
}

template <class T>
int upload(ospf_sweep* s, T** p, const std::vector<T>& h) {
  int rc = dalloc(s, p, h.size());
  if (rc) return rc;
  if (!h.empty()) SCHK(s, hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return OSPF_OK;
}

// a stream / an event of the sweep (from the context's pools): its index, < 0 on error
int new_stream(ospf_sweep* s);
int new_event(ospf_sweep* s);
// Row pitch (u32 words) of the sweep's dist / one-word next-hop rows
uint32_t row_pitch(uint32_t V);
// CSR bytes one distance-only scan reads: neighbour ids + row offsets
uint64_t scan_bytes(const ospf_ctx* c, bool weighted);
// owned root r's digest is slot `slot` of dig_all; its rows are (d, nh, W)
void own(ospf_sweep* s, uint32_t r, uint32_t slot, const uint32_t* d, const uint32_t* nh, uint32_t W);
// OSPF_SWEEP_EARLY_START: queue the units planned so far
int start_early(ospf_sweep* s);

// ---------------------------------------------------------------- units (sweep_units.hip)
// `roots` in order own digest slots slot0, slot0 + 1, ... and W-word next-hop
// rows j of `nh` (pitch nh_pitch words); their dist rows are rows pos[r] of
// `dist` (pitch dist_pitch words), rows j without `pos`. With `only`, the
// roots it marks (the others keep their slot and rows unowned).
void own_rows(ospf_sweep* s, const std::vector<uint32_t>& roots, uint32_t slot0, const uint32_t* dist,
              size_t dist_pitch, const uint32_t* nh, size_t nh_pitch, uint32_t W,
              const std::vector<uint32_t>* pos = nullptr, const std::vector<uint8_t>* only = nullptr);
// a class's roots on the device with packed dist and W-word next-hop rows of
// their own, owning digest slots slot, slot + 1, ...; slot moves past them
int class_rows(ospf_sweep* s, const std::vector<uint32_t>& roots, uint32_t W, uint32_t& slot,
               uint32_t** d_roots, uint32_t** dist, uint32_t** nh);
// append a planned unit (capture order); the step's compulsory bytes count
// step_bytes for it
void add_unit(ospf_sweep* s, Unit&& u, uint64_t step_bytes);
inline void add_unit(ospf_sweep* s, Unit&& u) {
  const uint64_t b = u.comp;
  add_unit(s, std::move(u), b);
}
// a unit that runs ospf_run_batch_dev over n device roots from the run's
// start (the caller picks its stream, kernel text and event)
Unit batch_unit(ospf_ctx* c, const std::string& name, const uint32_t* d_roots, uint32_t n, uint32_t flags,
                uint32_t W, uint32_t mx, uint32_t* dist, uint32_t* nh, ospf_digest* dg, uint64_t comp);
// batch_unit for one width class (`cap`) on a stream of its own: kernel text
// and scan bytes from the variant the engine will pick (ospf_plan_n)
int class_batch_unit(ospf_sweep* s, Unit& u, const std::string& name, const uint32_t* d_roots, uint32_t n,
                     uint32_t flags, uint32_t W, uint32_t mx, uint32_t* dist, uint32_t* nh,
                     ospf_digest* dg, bool weighted);

// ---------------------------------------------------------------- planners
// each appends the part's units, rows and digest slots to the sweep
int plan_derive(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine);
int plan_batch(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine, bool weighted);
int plan_lds(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine);
int plan_wcover(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                const std::vector<uint8_t>& leaf);
int plan_wmulti(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                const std::vector<uint8_t>& leaf);
int plan_wderive(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                 const std::vector<uint8_t>& leaf);

// ---------------------------------------------------------------- select
// ospf_sweep_select_dev without the fault-injection hook (the host and
// multi-device calls hook once themselves)
int select_queue(ospf_sweep* s, const ospf_select_table* t, uint32_t nh_words, uint32_t* d_metric,
                 uint32_t* d_count, uint32_t* d_nh, void* stream);

// the table's contract (ospf_select_table) for a graph of V nodes: null when
// it holds, else what is wrong
const char* select_table_check(const ospf_select_table* t, uint32_t V);
// the owned roots' rows as a device table (s->d_sel_rows, owned-roots order),
// uploaded on first use
int select_rows(ospf_sweep* s);

// device outputs of one select ([n][P], [n][P], [n][P][W]; only the wanted
// ones), freed by the destructor
struct SelectOut {
  uint32_t *m = nullptr, *k = nullptr, *nh = nullptr;
  ~SelectOut() {
    if (m) hipFree(m);
    if (k) hipFree(k);
    if (nh) hipFree(nh);
  }
  bool alloc(size_t cells, uint32_t W, bool wm, bool wk, bool wnh) {
    return (!wm || hipMalloc((void**)&m, cells * 4) == hipSuccess) &&
           (!wk || hipMalloc((void**)&k, cells * 4) == hipSuccess) &&
           (!wnh || hipMalloc((void**)&nh, cells * W * 4) == hipSuccess);
  }
};

// ---------------------------------------------------------------- select policy
// ospf_sweep_select_policy_dev without the fault-injection hook (the host and
// multi-device calls hook once themselves)
int policy_queue(ospf_sweep* s, const ospf_select_ptable* t, uint32_t nh_words,
                 const ospf_select_pout* d_out, void* stream);
// the policy table's contract (ospf_select_ptable) for a graph of V nodes:
// null when it holds, else what is wrong
const char* select_ptable_check(const ospf_select_ptable* t, uint32_t V);
// the widest next-hop row among the owned roots, in words
uint32_t policy_row_words(const ospf_sweep* s);
// What a policy launch reads beside the rows, made ready on the device: the
// rows table (select_rows), the owned roots' ids (s->d_pol_roots) and the
// table's columns copied into s->d_pol_tab (offsets, nodes, pref, min_nexthop,
// then `flags` when given: one word per entry, ospf_select_stable's), after a
// host wait for the last launch that read that buffer. The caller records
// s->pol_ev behind its kernel.
struct PolicyTab {
  const uint32_t *off, *nodes, *pref, *mnh, *flags;  // device; mnh / flags null when not given
};
int policy_upload(ospf_sweep* s, const ospf_select_ptable* t, const uint32_t* flags, PolicyTab* d);
// ospf_sweep_select_srmpls_dev without the fault-injection hook
int srmpls_queue(ospf_sweep* s, const ospf_select_stable* t, uint32_t nh_words,
                 const ospf_select_sout* d_out, void* stream);

// device outputs of one policy select (only the wanted ones of `want`), freed
// by the destructor
struct PolicyOut {
  ospf_select_pout o{};
  ~PolicyOut() {
    for (uint32_t* p : {o.metric, o.count, o.nh, o.links, o.need, o.best})
      if (p) (void)hipFree(p);
  }
  bool alloc(size_t cells, uint32_t W, const ospf_select_pout* want) {
    auto get = [](uint32_t** p, size_t words) { return hipMalloc((void**)p, words * 4) == hipSuccess; };
    return (!want->metric || get(&o.metric, cells)) && (!want->count || get(&o.count, cells)) &&
           (!want->nh || get(&o.nh, cells * W)) && (!want->links || get(&o.links, cells)) &&
           (!want->need || get(&o.need, cells)) && (!want->best || get(&o.best, cells));
  }
};

}  // namespace sweep
}  // namespace ospf_int
