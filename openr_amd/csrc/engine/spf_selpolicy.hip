// spf_selpolicy.hip — route selection under the reference's best-route policy
// over a sweep's resident rows (gfx950): what createRouteForPrefix
// (openr/decision/SpfSolver.cpp:197-458) decides per root before and after it
// takes the minimum -- the unreached announcers dropped, the best
// (path preference, source preference, distance) class kept (:649-676), the
// drained announcers filtered unless all are (:709-731), the route withheld
// below minNexthop (:976-1000) -- for every owned root of a sweep and every
// prefix of a table, in one launch. The rule and its 64-bit key are in
// spf_selpolicy_dev.h.
//
// Shape: select_kernel's (spf_select.hip). A workgroup per root (grid-stride),
// its waves striding over chunks of 64 prefixes; a prefix of <= kSelShort
// announcers is one lane's, a longer one the wave's (a lane per announcer),
// and roots of more than kSelLaneW next-hop words take every prefix with a
// lane per word. The block owns one root, so the links c(r, k) of the root's
// distinct-neighbour slots k -- up links r - k at the smallest metric r
// advertises on an up link to k, every up link under hop count (as
// ucmp_links_kernel has them) -- are built once per root in LDS from the
// root's CSR row: atomicMin of the metric, then a count where it is met, then
// packed to u16 (exact: the load refuses a parallel group of more than
// OSPF_MAX_PARALLEL_LINKS = 0xFFFF entries, so the pack's cap is never
// reached). An entry's `links` is the sum of c over its set next-hop bits.
// Every word of a wanted output is written once by plain vector stores; no
// memset, no global atomics, no scratch.
//
// Out of scope (include/openr_spf.h says so too): K_SHORTEST_DISTANCE_2 and
// PER_AREA_SHORTEST_DISTANCE, BGP metric vectors. (SR_MPLS per-destination next
// hops: spf_selsrmpls.hip, one area and one sweep. Several areas:
// spf_selareas.hip. A policy table in ospf_selstate_*:
// spf_seldelta_policy.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "spf_selpolicy_dev.h"
#include "sweep_impl.h"

namespace {

using namespace ospf_sel;
using namespace ospf_selpol;

struct PolicyArgs {
  const ospf_int::SelRow* rows;  // [n_roots], owned-roots order
  const uint32_t* roots;         // [n_roots] their node ids
  uint32_t n_roots, P, Wout, hop;
  uint32_t cap;                  // LDS slots (>= every root's distinct neighbours)
  Table t;
  // the loaded graph: the root's CSR row
  const uint32_t* row_ptr;
  const uint32_t* colx;
  const uint32_t* w;
  const uint16_t* didx;
  const uint32_t* dn_off;
  uint32_t *o_metric, *o_count, *o_nh, *o_links, *o_need, *o_best;
};

__global__ __launch_bounds__(256) void policy_kernel(const PolicyArgs a) {
  extern __shared__ uint32_t lds[];
  const uint16_t* cslot = reinterpret_cast<const uint16_t*>(lds);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P, Wout = a.Wout;
  const bool want_nh = a.o_nh != nullptr, want_links = a.o_links != nullptr;
  const bool aligned16 = !((uintptr_t)a.o_nh & 15u);
  for (uint32_t ri = blockIdx.x; ri < a.n_roots; ri += gridDim.x) {
    const uint32_t* __restrict__ dist = a.rows[ri].dist;
    const uint32_t* __restrict__ nh = a.rows[ri].nh;
    const uint32_t W = a.rows[ri].W;
    const uint32_t r = a.roots[ri];
    const uint32_t ns = min(a.dn_off[r + 1] - a.dn_off[r], a.cap);
    const size_t ob = (size_t)ri * P;
    if (want_links) build_links(a, r, ns, lds);  // block-uniform
    for (uint32_t base = wv * 64u; base < P; base += nwv * 64u) {
      const uint32_t p = base + lane;
      const bool in = p < P;
      const uint32_t n = min(64u, P - base);  // prefixes of this chunk
      uint32_t lo = 0, hi = 0;
      if (in) {
        lo = a.t.off[p];
        hi = a.t.off[p + 1];
      }
      Entry e;
      uint32_t links = 0;
      if (W <= kSelLaneW) {
        uint32_t acc[kSelLaneW];
#pragma unroll
        for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
        const bool mine = in && hi - lo <= kSelShort;
        const unsigned long long wide = __ballot(in && !mine);
        // the words feed the links too
        if (mine) policy_by_lane(a.t, dist, nh, W, r, lo, hi, want_nh || want_links, e, acc);
        // the chunk's long prefixes, one at a time by the wave; the result
        // parked in the prefix's own lane
        for (unsigned long long t = wide; t; t &= t - 1ull) {
          const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
          Entry we;
          uint32_t wa[kSelLaneW];
          policy_by_lanes(a.t, dist, nh, W, r, lane_get(lo, j), lane_get(hi, j), lane,
                          want_nh || want_links, we, wa);
          if (lane == j) {
            e = we;
#pragma unroll
            for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = wa[w];
          }
        }
        if (want_links) links = links_of(acc, W, cslot, ns);
        if (want_nh)
          store_chunk_words(a.o_nh + (ob + base) * Wout, aligned16, acc, W, Wout, n, lane, in);
      } else {
        for (uint32_t j = 0; j < n; ++j) {
          Entry we;
          const uint32_t wl =
              policy_by_words(a.t, dist, nh, W, r, lane_get(lo, j), lane_get(hi, j), lane, Wout,
                              want_nh ? a.o_nh + (ob + base + j) * Wout : nullptr, cslot, ns,
                              want_links, we);
          if (lane == j) {
            e = we;
            links = wl;
          }
        }
      }
      if (in) {
        if (a.o_metric) a.o_metric[ob + p] = e.m;
        if (a.o_count) a.o_count[ob + p] = e.cnt;
        if (a.o_links) a.o_links[ob + p] = links;
        if (a.o_need) a.o_need[ob + p] = e.need;
        if (a.o_best) a.o_best[ob + p] = e.best;
      }
    }
  }
}

using namespace ospf_int::sweep;

bool any_out(const ospf_select_pout* o) {
  return o->metric || o->count || o->nh || o->links || o->need || o->best;
}

}  // namespace

uint32_t ospf_int::sweep::policy_row_words(const ospf_sweep* s) {
  uint32_t mw = 0;
  for (uint32_t r : s->roots) mw = std::max(mw, s->row_w[r]);
  return mw;
}

// the policy table's contract beyond ospf_select_table's
const char* ospf_int::sweep::select_ptable_check(const ospf_select_ptable* t, uint32_t V) {
  if (!t) return "select: null table";
  const ospf_select_table plain{t->n_prefixes, t->offsets, t->nodes};
  if (const char* bad = select_table_check(&plain, V)) return bad;
  const uint32_t A = t->n_prefixes ? t->offsets[t->n_prefixes] : 0u;
  if (A && !t->pref) return "select policy: null pref";
  for (uint32_t k = 0; k < A; ++k)
    if (t->pref[k] >= 0x80000000u) return "select policy: a pref >= 2^31";
  return nullptr;
}

// the device side of a policy table (sweep_impl.h)
int ospf_int::sweep::policy_upload(ospf_sweep* s, const ospf_select_ptable* t,
                                   const uint32_t* flags, PolicyTab* d) {
  ospf_ctx* c = s->c;
  const uint32_t P = t->n_prefixes;
  SCHK(s, hipSetDevice(c->device));
  if (const int rc = select_rows(s)) return rc;
  if (!s->d_pol_roots) {
    uint32_t* d = nullptr;
    if (const int rc = upload(s, &d, s->roots)) return rc;
    s->d_pol_roots = d;
  }
  // the table's device copy (offsets, nodes, pref, min_nexthop): the buffer is
  // the last call's, free once that call's kernel is done
  const size_t A = t->offsets[P], words = (size_t)P + 1 + (flags ? 4 : 3) * A;
  if (s->pol_ev) SCHK(s, hipEventSynchronize(s->pol_ev));
  if (words > s->pol_tab_words) {
    if (s->d_pol_tab) SCHK(s, hipFree(s->d_pol_tab));
    s->d_pol_tab = nullptr;
    s->pol_tab_words = 0;
    void* q = nullptr;
    if (hipMalloc(&q, words * 4) != hipSuccess) {
      (void)hipGetLastError();
      return sfail(s, OSPF_E_NOMEM, "select policy: hipMalloc of the prefix table");
    }
    s->d_pol_tab = (uint32_t*)q;
    s->pol_tab_words = words;
  }
  uint32_t* d_off = s->d_pol_tab;
  uint32_t* d_nodes = d_off + P + 1;
  uint32_t* d_pref = d_nodes + A;
  uint32_t* d_mnh = d_pref + A;
  SCHK(s, hipMemcpy(d_off, t->offsets, ((size_t)P + 1) * 4, hipMemcpyHostToDevice));
  if (A) {
    SCHK(s, hipMemcpy(d_nodes, t->nodes, A * 4, hipMemcpyHostToDevice));
    SCHK(s, hipMemcpy(d_pref, t->pref, A * 4, hipMemcpyHostToDevice));
    if (t->min_nexthop)
      SCHK(s, hipMemcpy(d_mnh, t->min_nexthop, A * 4, hipMemcpyHostToDevice));
  }
  if (!s->pol_ev) SCHK(s, hipEventCreateWithFlags(&s->pol_ev, hipEventDisableTiming));
  if (flags && A) SCHK(s, hipMemcpy(d_mnh + A, flags, A * 4, hipMemcpyHostToDevice));
  *d = PolicyTab{d_off, d_nodes, d_pref, t->min_nexthop && A ? d_mnh : nullptr,
                 flags && A ? d_mnh + A : nullptr};
  return OSPF_OK;
}

// ospf_sweep_select_policy_dev without the fault-injection hook (the host and
// multi-device calls hook once themselves)
int ospf_int::sweep::policy_queue(ospf_sweep* s, const ospf_select_ptable* t, uint32_t nh_words,
                                  const ospf_select_pout* d_out, void* stream) {
  ospf_ctx* c = s->c;
  if (!s->ran) return sfail(s, OSPF_E_INVAL, "sweep: select before the first run");
  if (const char* bad = select_ptable_check(t, s->V)) return sfail(s, OSPF_E_INVAL, bad);
  if (nh_words < policy_row_words(s))
    return sfail(s, OSPF_E_INVAL, "sweep: nh_words below a root's next-hop words");
  // the kernel reads the live CSR and no-transit bits beside the rows
  if (!c || !c->loaded || c->graph_gen != s->gen || c->mask.on || c->info.n_nodes != s->V)
    return sfail(s, OSPF_E_INVAL, "select policy: the graph changed since the sweep was created");
  const uint32_t n = (uint32_t)s->roots.size(), P = t->n_prefixes;
  if (!n || !P || !any_out(d_out)) return OSPF_OK;
  PolicyTab d{};
  if (const int rc = policy_upload(s, t, nullptr, &d)) return rc;
  PolicyArgs a{};
  a.rows = s->d_sel_rows;
  a.roots = s->d_pol_roots;
  a.n_roots = n;
  a.P = P;
  a.Wout = nh_words;
  a.hop = (s->opts.flags & OSPF_HOP_COUNT) ? 1u : 0u;
  a.cap = std::max(1u, c->max_dn);
  a.t = Table{d.off, d.nodes, d.pref, d.mnh, c->g.nt_bits};
  a.row_ptr = c->g.row_ptr;
  a.colx = c->g.colx;
  a.w = c->g.w;
  a.didx = c->g.didx;
  a.dn_off = c->g.dn_off;
  a.o_metric = d_out->metric;
  a.o_count = d_out->count;
  a.o_nh = d_out->nh;
  a.o_links = d_out->links;
  a.o_need = d_out->need;
  a.o_best = d_out->best;
  // a wave per 64 prefixes of the root, at most 4; roots beyond the grid by
  // stride; LDS: two words per slot while a root's links are built
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  const uint32_t grid = std::min(n, 1u << 20);
  const size_t lds = d_out->links ? (size_t)a.cap * 8 : 0;
  if (lds > c->lds_limit)
    return sfail(s, OSPF_E_RANGE, "select policy: the widest root's link counts do not fit the LDS");
  hipLaunchKernelGGL(policy_kernel, dim3(grid), dim3(64u * waves), lds, (hipStream_t)stream, a);
  SCHK(s, hipGetLastError());
  SCHK(s, hipEventRecord(s->pol_ev, (hipStream_t)stream));
  return OSPF_OK;
}

extern "C" {

int ospf_sweep_select_policy_dev(ospf_sweep* s, const ospf_select_ptable* t, uint32_t nh_words,
                                 const ospf_select_pout* d_out, void* stream) {
  if (!s || !t || !d_out) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  return policy_queue(s, t, nh_words, d_out, stream);
}

int ospf_sweep_select_policy(ospf_sweep* s, const ospf_select_ptable* t, uint32_t nh_words,
                             const ospf_select_pout* out) {
  if (!s || !t || !out) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  const size_t cells = s->roots.size() * (size_t)t->n_prefixes;
  PolicyOut d;
  if (cells && s->ran) {
    SCHK(s, hipSetDevice(s->c->device));
    SCHK(s, hipDeviceSynchronize());  // the rows, whichever streams ran the sweep
    if (!d.alloc(cells, std::max(1u, nh_words), out)) {
      (void)hipGetLastError();
      return sfail(s, OSPF_E_NOMEM, "select policy: hipMalloc of the outputs");
    }
  }
  const int rc = policy_queue(s, t, nh_words, &d.o, nullptr);
  if (rc || !cells) return rc;
  // into buffers of this call first: a failed copy leaves the caller's as they were
  std::vector<uint32_t> h[6];
  uint32_t* const src[6] = {d.o.metric, d.o.count, d.o.nh, d.o.links, d.o.need, d.o.best};
  uint32_t* const dst[6] = {out->metric, out->count, out->nh, out->links, out->need, out->best};
  for (int i = 0; i < 6; ++i) {
    if (!src[i]) continue;
    h[i].resize(cells * (i == 2 ? nh_words : 1u));
    SCHK(s, hipMemcpy(h[i].data(), src[i], h[i].size() * 4, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 6; ++i)
    if (src[i]) std::copy(h[i].begin(), h[i].end(), dst[i]);
  return OSPF_OK;
}

}  // extern "C"
