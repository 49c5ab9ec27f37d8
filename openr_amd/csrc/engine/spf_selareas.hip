// spf_selareas.hip — route selection under the reference's best-route policy
// across several areas, over the resident rows of one sweep per area (gfx950):
// createRouteForPrefix (openr/decision/SpfSolver.cpp:197-458) for every node of
// the union of the areas and every prefix of a table of (node, area) entries,
// in one launch. The rule is spelled out at ospf_areas_select_policy in
// include/openr_spf.h; with one area it is policy_kernel's (spf_selpolicy.hip).
//
// Per (global root g, prefix p) the work is four walks over the prefix's
// entries: (1) the smallest key pref << 33 | drained << 32 | dist over the
// entries g reaches in their own areas -- only its high word, the class and
// the drained bit, is meaningful across areas; (2) need, best and the areas
// that hold an entry of their own in S'; (3) per such area a the smallest
// dist_a[g][n] over the nodes n of all of S' (other areas' announcers looked
// up by name: lid[a][n]), which gives the metric and the winning areas; (4)
// per area of g the count and the next-hop words of the nodes at the metric.
// The entries are re-walked per area rather than kept as per-area partials:
// a root has a handful of areas but up to 32 are allowed, and 32 x (metric,
// count, kSelLaneW words) per lane would cost the occupancy every root pays
// for; the re-walk re-reads table words the L2 holds and distance words of
// the root's own rows.
//
// Shape: policy_kernel's. A workgroup per global root (grid-stride), so every
// gather lands in that root's rows of its few areas; the root's per-area state
// (row pointers, local id, widths) sits in LDS. Waves stride over chunks of 64
// prefixes. When every area of the root has <= kSelLaneW next-hop words, a
// prefix of <= kSelShort entries is one lane's (its S' membership an 8-bit
// mask) and a longer one the wave's, a lane per entry; a root with a wider
// area takes every prefix by the wave, and the wide area's words with a lane
// per word. The links c(r, k) of the root's neighbour slots are built per
// area of the root with build_links (spf_selpolicy_dev.h) and packed one area
// after the other in LDS. Every word of a wanted output is written once by
// plain vector stores; no memset, no global atomics, no scratch.
//
// The per-prefix device functions are in spf_selareas_dev.h, shared with the
// resident state and its delta (spf_seldelta_areas.hip).
//
// Out of scope (include/openr_spf.h says so too): UCMP across areas, SR_MPLS
// per-destination next hops across areas (one area: spf_selsrmpls.hip) and
// KSP2, BGP metric vectors, ospf_msweep and several devices.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "spf_selareas_dev.h"
#include "spf_selstate.h"
#include "sweep_impl.h"

namespace {

using namespace ospf_selareas;
using ospf_selareas::kNone;  // not ospf_int::sweep's

// one area as the kernel sees it (device memory, [n_areas])
struct AreaDev {
  const ospf_int::SelRow* rows;  // [V_a] by node id
  const uint32_t* lid;           // [G] global id -> node id, kNone: absent
  const uint32_t* nt_bits;       // the loaded graph
  const uint32_t* row_ptr;
  const uint32_t* colx;
  const uint32_t* w;
  const uint16_t* didx;
  const uint32_t* dn_off;
  uint32_t* o_nh;                // [V_a][P][Wout] or null
  uint32_t Wout, cap;            // cap: LDS slots while the links are built
};

struct AreasArgs {
  const AreaDev* areas;
  uint32_t A, G, P, hop;
  uint32_t capmax;   // LDS slots of the widest root of any area
  uint32_t sumcap;   // u16 link counts behind them: the largest sum over a root's areas
  Tab t;
  uint32_t *o_metric, *o_count, *o_links, *o_need, *o_best, *o_areas;
};

__global__ __launch_bounds__(256) void areas_kernel(const AreasArgs a) {
  extern __shared__ uint32_t lds[];
  __shared__ RootArea ra[kMaxAreas];
  __shared__ uint32_t s_wide;
  // the link counts: build_links' 2 * capmax words, then the packed u16 counts
  // of the root's areas
  uint16_t* cpack = reinterpret_cast<uint16_t*>(lds + 2u * a.capmax);
  const uint16_t* cslot = cpack;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P, A = a.A;
  const bool want_links = a.o_links != nullptr;
  for (uint32_t g = blockIdx.x; g < a.G; g += gridDim.x) {
    __syncthreads();  // the previous root's areas are read no more
    if (threadIdx.x < A) {
      const AreaDev& ad = a.areas[threadIdx.x];
      RootArea x{};
      x.lid = ad.lid;
      x.nt = ad.nt_bits;
      x.la = ad.lid[g];
      if (x.la != kNone) {
        const ospf_int::SelRow row = ad.rows[x.la];
        x.dist = row.dist;
        x.nh = row.nh;
        x.W = row.W;
        x.Wout = ad.Wout;
        x.o_nh = ad.o_nh ? ad.o_nh + (size_t)x.la * P * ad.Wout : nullptr;
        x.ns = min(ad.dn_off[x.la + 1] - ad.dn_off[x.la], ad.cap);
      }
      ra[threadIdx.x] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t off = 0, wide = 0;
      for (uint32_t ar = 0; ar < A; ++ar) {
        if (ra[ar].la == kNone) continue;
        ra[ar].ns = min(ra[ar].ns, a.sumcap - off);  // the host sized sumcap for every root
        ra[ar].coff = off;
        off += ra[ar].ns;
        wide |= ra[ar].W > kSelLaneW ? 1u : 0u;
      }
      s_wide = wide;
    }
    __syncthreads();
    if (want_links)
      for (uint32_t ar = 0; ar < A; ++ar) {  // block-uniform
        if (ra[ar].la == kNone) continue;
        const AreaDev& ad = a.areas[ar];
        const LinkArgs la{ad.row_ptr, ad.colx, ad.w, ad.didx, a.hop, a.capmax};
        const uint32_t ns = ra[ar].ns;
        build_links(la, ra[ar].la, ns, lds);
        const uint16_t* c16 = reinterpret_cast<const uint16_t*>(lds);
        for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) cpack[ra[ar].coff + i] = c16[i];
      }
    __syncthreads();
    const bool root_wide = s_wide != 0u;
    const size_t ob = (size_t)g * P;
    for (uint32_t base = wv * 64u; base < P; base += nwv * 64u) {
      const uint32_t p = base + lane;
      const bool in = p < P;
      const uint32_t n = min(64u, P - base);  // prefixes of this chunk
      uint32_t lo = 0, hi = 0;
      if (in) {
        lo = a.t.off[p];
        hi = a.t.off[p + 1];
      }
      const bool mine = in && !root_wide && hi - lo <= kSelShort;
      const unsigned long long wide = __ballot(in && !mine);
      Sel s;
      if (mine) s = sel_by_lane(a.t, ra, g, lo, hi);
      // the chunk's other prefixes, one at a time by the wave; the result
      // parked in the prefix's own lane
      for (unsigned long long q = wide; q; q &= q - 1ull) {
        const uint32_t j = (uint32_t)__ffsll((long long)q) - 1u;
        const Sel ws = sel_by_wave(a.t, ra, g, lane_get(lo, j), lane_get(hi, j), lane);
        if (lane == j) s = ws;
      }
      uint32_t cnt = 0, links = 0;
      for (uint32_t ar = 0; ar < A; ++ar) {  // wave-uniform
        const RootArea& x = ra[ar];
        if (x.la == kNone) continue;
        const bool want_words = x.o_nh != nullptr || want_links;
        if (x.W <= kSelLaneW) {
          uint32_t acc[kSelLaneW];
#pragma unroll
          for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
          if (mine && ((s.win >> ar) & 1u)) area_by_lane(a.t, x, ar, lo, s, want_words, cnt, acc);
          for (unsigned long long q = wide; q; q &= q - 1ull) {
            const uint32_t j = (uint32_t)__ffsll((long long)q) - 1u;
            Sel ws;
            ws.m = lane_get(s.m, j);
            ws.win = lane_get(s.win, j);
            ws.cls = lane_get(s.cls, j);
            if (!((ws.win >> ar) & 1u)) continue;  // wave-uniform
            uint32_t wc = 0, wa[kSelLaneW];
#pragma unroll
            for (uint32_t w = 0; w < kSelLaneW; ++w) wa[w] = 0;
            area_by_wave(a.t, ra, ar, lane_get(lo, j), lane_get(hi, j), ws, lane, want_words, wc,
                         wa);
            if (lane == j) {
              cnt += wc;
#pragma unroll
              for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = wa[w];
            }
          }
          if (want_links) links += links_of(acc, x.W, cslot + x.coff, x.ns);
          if (x.o_nh)
            store_chunk_words(x.o_nh + (size_t)base * x.Wout, !((uintptr_t)x.o_nh & 15u), acc, x.W,
                              x.Wout, n, lane, in);
        } else {
          // a wide area: the root is wide, so every prefix is the wave's
          for (uint32_t j = 0; j < n; ++j) {
            Sel ws;
            ws.m = lane_get(s.m, j);
            ws.win = lane_get(s.win, j);
            ws.cls = lane_get(s.cls, j);
            uint32_t wc = 0;
            const uint32_t wl = area_by_words(
                a.t, ra, ar, lane_get(lo, j), lane_get(hi, j), ws, lane,
                x.o_nh ? x.o_nh + (size_t)(base + j) * x.Wout : nullptr, cslot, want_links, wc);
            if (lane == j) {
              cnt += wc;
              links += wl;
            }
          }
        }
      }
      if (in) {
        if (a.o_metric) a.o_metric[ob + p] = s.m;
        if (a.o_count) a.o_count[ob + p] = cnt;
        if (a.o_links) a.o_links[ob + p] = links;
        if (a.o_need) a.o_need[ob + p] = s.need;
        if (a.o_best) a.o_best[ob + p] = s.best;
        if (a.o_areas) a.o_areas[ob + p] = s.win;
      }
    }
  }
}

using namespace ospf_int::sweep;

using ospf_int::selst::area_rows;
using ospf_int::selst::areas_sweep_error;
using ospf_int::selst::areas_table_error;
using ospf_int::selst::max_words;

// the call's contract: null when it holds, else what is wrong. Fills lid
// [A][G] (global -> node id) on the way.
const char* areas_check(const ospf_areas_table* t, const ospf_areas_pout* out,
                        std::vector<uint32_t>& lid) {
  const uint32_t A = t->n_areas;
  ospf_sweep* s0 = t->sweeps[0];
  if (!t->gid) return "select areas: null gid";
  for (uint32_t a = 0; a < A; ++a) {
    const ospf_sweep* s = t->sweeps[a];
    if (const char* bad = areas_sweep_error(s, s0)) return bad;
    if (s->V && !t->gid[a]) return "select areas: null gid of an area";
    if (out->nh && out->nh[a]) {
      if (!out->nh_words) return "select areas: null nh_words";
      if (out->nh_words[a] < std::max(1u, max_words(s)))
        return "select areas: nh_words below a root's next-hop words";
    }
  }
  std::vector<uint32_t> V(A);
  for (uint32_t a = 0; a < A; ++a) V[a] = t->sweeps[a]->V;
  return areas_table_error(t, V.data(), lid);
}

}  // namespace

const char* ospf_int::selst::areas_sweep_error(const ospf_sweep* s, const ospf_sweep* s0) {
  const ospf_ctx* c = s->c;
  if (!s->ran) return "select areas: a sweep has not run";
  if (!c || !c->loaded || c->graph_gen != s->gen || c->mask.on || c->info.n_nodes != s->V)
    return "select areas: an area's graph changed since its sweep was created";
  if (!s0->c || c->device != s0->c->device) return "select areas: sweeps on different devices";
  if (s->roots.size() != s->V) return "select areas: a sweep does not own every root";
  if ((s->opts.flags & OSPF_HOP_COUNT) != (s0->opts.flags & OSPF_HOP_COUNT))
    return "select areas: mixed metric modes";
  return nullptr;
}

const char* ospf_int::selst::areas_table_error(const ospf_areas_table* t, const uint32_t* Va,
                                               std::vector<uint32_t>& lid) {
  const uint32_t A = t->n_areas, G = t->n_global;
  if (!t->gid) return "select areas: null gid";
  for (uint32_t a = 0; a < A; ++a)
    if (Va[a] && !t->gid[a]) return "select areas: null gid of an area";
  lid.assign((size_t)A * G, ospf_selareas::kNone);
  std::vector<uint8_t> held(G, 0);
  for (uint32_t a = 0; a < A; ++a) {
    const uint32_t V = Va[a];
    for (uint32_t i = 0; i < V; ++i) {
      const uint32_t g = t->gid[a][i];
      if (g >= G) return "select areas: a gid >= n_global";
      if (i && g <= t->gid[a][i - 1]) return "select areas: gid not strictly ascending";
      lid[(size_t)a * G + g] = i;
      held[g] = 1;
    }
  }
  for (uint32_t g = 0; g < G; ++g)
    if (!held[g]) return "select areas: a global id no area holds";
  const uint32_t P = t->n_prefixes;
  if (!P) return nullptr;
  if (!t->offsets) return "select areas: null offsets";
  if (t->offsets[0] != 0) return "select areas: offsets[0] != 0";
  for (uint32_t p = 0; p < P; ++p)
    if (t->offsets[p + 1] < t->offsets[p]) return "select areas: offsets not monotone";
  const uint32_t E = t->offsets[P];
  if (E && (!t->node || !t->area)) return "select areas: null node / area";
  if (E && !t->pref) return "select areas: null pref";
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t k = t->offsets[p]; k < t->offsets[p + 1]; ++k) {
      if (t->area[k] >= A) return "select areas: an area >= n_areas";
      if (t->node[k] >= G) return "select areas: a node >= n_global";
      if (lid[(size_t)t->area[k] * G + t->node[k]] == ospf_selareas::kNone)
        return "select areas: an entry's node is absent from its area";
      if (k > t->offsets[p] &&
          (t->node[k] < t->node[k - 1] ||
           (t->node[k] == t->node[k - 1] && t->area[k] <= t->area[k - 1])))
        return "select areas: entries not strictly ascending in (node, area)";
      if (t->pref[k] >= 0x80000000u) return "select areas: a pref >= 2^31";
    }
  return nullptr;
}

namespace {

bool any_out(const ospf_areas_table* t, const ospf_areas_pout* o) {
  if (o->metric || o->count || o->links || o->need || o->best || o->areas) return true;
  if (o->nh)
    for (uint32_t a = 0; a < t->n_areas; ++a)
      if (o->nh[a]) return true;
  return false;
}

}  // namespace

int ospf_int::selst::area_rows(ospf_sweep* s) {
  if (s->d_area_rows) return OSPF_OK;
  std::vector<ospf_int::SelRow> h(s->V);
  for (uint32_t v = 0; v < s->V; ++v)
    h[v] = ospf_int::SelRow{s->row_dist[v], s->row_nh[v], s->row_w[v], 0u};
  ospf_int::SelRow* d = nullptr;
  if (const int rc = ospf_int::sweep::upload(s, &d, h)) return rc;
  s->d_area_rows = d;
  return OSPF_OK;
}

namespace {

// the fault-injection hook of every area's context, as each area's own call
// would take it
int areas_injected(const ospf_areas_table* t) {
  for (uint32_t a = 0; a < t->n_areas; ++a)
    if (ospf_int::injected(t->sweeps[a]->c)) {
      const std::string m = t->sweeps[a]->c->err;
      return sfail(t->sweeps[0], OSPF_E_DEVICE, m);
    }
  return OSPF_OK;
}

bool areas_args_ok(const ospf_areas_table* t, const ospf_areas_pout* o) {
  if (!t || !o || !t->sweeps || !t->sweeps[0]) return false;
  if (t->n_areas == 0 || t->n_areas > kMaxAreas)
    return sfail(t->sweeps[0], OSPF_E_INVAL, "select areas: n_areas outside 1 .. 32"), false;
  for (uint32_t a = 0; a < t->n_areas; ++a)
    if (!t->sweeps[a]) return sfail(t->sweeps[0], OSPF_E_INVAL, "select areas: a null sweep"), false;
  return true;
}

// ospf_areas_select_policy_dev without the argument checks and the hook.
// `checked`: lid of a contract check the caller already made (else made here).
int areas_queue(const ospf_areas_table* t, const ospf_areas_pout* d_out, void* stream,
                const std::vector<uint32_t>* checked = nullptr) {
  ospf_sweep* s0 = t->sweeps[0];
  const uint32_t A = t->n_areas, G = t->n_global, P = t->n_prefixes;
  std::vector<uint32_t> own;
  if (!checked)
    if (const char* bad = areas_check(t, d_out, own)) return sfail(s0, OSPF_E_INVAL, bad);
  const std::vector<uint32_t>& lid = checked ? *checked : own;
  if (!G || !P || !any_out(t, d_out)) return OSPF_OK;
  ospf_ctx* c0 = s0->c;
  SCHK(s0, hipSetDevice(c0->device));
  for (uint32_t a = 0; a < A; ++a)
    if (const int rc = area_rows(t->sweeps[a]))
      return sfail(s0, rc, t->sweeps[a]->err);
  // LDS: build_links' two words per slot of the widest root, then the u16
  // counts of one root's areas, the largest sum over the roots
  uint32_t capmax = 1, sumcap = 0;
  {
    std::vector<uint32_t> sum(G, 0);
    for (uint32_t a = 0; a < A; ++a) {
      const ospf_ctx* c = t->sweeps[a]->c;
      const uint32_t cap = std::max(1u, c->max_dn), V = t->sweeps[a]->V;
      capmax = std::max(capmax, cap);
      const bool known = c->h_dn_off.size() == (size_t)V + 1;
      for (uint32_t i = 0; i < V; ++i)
        sum[t->gid[a][i]] += known ? std::min(cap, c->h_dn_off[i + 1] - c->h_dn_off[i]) : cap;
    }
    for (uint32_t g = 0; g < G; ++g) sumcap = std::max(sumcap, sum[g]);
  }
  const size_t lds = d_out->links ? (size_t)capmax * 8 + (((size_t)sumcap * 2 + 3) & ~(size_t)3) : 0;
  if (lds > c0->lds_limit)
    return sfail(s0, OSPF_E_RANGE, "select areas: the widest root's link counts do not fit the LDS");
  // the call's device block: the areas, lid [A][G], then the table (offsets,
  // node, area, loc, pref, min_nexthop). The block is the last call's, free
  // once that call's kernel is done.
  const size_t E = t->offsets[P];
  const size_t areas_words = (sizeof(AreaDev) * A + 3) / 4;
  const size_t words = areas_words + (size_t)A * G + (size_t)P + 1 + 5 * E;
  std::vector<uint32_t> h(words, 0);
  if (s0->areas_ev) SCHK(s0, hipEventSynchronize(s0->areas_ev));
  if (words * 4 > s0->areas_blob_bytes) {
    if (s0->d_areas_blob) SCHK(s0, hipFree(s0->d_areas_blob));
    s0->d_areas_blob = nullptr;
    s0->areas_blob_bytes = 0;
    void* q = nullptr;
    if (hipMalloc(&q, words * 4) != hipSuccess) {
      (void)hipGetLastError();
      return sfail(s0, OSPF_E_NOMEM, "select areas: hipMalloc of the call's block");
    }
    s0->d_areas_blob = q;
    s0->areas_blob_bytes = words * 4;
  }
  uint32_t* d = (uint32_t*)s0->d_areas_blob;
  uint32_t* d_lid = d + areas_words;
  uint32_t* d_off = d_lid + (size_t)A * G;
  uint32_t* d_node = d_off + P + 1;
  uint32_t* d_area = d_node + E;
  uint32_t* d_loc = d_area + E;
  uint32_t* d_pref = d_loc + E;
  uint32_t* d_mnh = d_pref + E;
  AreaDev* ha = reinterpret_cast<AreaDev*>(h.data());
  for (uint32_t a = 0; a < A; ++a) {
    const ospf_sweep* s = t->sweeps[a];
    const ospf_ctx* c = s->c;
    AreaDev& x = ha[a];
    x.rows = s->d_area_rows;
    x.lid = d_lid + (size_t)a * G;
    x.nt_bits = c->g.nt_bits;
    x.row_ptr = c->g.row_ptr;
    x.colx = c->g.colx;
    x.w = c->g.w;
    x.didx = c->g.didx;
    x.dn_off = c->g.dn_off;
    x.o_nh = d_out->nh ? d_out->nh[a] : nullptr;
    x.Wout = x.o_nh ? d_out->nh_words[a] : 1u;
    x.cap = std::max(1u, c->max_dn);
  }
  uint32_t* hp = h.data() + areas_words;
  std::copy(lid.begin(), lid.end(), hp);
  hp += (size_t)A * G;
  std::copy(t->offsets, t->offsets + P + 1, hp);
  hp += P + 1;
  if (E) {
    std::copy(t->node, t->node + E, hp);
    std::copy(t->area, t->area + E, hp + E);
    for (size_t k = 0; k < E; ++k) hp[2 * E + k] = lid[(size_t)t->area[k] * G + t->node[k]];
    std::copy(t->pref, t->pref + E, hp + 3 * E);
    if (t->min_nexthop) std::copy(t->min_nexthop, t->min_nexthop + E, hp + 4 * E);
  }
  SCHK(s0, hipMemcpy(d, h.data(), words * 4, hipMemcpyHostToDevice));
  if (!s0->areas_ev) SCHK(s0, hipEventCreateWithFlags(&s0->areas_ev, hipEventDisableTiming));
  AreasArgs k{};
  k.areas = reinterpret_cast<const AreaDev*>(d);
  k.A = A;
  k.G = G;
  k.P = P;
  k.hop = (s0->opts.flags & OSPF_HOP_COUNT) ? 1u : 0u;
  k.capmax = capmax;
  k.sumcap = sumcap;
  k.t = Tab{d_off, d_node, d_area, d_loc, d_pref, t->min_nexthop && E ? d_mnh : nullptr};
  k.o_metric = d_out->metric;
  k.o_count = d_out->count;
  k.o_links = d_out->links;
  k.o_need = d_out->need;
  k.o_best = d_out->best;
  k.o_areas = d_out->areas;
  // a wave per 64 prefixes of the root, at most 4; roots beyond the grid by stride
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  const uint32_t grid = std::min(G, 1u << 20);
  hipLaunchKernelGGL(areas_kernel, dim3(grid), dim3(64u * waves), lds, (hipStream_t)stream, k);
  SCHK(s0, hipGetLastError());
  SCHK(s0, hipEventRecord(s0->areas_ev, (hipStream_t)stream));
  return OSPF_OK;
}

// device outputs of one call (only the wanted ones), freed by the destructor
struct AreasOut {
  std::vector<uint32_t*> all;
  uint32_t* hdr[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<uint32_t*> nh;
  ~AreasOut() {
    for (uint32_t* p : all) (void)hipFree(p);
  }
  bool get(uint32_t** p, size_t words) {
    if (hipMalloc((void**)p, std::max<size_t>(words, 1) * 4) != hipSuccess) return false;
    all.push_back(*p);
    return true;
  }
};

}  // namespace

extern "C" {

int ospf_areas_select_policy_dev(const ospf_areas_table* t, const ospf_areas_pout* d_out,
                                 void* stream) {
  if (!areas_args_ok(t, d_out)) return OSPF_E_INVAL;
  if (const int rc = areas_injected(t)) return rc;
  return areas_queue(t, d_out, stream);
}

int ospf_areas_select_policy(const ospf_areas_table* t, const ospf_areas_pout* out) {
  if (!areas_args_ok(t, out)) return OSPF_E_INVAL;
  if (const int rc = areas_injected(t)) return rc;
  ospf_sweep* s0 = t->sweeps[0];
  const uint32_t A = t->n_areas;
  const size_t cells = (size_t)t->n_global * t->n_prefixes;
  // the contract first: nothing is allocated, copied or written on error
  std::vector<uint32_t> lid;
  if (const char* bad = areas_check(t, out, lid)) return sfail(s0, OSPF_E_INVAL, bad);
  if (!cells) return OSPF_OK;
  SCHK(s0, hipSetDevice(s0->c->device));
  SCHK(s0, hipDeviceSynchronize());  // the rows, whichever streams ran the sweeps
  AreasOut d;
  uint32_t* const want[6] = {out->metric, out->count, out->links, out->need, out->best, out->areas};
  bool ok = true;
  for (int i = 0; i < 6 && ok; ++i)
    if (want[i]) ok = d.get(&d.hdr[i], cells);
  d.nh.assign(A, nullptr);
  std::vector<size_t> nh_words(A, 0);
  for (uint32_t a = 0; a < A && ok; ++a)
    if (out->nh && out->nh[a]) {
      nh_words[a] = (size_t)t->sweeps[a]->V * t->n_prefixes * out->nh_words[a];
      ok = d.get(&d.nh[a], nh_words[a]);
    }
  if (!ok) {
    (void)hipGetLastError();
    return sfail(s0, OSPF_E_NOMEM, "select areas: hipMalloc of the outputs");
  }
  const ospf_areas_pout dev{d.hdr[0], d.hdr[1], d.hdr[2], d.hdr[3], d.hdr[4], d.hdr[5],
                            out->nh ? d.nh.data() : nullptr, out->nh_words};
  if (const int rc = areas_queue(t, &dev, nullptr, &lid)) return rc;
  // into buffers of this call first: a failed copy leaves the caller's as they were
  std::vector<std::vector<uint32_t>> h(6 + A);
  for (int i = 0; i < 6; ++i)
    if (d.hdr[i]) {
      h[i].resize(cells);
      SCHK(s0, hipMemcpy(h[i].data(), d.hdr[i], cells * 4, hipMemcpyDeviceToHost));
    }
  for (uint32_t a = 0; a < A; ++a)
    if (d.nh[a] && nh_words[a]) {
      h[6 + a].resize(nh_words[a]);
      SCHK(s0, hipMemcpy(h[6 + a].data(), d.nh[a], nh_words[a] * 4, hipMemcpyDeviceToHost));
    }
  for (int i = 0; i < 6; ++i)
    if (d.hdr[i]) std::copy(h[i].begin(), h[i].end(), want[i]);
  for (uint32_t a = 0; a < A; ++a)
    if (d.nh[a]) std::copy(h[6 + a].begin(), h[6 + a].end(), out->nh[a]);
  return OSPF_OK;
}

}  // extern "C"
