// spf_seldelta_areas.hip — the multi-area route selections a re-sweep of some
// areas (or a change of the entries' attributes) changed, on the device
// (gfx950): DecisionRouteDb::calculateUpdate (openr/decision/SpfSolver.cpp:
// 24-59) over the routes createRouteForPrefix (:197-458) produces across
// areas, i.e. ospf_areas_select_policy's route DB kept resident.
//
// An ospf_areastate keeps per global root g, by global id, a block metric[P],
// count[P], links[P], need[P], best[P], areas[P], then for every area a that
// holds g (in area order) nh_a[P][W_a(g)] in the root's own width there (SoA,
// no padding), in two buffers, and every area's distinct-neighbour lists.
// areas_delta_kernel computes the sweeps' selection with areas_kernel's
// per-prefix device functions (spf_selareas_dev.h), stores it into the shadow
// buffer, compares it with the committed cell and appends what differs to a
// change list; the host commits by swapping.
//
// Shape: areas_kernel's -- a workgroup per global root (grid-stride), the
// root's per-area records and packed link counts in LDS (nothing beyond
// areas_kernel's), waves striding over chunks of 64 prefixes, the lane / wave /
// word strategies by the same predicates. Per chunk: the new cell; its store
// (the six columns one coalesced store each, an area of <= kSelLaneW words
// through store_chunk_words, a wider one by area_by_words, a lane per word);
// the committed cell loaded the same way; the comparison (in the prefix's lane,
// or for a wide area in the lanes that wrote the words, a ballot making the
// verdict the wave's); the chunk's changed cells' list positions from ONE
// atomicAdd of the wave. The counters always count; a record is written only
// below the caller's capacity. A record is two 16-B stores: {root, prefix,
// metric, count}, {links, need, best, areas}; its next-hop row is copied from
// the shadow cell by the wave.
// The rebase test runs per wave and per area of the root, as seldelta_kernel
// does it (every wave compares the lists itself: no LDS, no barrier). A
// committed cell sits at the same place of its block as the new one: a root
// whose width changed in any area is rebased and not compared.
// Every shadow word is written once by plain vector stores; no memset of the
// buffers, no scratch, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "spf_selareas_dev.h"
#include "spf_selstate.h"
#include "sweep_impl.h"

// ---------------------------------------------------------------- the state
struct ospf_areastate {
  ospf_ctx* c = nullptr;  // area 0's context; null once any of them was closed
  std::string err;
  uint32_t A = 0, G = 0, P = 0;
  std::vector<ospf_ctx*> ctx;  // [A]
  std::vector<uint32_t> V;     // [A]
  std::vector<uint32_t> lid;   // [A][G] global id -> node id
  // the table's copy; t_loc: the entry's node id in its own area (t_mnh empty:
  // all unset)
  std::vector<uint32_t> t_off, t_node, t_area, t_loc, t_pref, t_mnh;
  // lid, offsets, node, area, loc, pref, min_nexthop
  uint32_t* d_tab = nullptr;
  void* d_areas = nullptr;  // the call's per-area records [A]
  bool primed = false;
  int cur = 0;  // the committed buffer
  struct Buf {
    uint32_t* data = nullptr;  // the root blocks
    size_t data_words = 0;     // allocated
    uint64_t* off = nullptr;   // [G] block offset (words) by global id
    uint32_t* w = nullptr;     // [A][G] next-hop words (0: the area does not hold the root)
    uint32_t* dn_off = nullptr;  // the areas' [V_a + 1] one after the other
    uint32_t* dn = nullptr;      // the areas' lists one after the other
    size_t dn_words = 0;         // allocated
    std::vector<uint64_t> h_off;
    std::vector<uint32_t> h_w;
    std::vector<size_t> h_dnb;  // [A] where area a's list starts in dn
  } b[2];
  uint32_t* d_cnt = nullptr;  // [2]
  uint4* d_chg = nullptr;     // change records, two uint4 each
  uint32_t* d_chg_nh = nullptr;
  uint32_t* d_reb = nullptr;
  size_t chg_cap = 0, chg_nh_words = 0, reb_cap = 0;
  uint64_t device_bytes = 0;
};

namespace {

using namespace ospf_selareas;
using ospf_selareas::kNone;  // not ospf_int::sweep's

// one area as the kernel sees it (device memory, [n_areas])
struct DArea {
  const ospf_int::SelRow* rows;  // [V_a] by node id
  const uint32_t* lid;           // [G] global id -> node id, kNone: absent
  const uint32_t* nt_bits;       // the loaded graph
  const uint32_t* row_ptr;
  const uint32_t* colx;
  const uint32_t* w;
  const uint16_t* didx;
  const uint32_t* n_dn_off;  // the graph's distinct-neighbour lists (the shadow buffer's copy)
  const uint32_t* n_dn;
  const uint32_t* o_dn_off;  // the committed ones, and the committed widths [G]
  const uint32_t* o_dn;
  const uint32_t* o_w;
  uint32_t cap;              // LDS slots while the links are built
  uint32_t nh_base, nh_words;  // the area's words within a record's next-hop row
};

struct AdArgs {
  const DArea* areas;
  uint32_t A, G, P, hop;
  uint32_t capmax;  // LDS slots of the widest root of any area
  uint32_t sumcap;  // u16 link counts behind them: the largest sum over a root's areas
  Tab t;
  uint32_t* n_data;  // the shadow buffer (written): root blocks at n_off[g] words
  const uint64_t* n_off;
  const uint32_t* o_data;  // the committed one (null: prime, nothing compared)
  const uint64_t* o_off;
  uint32_t* counters;  // [0] changed cells, [1] rebased roots
  uint4* changes;      // ospf_areas_change records, two uint4 each
  uint32_t* chg_nh;    // [chg_cap][nh_total] or null
  uint32_t nh_total, chg_cap;
  uint32_t* rebased;
  uint32_t cap_rebased;
};

__global__ __launch_bounds__(256) void areas_delta_kernel(const AdArgs a) {
  extern __shared__ uint32_t lds[];
  __shared__ RootArea ra[kMaxAreas];
  __shared__ uint32_t s_wide;
  // the link counts: build_links' 2 * capmax words, then the packed u16 counts
  // of the root's areas
  uint16_t* cpack = reinterpret_cast<uint16_t*>(lds + 2u * a.capmax);
  const uint16_t* cslot = cpack;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P, A = a.A;
  for (uint32_t g = blockIdx.x; g < a.G; g += gridDim.x) {
    __syncthreads();  // the previous root's areas are read no more
    if (threadIdx.x < A) {
      const DArea& ad = a.areas[threadIdx.x];
      RootArea x{};
      x.lid = ad.lid;
      x.nt = ad.nt_bits;
      x.la = ad.lid[g];
      if (x.la != kNone) {
        const ospf_int::SelRow row = ad.rows[x.la];
        x.dist = row.dist;
        x.nh = row.nh;
        x.W = row.W;
        x.Wout = row.W;  // the resident words are in the root's own width
        x.ns = min(ad.n_dn_off[x.la + 1] - ad.n_dn_off[x.la], ad.cap);
      }
      ra[threadIdx.x] = x;
    }
    __syncthreads();
    uint32_t* n_blk = a.n_data + a.n_off[g];
    if (threadIdx.x == 0) {
      uint32_t off = 0, wide = 0;
      uint32_t* words = n_blk + 6 * (size_t)P;  // the areas' words behind the six columns
      for (uint32_t ar = 0; ar < A; ++ar) {
        if (ra[ar].la == kNone) continue;
        ra[ar].ns = min(ra[ar].ns, a.sumcap - off);  // the host sized sumcap for every root
        ra[ar].coff = off;
        off += ra[ar].ns;
        wide |= ra[ar].W > kSelLaneW ? 1u : 0u;
        ra[ar].o_nh = words;
        words += (size_t)P * ra[ar].W;
      }
      s_wide = wide;
    }
    __syncthreads();
    for (uint32_t ar = 0; ar < A; ++ar) {  // block-uniform
      if (ra[ar].la == kNone) continue;
      const DArea& ad = a.areas[ar];
      const LinkArgs la{ad.row_ptr, ad.colx, ad.w, ad.didx, a.hop, a.capmax};
      const uint32_t ns = ra[ar].ns;
      build_links(la, ra[ar].la, ns, lds);
      const uint16_t* c16 = reinterpret_cast<const uint16_t*>(lds);
      for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) cpack[ra[ar].coff + i] = c16[i];
    }
    __syncthreads();
    bool cmp = a.o_data != nullptr;
    if (cmp) {
      // the root's distinct neighbours then and now in each of its areas (each
      // wave the whole lists)
      bool diff = false;
      for (uint32_t ar = 0; ar < A; ++ar) {  // wave-uniform
        const uint32_t la = ra[ar].la;
        if (la == kNone) continue;
        const DArea& ad = a.areas[ar];
        const uint32_t olo = ad.o_dn_off[la], ocnt = ad.o_dn_off[la + 1] - olo;
        const uint32_t nlo = ad.n_dn_off[la], ncnt = ad.n_dn_off[la + 1] - nlo;
        if (ocnt != ncnt || ad.o_w[g] != ra[ar].W) diff = true;
        else
          for (uint32_t k = lane; k < ncnt; k += 64) diff |= ad.o_dn[olo + k] != ad.n_dn[nlo + k];
      }
      if (__ballot(diff)) {  // rebased: listed once, nothing compared
        cmp = false;
        if (threadIdx.x == 0) {
          const uint32_t i = atomicAdd(&a.counters[1], 1u);
          if (i < a.cap_rebased) a.rebased[i] = g;
        }
      }
    }
    // the committed block: its columns and words lie as the new ones do (the
    // widths are the same, or the root was rebased)
    const uint32_t* o_blk = cmp ? a.o_data + a.o_off[g] : nullptr;
    const bool root_wide = s_wide != 0u;
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
      bool ch = false;  // this lane's cell differs from the committed one
      for (uint32_t ar = 0; ar < A; ++ar) {  // wave-uniform
        const RootArea& x = ra[ar];
        if (x.la == kNone) continue;
        const uint32_t* o_words = cmp ? o_blk + (x.o_nh - n_blk) : nullptr;
        if (x.W <= kSelLaneW) {
          uint32_t acc[kSelLaneW];
#pragma unroll
          for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
          if (mine && ((s.win >> ar) & 1u)) area_by_lane(a.t, x, ar, lo, s, true, cnt, acc);
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
            area_by_wave(a.t, ra, ar, lane_get(lo, j), lane_get(hi, j), ws, lane, true, wc, wa);
            if (lane == j) {
              cnt += wc;
#pragma unroll
              for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = wa[w];
            }
          }
          links += links_of(acc, x.W, cslot + x.coff, x.ns);
          store_chunk_words(x.o_nh + (size_t)base * x.W, !((uintptr_t)x.o_nh & 15u), acc, x.W, x.W,
                            n, lane, in);
          if (cmp && in) {
            const uint32_t* ow = o_words + (size_t)p * x.W;
#pragma unroll
            for (uint32_t w = 0; w < kSelLaneW; ++w)
              if (w < x.W) ch |= ow[w] != acc[w];
          }
        } else {
          // a wide area: the root is wide, so every prefix is the wave's
          for (uint32_t j = 0; j < n; ++j) {
            Sel ws;
            ws.m = lane_get(s.m, j);
            ws.win = lane_get(s.win, j);
            ws.cls = lane_get(s.cls, j);
            uint32_t wc = 0;
            uint32_t* dstw = x.o_nh + (size_t)(base + j) * x.W;
            const uint32_t wl = area_by_words(a.t, ra, ar, lane_get(lo, j), lane_get(hi, j), ws,
                                              lane, dstw, cslot, true, wc);
            bool diff = false;
            if (cmp) {  // each lane the words it has just written
              const uint32_t* ow = o_words + (size_t)(base + j) * x.W;
              for (uint32_t w = lane; w < x.W; w += 64) diff |= dstw[w] != ow[w];
            }
            const bool any = __ballot(diff) != 0ull;
            if (lane == j) {
              cnt += wc;
              links += wl;
              ch |= any;
            }
          }
        }
      }
      if (in) {
        n_blk[p] = s.m;
        n_blk[(size_t)P + p] = cnt;
        n_blk[2 * (size_t)P + p] = links;
        n_blk[3 * (size_t)P + p] = s.need;
        n_blk[4 * (size_t)P + p] = s.best;
        n_blk[5 * (size_t)P + p] = s.win;
        if (cmp)
          ch |= o_blk[p] != s.m || o_blk[(size_t)P + p] != cnt ||
                o_blk[2 * (size_t)P + p] != links || o_blk[3 * (size_t)P + p] != s.need ||
                o_blk[4 * (size_t)P + p] != s.best || o_blk[5 * (size_t)P + p] != s.win;
      }
      // append the chunk's changed cells: one atomicAdd of the wave
      const unsigned long long mask = __ballot(ch);
      if (mask) {
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t b0 = 0;
        if (lane == leader) b0 = atomicAdd(&a.counters[0], (uint32_t)__popcll(mask));
        b0 = lane_get(b0, leader);
        const uint32_t idx = b0 + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (ch && idx < a.chg_cap) {
          a.changes[2 * (size_t)idx] = make_uint4(g, p, s.m, cnt);
          a.changes[2 * (size_t)idx + 1] = make_uint4(links, s.need, s.best, s.win);
        }
        if (a.chg_nh) {
          // a record's row by the wave, from the shadow cell: a narrow area's
          // words were stored by other lanes of this wave, so the stores are
          // made visible to the workgroup first
          __threadfence_block();
          for (unsigned long long t = mask; t; t &= t - 1ull) {
            const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
            const uint32_t ij = lane_get(idx, j);
            if (ij >= a.chg_cap) continue;
            uint32_t* o = a.chg_nh + (size_t)ij * a.nh_total;
            for (uint32_t ar = 0; ar < A; ++ar) {
              const DArea& ad = a.areas[ar];
              const RootArea& x = ra[ar];
              const uint32_t W = x.la == kNone ? 0u : x.W;
              const uint32_t* src = W ? x.o_nh + (size_t)(base + j) * W : nullptr;
              for (uint32_t w = lane; w < ad.nh_words; w += 64)
                o[ad.nh_base + w] = w < W ? src[w] : 0u;
            }
          }
        }
      }
    }
  }
}

using namespace ospf_int;
using namespace ospf_int::selst;

void release(ospf_areastate* st) {
  if (!st->c) return;
  (void)hipSetDevice(st->c->device);
  (void)hipDeviceSynchronize();
  for (auto& b : st->b) {
    (void)hipFree(b.data);
    (void)hipFree(b.off);
    (void)hipFree(b.w);
    (void)hipFree(b.dn_off);
    (void)hipFree(b.dn);
    b = ospf_areastate::Buf{};
  }
  (void)hipFree(st->d_tab);
  (void)hipFree(st->d_areas);
  (void)hipFree(st->d_cnt);
  (void)hipFree(st->d_chg);
  (void)hipFree(st->d_chg_nh);
  (void)hipFree(st->d_reb);
  st->d_tab = st->d_cnt = st->d_chg_nh = st->d_reb = nullptr;
  st->d_areas = nullptr;
  st->d_chg = nullptr;
  st->chg_cap = st->chg_nh_words = st->reb_cap = 0;
  st->device_bytes = 0;
  st->primed = false;
}

// off every context's list; the state is dead to all of them
void detach(ospf_areastate* st) {
  for (ospf_ctx* c : st->ctx) {
    auto& l = c->live_areastates;
    l.erase(std::remove(l.begin(), l.end(), st), l.end());
  }
  st->ctx.clear();
  st->c = nullptr;
}

constexpr const char* kClosed = "areastate: a context of the state was closed";

// the fault-injection hook of every area's context, each context once (two
// areas on one context count one call)
int hooked(ospf_areastate* st) {
  for (size_t a = 0; a < st->ctx.size(); ++a) {
    ospf_ctx* c = st->ctx[a];
    if (std::find(st->ctx.begin(), st->ctx.begin() + a, c) != st->ctx.begin() + a) continue;
    if (injected(c)) return stfail(st, OSPF_E_DEVICE, std::string(c->err));
  }
  return OSPF_OK;
}

// what makes `sweeps` unusable for the state (null: usable)
const char* sweeps_error(const ospf_areastate* st, ospf_sweep* const* sweeps) {
  for (uint32_t a = 0; a < st->A; ++a)
    if (!sweeps[a]) return "areastate: a null sweep";
  for (uint32_t a = 0; a < st->A; ++a) {
    const ospf_sweep* s = sweeps[a];
    if (s->c != st->ctx[a]) return "areastate: a sweep belongs to another context than its area's";
    if (const char* bad = areas_sweep_error(s, sweeps[0])) return bad;
    if (s->V != st->V[a]) return "areastate: an area's graph has another node count";
    if (st->ctx[a]->h_dn_off.size() != (size_t)s->V + 1)
      return "areastate: an area's distinct-neighbour lists are not loaded";
  }
  return nullptr;
}

// the pref / min_nexthop columns' contract for E entries
const char* columns_error(size_t E, const uint32_t* pref) {
  if (E && !pref) return "select areas: null pref";
  for (size_t k = 0; k < E; ++k)
    if (pref[k] >= 0x80000000u) return "select areas: a pref >= 2^31";
  return nullptr;
}

// the sweeps' selection into the shadow buffer; with `compare` the cells that
// differ from the committed buffer's and the rebased roots are listed (up to
// the caps) and counted. Nothing is committed.
int write_shadow(ospf_areastate* st, ospf_sweep* const* sweeps, bool compare,
                 const uint32_t* nh_words, bool want_nh, uint32_t cap, uint32_t cap_reb,
                 uint32_t counts[2]) {
  ospf_ctx* c0 = st->c;
  const uint32_t A = st->A, G = st->G, P = st->P;
  ospf_areastate::Buf& nb = st->b[st->cur ^ 1];
  const ospf_areastate::Buf& ob = st->b[st->cur];
  counts[0] = counts[1] = 0;
  STCHK(st, hipSetDevice(c0->device));
  STCHK(st, hipDeviceSynchronize());  // the rows, whichever streams ran the sweeps
  for (uint32_t a = 0; a < A; ++a)
    if (const int rc = area_rows(sweeps[a])) return stfail(st, rc, "areastate: " + sweeps[a]->err);
  // block offsets by global id, in these sweeps' widths; the LDS the widest
  // root needs (build_links' two words per slot, then the u16 counts of one
  // root's areas, the largest sum over the roots)
  nb.h_off.resize(G);
  nb.h_w.assign((size_t)A * G, 0u);
  uint64_t words = 0;
  uint32_t capmax = 1, sumcap = 0;
  size_t dn_total = 0;
  for (uint32_t a = 0; a < A; ++a) {
    capmax = std::max(capmax, std::max(1u, st->ctx[a]->max_dn));
    dn_total += st->ctx[a]->h_dn.size();
  }
  for (uint32_t g = 0; g < G; ++g) {
    nb.h_off[g] = words;
    uint64_t wsum = 0;
    uint32_t slots = 0;
    for (uint32_t a = 0; a < A; ++a) {
      const uint32_t la = st->lid[(size_t)a * G + g];
      if (la == kNone) continue;
      const ospf_ctx* c = st->ctx[a];
      nb.h_w[(size_t)a * G + g] = sweeps[a]->row_w[la];
      wsum += sweeps[a]->row_w[la];
      slots += std::min(std::max(1u, c->max_dn), c->h_dn_off[la + 1] - c->h_dn_off[la]);
    }
    sumcap = std::max(sumcap, slots);
    words += (uint64_t)P * (6u + wsum);
  }
  const size_t lds = (size_t)capmax * 8 + (((size_t)sumcap * 2 + 3) & ~(size_t)3);
  if (lds > c0->lds_limit)
    return stfail(st, OSPF_E_RANGE, "areastate: the widest root's link counts do not fit the LDS");
  int rc;
  if ((rc = grow(st, &nb.data, &nb.data_words, words))) return rc;
  if ((rc = grow(st, &nb.dn, &nb.dn_words, dn_total))) return rc;
  STCHK(st, hipMemcpy(nb.off, nb.h_off.data(), (size_t)G * 8, hipMemcpyHostToDevice));
  if (G) STCHK(st, hipMemcpy(nb.w, nb.h_w.data(), (size_t)A * G * 4, hipMemcpyHostToDevice));
  // the areas' lists one after the other: dn_off at the same place in every
  // version (V_a is the state's), dn where this version's lists put it
  std::vector<size_t> dno(A);
  nb.h_dnb.resize(A);
  {
    size_t o = 0, d = 0;
    for (uint32_t a = 0; a < A; ++a) {
      const ospf_ctx* c = st->ctx[a];
      dno[a] = o;
      nb.h_dnb[a] = d;
      STCHK(st, hipMemcpy(nb.dn_off + o, c->h_dn_off.data(), ((size_t)st->V[a] + 1) * 4,
                          hipMemcpyHostToDevice));
      if (!c->h_dn.empty())
        STCHK(st, hipMemcpy(nb.dn + d, c->h_dn.data(), c->h_dn.size() * 4, hipMemcpyHostToDevice));
      o += (size_t)st->V[a] + 1;
      d += c->h_dn.size();
    }
  }
  uint32_t nh_total = 0;
  std::vector<DArea> ha(A);
  for (uint32_t a = 0; a < A; ++a) {
    const ospf_ctx* c = st->ctx[a];
    DArea& x = ha[a];
    x.rows = sweeps[a]->d_area_rows;
    x.lid = st->d_tab + (size_t)a * G;
    x.nt_bits = c->g.nt_bits;
    x.row_ptr = c->g.row_ptr;
    x.colx = c->g.colx;
    x.w = c->g.w;
    x.didx = c->g.didx;
    x.n_dn_off = nb.dn_off + dno[a];
    x.n_dn = nb.dn + nb.h_dnb[a];
    if (compare) {
      x.o_dn_off = ob.dn_off + dno[a];
      x.o_dn = ob.dn + ob.h_dnb[a];
      x.o_w = ob.w + (size_t)a * G;
    }
    x.cap = std::max(1u, c->max_dn);
    x.nh_base = nh_total;
    x.nh_words = want_nh ? nh_words[a] : 0u;
    nh_total += x.nh_words;
  }
  STCHK(st, hipMemcpy(st->d_areas, ha.data(), sizeof(DArea) * A, hipMemcpyHostToDevice));
  if (compare) {
    if ((rc = grow(st, &st->d_chg, &st->chg_cap, (size_t)cap * 2u))) return rc;  // two uint4 each
    if (want_nh && (rc = grow(st, &st->d_chg_nh, &st->chg_nh_words, (size_t)cap * nh_total)))
      return rc;
    if ((rc = grow(st, &st->d_reb, &st->reb_cap, cap_reb))) return rc;
  }
  const uint32_t zero[2] = {0, 0};
  STCHK(st, hipMemcpy(st->d_cnt, zero, sizeof(zero), hipMemcpyHostToDevice));
  if (!G || !P) return OSPF_OK;  // no cell: nothing to store or compare
  const size_t E = st->t_node.size();
  uint32_t* d_off = st->d_tab + (size_t)A * G;
  uint32_t* d_node = d_off + P + 1;
  AdArgs k{};
  k.areas = reinterpret_cast<const DArea*>(st->d_areas);
  k.A = A;
  k.G = G;
  k.P = P;
  k.hop = (sweeps[0]->opts.flags & OSPF_HOP_COUNT) ? 1u : 0u;
  k.capmax = capmax;
  k.sumcap = sumcap;
  k.t = Tab{d_off, d_node, d_node + E, d_node + 2 * E, d_node + 3 * E,
            st->t_mnh.empty() ? nullptr : d_node + 4 * E};
  k.n_data = nb.data;
  k.n_off = nb.off;
  if (compare) {
    k.o_data = ob.data;
    k.o_off = ob.off;
    k.changes = st->d_chg;
    k.chg_nh = want_nh && nh_total ? st->d_chg_nh : nullptr;
    k.nh_total = nh_total;
    k.chg_cap = cap;
    k.rebased = st->d_reb;
    k.cap_rebased = cap_reb;
  }
  k.counters = st->d_cnt;
  // a wave per 64 prefixes of the root, at most 4; roots beyond the grid by stride
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  hipLaunchKernelGGL(areas_delta_kernel, dim3(std::min(G, 1u << 20)), dim3(64u * waves), lds,
                     nullptr, k);
  STCHK(st, hipGetLastError());
  STCHK(st, hipDeviceSynchronize());
  STCHK(st, hipMemcpy(counts, st->d_cnt, 8, hipMemcpyDeviceToHost));
  return OSPF_OK;
}

}  // namespace

extern "C" {

int ospf_areastate_create(const ospf_areas_table* t, ospf_areastate** out) {
  if (!t || !out || !t->sweeps) return OSPF_E_INVAL;
  *out = nullptr;
  const uint32_t A = t->n_areas;
  if (A == 0 || A > kMaxAreas) return OSPF_E_INVAL;
  for (uint32_t a = 0; a < A; ++a)
    if (!t->sweeps[a] || !t->sweeps[a]->c) return OSPF_E_INVAL;
  ospf_ctx* c0 = t->sweeps[0]->c;
  std::vector<uint32_t> V(A), lid;
  for (uint32_t a = 0; a < A; ++a) {
    const ospf_ctx* c = t->sweeps[a]->c;
    if (!c->loaded) return fail(c0, OSPF_E_NOGRAPH, "no graph loaded");
    if (c->device != c0->device) return fail(c0, OSPF_E_INVAL, "select areas: sweeps on different devices");
    V[a] = t->sweeps[a]->V;
  }
  if (const char* bad = areas_table_error(t, V.data(), lid)) return fail(c0, OSPF_E_INVAL, bad);
  ospf_areastate* st = new (std::nothrow) ospf_areastate();
  if (!st) return OSPF_E_NOMEM;
  st->c = c0;
  st->A = A;
  st->G = t->n_global;
  st->P = t->n_prefixes;
  st->V = V;
  st->lid = lid;
  for (uint32_t a = 0; a < A; ++a) st->ctx.push_back(t->sweeps[a]->c);
  const uint32_t G = st->G, P = st->P;
  if (P) {
    const size_t E = t->offsets[P];
    st->t_off.assign(t->offsets, t->offsets + P + 1);
    if (E) {
      st->t_node.assign(t->node, t->node + E);
      st->t_area.assign(t->area, t->area + E);
      st->t_pref.assign(t->pref, t->pref + E);
      if (t->min_nexthop) st->t_mnh.assign(t->min_nexthop, t->min_nexthop + E);
      st->t_loc.resize(E);
      for (size_t k = 0; k < E; ++k) st->t_loc[k] = lid[(size_t)t->area[k] * G + t->node[k]];
    }
  } else {
    st->t_off.assign(1, 0u);
  }
  auto setup = [&]() -> int {
    STCHK(st, hipSetDevice(c0->device));
    const size_t E = st->t_node.size();
    // lid, offsets, then node / area / loc / pref / min_nexthop
    std::vector<uint32_t> h((size_t)A * G + P + 1 + 5 * E, 0u);
    uint32_t* hp = h.data();
    std::copy(st->lid.begin(), st->lid.end(), hp);
    hp += (size_t)A * G;
    std::copy(st->t_off.begin(), st->t_off.end(), hp);
    hp += P + 1;
    if (E) {
      std::copy(st->t_node.begin(), st->t_node.end(), hp);
      std::copy(st->t_area.begin(), st->t_area.end(), hp + E);
      std::copy(st->t_loc.begin(), st->t_loc.end(), hp + 2 * E);
      std::copy(st->t_pref.begin(), st->t_pref.end(), hp + 3 * E);
      std::copy(st->t_mnh.begin(), st->t_mnh.end(), hp + 4 * E);
    }
    size_t have = 0;
    int rc;
    if ((rc = grow(st, &st->d_tab, &have, h.size()))) return rc;
    STCHK(st, hipMemcpy(st->d_tab, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    DArea* da = nullptr;
    if ((rc = grow(st, &da, &(have = 0), (size_t)A))) return rc;
    st->d_areas = da;
    if ((rc = grow(st, &st->d_cnt, &(have = 0), 2))) return rc;
    size_t dn_offs = 0;
    for (uint32_t a = 0; a < A; ++a) dn_offs += (size_t)st->V[a] + 1;
    for (auto& b : st->b) {
      if ((rc = grow(st, &b.off, &(have = 0), G))) return rc;
      if ((rc = grow(st, &b.w, &(have = 0), (size_t)A * G))) return rc;
      if ((rc = grow(st, &b.dn_off, &(have = 0), dn_offs))) return rc;
    }
    return OSPF_OK;
  };
  if (const int rc = setup()) {
    release(st);
    delete st;
    return rc;
  }
  for (uint32_t a = 0; a < A; ++a) {
    ospf_ctx* c = st->ctx[a];
    auto& l = c->live_areastates;
    if (std::find(l.begin(), l.end(), st) == l.end()) l.push_back(st);
    c->release_areastate = [](ospf_areastate* x) {  // ospf_close: release now, detach
      release(x);
      detach(x);
    };
  }
  *out = st;
  return OSPF_OK;
}

int ospf_areastate_destroy(ospf_areastate* st) {
  if (!st) return OSPF_E_INVAL;
  if (st->c) {
    release(st);
    detach(st);
  }
  delete st;
  return OSPF_OK;
}

const char* ospf_areastate_last_error(const ospf_areastate* st) {
  return st ? st->err.c_str() : "null areas state";
}

uint64_t ospf_areastate_device_bytes(const ospf_areastate* st) { return st ? st->device_bytes : 0; }

int ospf_areastate_prime(ospf_areastate* st, ospf_sweep* const* sweeps) {
  if (!st || !sweeps) return OSPF_E_INVAL;
  if (!st->c) return stfail(st, OSPF_E_INVAL, kClosed);
  if (const int rc = hooked(st)) return rc;
  if (const char* bad = sweeps_error(st, sweeps)) return stfail(st, OSPF_E_INVAL, bad);
  uint32_t counts[2];
  const int rc = write_shadow(st, sweeps, false, nullptr, false, 0, 0, counts);
  if (rc) return rc;
  st->cur ^= 1;
  st->primed = true;
  return OSPF_OK;
}

int ospf_areastate_update(ospf_areastate* st, ospf_sweep* const* sweeps, const uint32_t* nh_words,
                          ospf_areas_change* changes, uint32_t* nh, uint32_t cap,
                          uint32_t* n_changes, uint32_t* rebased_roots, uint32_t cap_rebased,
                          uint32_t* n_rebased) {
  if (!st || !sweeps || !n_changes || !n_rebased || (cap && !changes) ||
      (cap_rebased && !rebased_roots))
    return OSPF_E_INVAL;
  *n_changes = *n_rebased = 0;
  if (!st->c) return stfail(st, OSPF_E_INVAL, kClosed);
  if (const int rc = hooked(st)) return rc;
  if (!st->primed) return stfail(st, OSPF_E_INVAL, "areastate: update before prime");
  if (const char* bad = sweeps_error(st, sweeps)) return stfail(st, OSPF_E_INVAL, bad);
  if (nh && !nh_words) return stfail(st, OSPF_E_INVAL, "areastate: null nh_words");
  uint64_t nh_total = 0;
  if (nh_words)
    for (uint32_t a = 0; a < st->A; ++a) {
      if (nh_words[a] < max_words(sweeps[a]))
        return stfail(st, OSPF_E_INVAL, "areastate: nh_words below a root's next-hop words");
      nh_total += nh_words[a];
    }
  if (nh_total > 0xFFFFFFFFull) return stfail(st, OSPF_E_INVAL, "areastate: nh_words too large");
  uint32_t counts[2];
  const bool want_nh = nh != nullptr && cap != 0 && nh_total != 0;
  const int rc = write_shadow(st, sweeps, true, nh_words, want_nh, cap, cap_rebased, counts);
  if (rc) return rc;
  *n_changes = counts[0];
  *n_rebased = counts[1];
  if (counts[0] > cap || counts[1] > cap_rebased)
    return stfail(st, OSPF_E_RANGE, "areastate: " + std::to_string(counts[0]) + " changes, " +
                                        std::to_string(counts[1]) +
                                        " rebased roots: above the caller's capacity");
  static_assert(sizeof(ospf_areas_change) == 2 * sizeof(uint4), "areas records are two uint4");
  if (counts[0]) {
    STCHK(st, hipMemcpy(changes, st->d_chg, (size_t)counts[0] * sizeof(ospf_areas_change),
                        hipMemcpyDeviceToHost));
    if (want_nh)
      STCHK(st, hipMemcpy(nh, st->d_chg_nh, (size_t)counts[0] * nh_total * 4, hipMemcpyDeviceToHost));
  }
  if (counts[1])
    STCHK(st, hipMemcpy(rebased_roots, st->d_reb, (size_t)counts[1] * 4, hipMemcpyDeviceToHost));
  st->cur ^= 1;  // commit
  return OSPF_OK;
}

int ospf_areastate_copy(ospf_areastate* st, const uint32_t* roots, uint32_t n,
                        const ospf_areas_pout* out) {
  if (!st || (n && !roots) || !out) return OSPF_E_INVAL;
  if (!st->c) return stfail(st, OSPF_E_INVAL, kClosed);
  if (const int rc = hooked(st)) return rc;
  if (!st->primed) return stfail(st, OSPF_E_INVAL, "areastate: copy before prime");
  const ospf_areastate::Buf& b = st->b[st->cur];
  const size_t P = st->P, G = st->G;
  const uint32_t A = st->A;
  bool any_nh = false;
  if (out->nh)
    for (uint32_t a = 0; a < A; ++a) any_nh |= out->nh[a] != nullptr;
  if (any_nh && !out->nh_words) return stfail(st, OSPF_E_INVAL, "areastate: null nh_words");
  for (uint32_t i = 0; i < n; ++i) {
    if (roots[i] >= G) return stfail(st, OSPF_E_INVAL, "areastate: root id outside the global ids");
    for (uint32_t a = 0; any_nh && a < A; ++a)
      if (out->nh[a] && b.h_w[a * G + roots[i]] > out->nh_words[a])
        return stfail(st, OSPF_E_INVAL, "areastate: nh_words below a root's next-hop words");
  }
  uint32_t* const col[6] = {out->metric, out->count, out->links, out->need, out->best, out->areas};
  bool any = any_nh;
  for (int k = 0; k < 6; ++k) any |= col[k] != nullptr;
  if (!n || !P || !any) return OSPF_OK;
  STCHK(st, hipSetDevice(st->c->device));
  // every block off the device first: a failed copy leaves the caller's buffers as they were
  std::vector<std::vector<uint32_t>> blk(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t g = roots[i];
    size_t wsum = 0;
    for (uint32_t a = 0; a < A; ++a) wsum += b.h_w[a * G + g];
    blk[i].resize(P * (6u + wsum));
    STCHK(st, hipMemcpy(blk[i].data(), b.data + b.h_off[g], blk[i].size() * 4, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t g = roots[i];
    for (int k = 0; k < 6; ++k)
      if (col[k]) std::memcpy(col[k] + i * P, blk[i].data() + k * P, P * 4);
    const uint32_t* src = blk[i].data() + 6 * P;
    for (uint32_t a = 0; a < A; ++a) {
      const uint32_t W = b.h_w[a * G + g];
      if (any_nh && out->nh[a]) {
        const size_t Wo = out->nh_words[a];
        uint32_t* dst = out->nh[a] + i * P * Wo;
        std::memset(dst, 0, P * Wo * 4);
        for (size_t p = 0; p < P && W; ++p) std::memcpy(dst + p * Wo, src + p * W, (size_t)W * 4);
      }
      src += P * W;
    }
  }
  return OSPF_OK;
}

int ospf_areastate_set_policy(ospf_areastate* st, const uint32_t* pref, const uint32_t* min_nexthop) {
  if (!st) return OSPF_E_INVAL;
  if (!st->c) return stfail(st, OSPF_E_INVAL, kClosed);
  if (const int rc = hooked(st)) return rc;
  const size_t E = st->t_node.size();
  if (const char* bad = columns_error(E, pref)) return stfail(st, OSPF_E_INVAL, bad);
  if (E) {
    // both columns in one copy: it either replaces them or leaves them
    std::vector<uint32_t> both(2 * E, 0u);
    std::copy(pref, pref + E, both.begin());
    if (min_nexthop) std::copy(min_nexthop, min_nexthop + E, both.begin() + E);
    STCHK(st, hipSetDevice(st->c->device));
    STCHK(st, hipDeviceSynchronize());
    uint32_t* d_pref = st->d_tab + (size_t)st->A * st->G + st->P + 1 + 3 * E;
    STCHK(st, hipMemcpy(d_pref, both.data(), both.size() * 4, hipMemcpyHostToDevice));
    st->t_pref.assign(pref, pref + E);
    if (min_nexthop) st->t_mnh.assign(min_nexthop, min_nexthop + E);
    else st->t_mnh.clear();
  }
  return OSPF_OK;
}

}  // extern "C"
