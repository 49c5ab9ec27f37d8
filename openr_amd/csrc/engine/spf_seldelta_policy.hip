// spf_seldelta_policy.hip — the route selections a re-sweep (or a change of
// the prefix attributes) changed under the reference's best-route policy, on
// the device (gfx950): DecisionRouteDb::calculateUpdate
// (openr/decision/SpfSolver.cpp:24-59) over the routes createRouteForPrefix
// (:197-458) produces, i.e. ospf_sweep_select_policy's route DB kept resident.
//
// A policy ospf_selstate (spf_selstate.h, hdr = 5) keeps per root and by node
// id a block metric[P], count[P], links[P], need[P], best[P], nh[P][W_root]
// (SoA, no padding) in two buffers; the rule and its 64-bit key are in
// spf_selpolicy_dev.h. seldelta_policy_kernel computes the sweep's selection
// with policy_kernel's per-prefix device functions, stores it into the shadow
// buffer, compares it with the committed entry and appends what differs to a
// change list; the host (spf_seldelta.hip: write_shadow) commits by swapping.
//
// Shape: seldelta_kernel's -- a workgroup per root (grid-stride), its waves
// striding over the table in chunks of 64 prefixes; the rebase test per wave
// (every wave compares the root's whole distinct-neighbour list, so the
// verdict is wave-uniform without LDS traffic); a chunk's changed entries take
// their list positions from ONE atomicAdd of the wave; the counters always
// count, a record is written only below the caller's capacity. Beside it, as
// in policy_kernel, the block builds the root's per-slot link counts once in
// LDS (build_links: 8 bytes per slot of the widest root while building, u16
// per slot after) -- an entry's `links` is their sum over its next-hop bits.
//   * W <= kSelLaneW: a prefix's entry and words sit in its own lane; the five
//     header columns are one coalesced store each, the words one contiguous
//     [n][W] region written cooperatively; the old entry is compared in the lane;
//   * W > kSelLaneW: policy_by_words writes the words (a lane per word); the
//     same lanes compare them with the old words, a ballot makes the verdict
//     the wave's and parks it in the prefix's lane.
// A record is two 16-B stores: {root, prefix, metric, count}, {links, need,
// best, installed}. Every word of the shadow entry is written once by plain
// vector stores; no memset, no scratch, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "spf_selpolicy_dev.h"
#include "spf_selstate.h"
#include "sweep_impl.h"

namespace {

using namespace ospf_sel;
using namespace ospf_selpol;

struct PdArgs {
  const ospf_int::SelRow* rows;  // the sweep's rows, owned-roots order
  const uint32_t* roots;         // node id of each row
  uint32_t n_roots, P, hop;
  uint32_t cap;  // LDS slots (>= every root's distinct neighbours)
  Table t;
  // the loaded graph: the root's CSR row
  const uint32_t* row_ptr;
  const uint32_t* colx;
  const uint32_t* w;
  const uint16_t* didx;
  // the shadow buffer (written): root blocks at n_off[node] words, the graph's
  // distinct-neighbour lists
  uint32_t* n_data;
  const uint64_t* n_off;
  const uint32_t* n_dn_off;
  const uint32_t* n_dn;
  // the stored selection (o_data null: prime, nothing compared)
  const uint32_t* o_data;
  const uint64_t* o_off;
  const uint32_t* o_w;
  const uint32_t* o_dn_off;
  const uint32_t* o_dn;
  uint32_t* counters;  // [0] changed entries, [1] rebased roots
  uint4* changes;      // ospf_select_pchange records, two uint4 each
  uint32_t* chg_nh;    // [chg_cap][nh_words] or null
  uint32_t nh_words, chg_cap;
  uint32_t* rebased;
  uint32_t cap_rebased;
};

__global__ __launch_bounds__(256) void seldelta_policy_kernel(const PdArgs a) {
  extern __shared__ uint32_t lds[];
  const uint16_t* cslot = reinterpret_cast<const uint16_t*>(lds);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P;
  for (uint32_t ri = blockIdx.x; ri < a.n_roots; ri += gridDim.x) {
    const uint32_t* __restrict__ dist = a.rows[ri].dist;
    const uint32_t* __restrict__ nh = a.rows[ri].nh;
    const uint32_t W = a.rows[ri].W;
    const uint32_t r = a.roots[ri];
    const uint32_t ns = min(a.n_dn_off[r + 1] - a.n_dn_off[r], a.cap);
    build_links(a, r, ns, lds);  // block-uniform
    uint32_t* n_m = a.n_data + a.n_off[r];
    uint32_t* n_c = n_m + P;
    uint32_t* n_l = n_c + P;
    uint32_t* n_n = n_l + P;
    uint32_t* n_b = n_n + P;
    uint32_t* n_nh = n_b + P;
    const bool aligned16 = !((uintptr_t)n_nh & 15u);
    bool cmp = a.o_data != nullptr;
    if (cmp) {
      // the root's distinct neighbours then and now (each wave the whole list)
      const uint32_t olo = a.o_dn_off[r], ocnt = a.o_dn_off[r + 1] - olo;
      const uint32_t nlo = a.n_dn_off[r], ncnt = a.n_dn_off[r + 1] - nlo;
      bool diff = ocnt != ncnt || a.o_w[r] != W;
      if (!diff)
        for (uint32_t k = lane; k < ncnt; k += 64) diff |= a.o_dn[olo + k] != a.n_dn[nlo + k];
      if (__ballot(diff)) {  // rebased: listed once, nothing compared
        cmp = false;
        if (threadIdx.x == 0) {
          const uint32_t i = atomicAdd(&a.counters[1], 1u);
          if (i < a.cap_rebased) a.rebased[i] = r;
        }
      }
    }
    const uint32_t* o_m = nullptr;
    const uint32_t* o_nh = nullptr;
    if (cmp) {
      o_m = a.o_data + a.o_off[r];  // its columns P words apart, as the new ones
      o_nh = o_m + 5 * (size_t)P;
    }
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
      uint32_t acc[kSelLaneW];
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
      bool ch = false;  // this lane's prefix differs from the stored entry
      if (W <= kSelLaneW) {
        const bool mine = in && hi - lo <= kSelShort;
        const unsigned long long wide = __ballot(in && !mine);
        if (mine) policy_by_lane(a.t, dist, nh, W, r, lo, hi, true, e, acc);
        // the chunk's long prefixes, one at a time by the wave; the result
        // parked in the prefix's own lane
        for (unsigned long long t = wide; t; t &= t - 1ull) {
          const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
          Entry we;
          uint32_t wa[kSelLaneW];
          policy_by_lanes(a.t, dist, nh, W, r, lane_get(lo, j), lane_get(hi, j), lane, true, we,
                          wa);
          if (lane == j) {
            e = we;
#pragma unroll
            for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = wa[w];
          }
        }
        links = links_of(acc, W, cslot, ns);
        store_chunk_words(n_nh + (size_t)base * W, aligned16, acc, W, W, n, lane, in);
        if (cmp && in) {
          const uint32_t* ow = o_nh + (size_t)p * W;
#pragma unroll
          for (uint32_t w = 0; w < kSelLaneW; ++w)
            if (w < W) ch |= ow[w] != acc[w];
        }
      } else {
        for (uint32_t j = 0; j < n; ++j) {
          Entry we;
          uint32_t* mine = n_nh + (size_t)(base + j) * W;
          const uint32_t wl = policy_by_words(a.t, dist, nh, W, r, lane_get(lo, j),
                                              lane_get(hi, j), lane, W, mine, cslot, ns, true, we);
          bool diff = false;
          if (cmp) {  // each lane the words it has just written
            const uint32_t* ow = o_nh + (size_t)(base + j) * W;
            for (uint32_t w = lane; w < W; w += 64) diff |= mine[w] != ow[w];
          }
          const bool any = __ballot(diff) != 0ull;
          if (lane == j) {
            e = we;
            links = wl;
            ch = any;
          }
        }
      }
      if (in) {
        n_m[p] = e.m;
        n_c[p] = e.cnt;
        n_l[p] = links;
        n_n[p] = e.need;
        n_b[p] = e.best;
        if (cmp)
          ch |= o_m[p] != e.m || o_m[P + p] != e.cnt || o_m[2 * (size_t)P + p] != links ||
                o_m[3 * (size_t)P + p] != e.need || o_m[4 * (size_t)P + p] != e.best;
      }
      // append the chunk's changed entries: one atomicAdd of the wave
      const unsigned long long mask = __ballot(ch);
      if (mask) {
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t b0 = 0;
        if (lane == leader) b0 = atomicAdd(&a.counters[0], (uint32_t)__popcll(mask));
        b0 = lane_get(b0, leader);
        const uint32_t idx = b0 + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const bool put = ch && idx < a.chg_cap;
        if (put) {
          const uint32_t installed = links > 0u && e.need <= links ? 1u : 0u;
          a.changes[2 * (size_t)idx] = make_uint4(r, p, e.m, e.cnt);
          a.changes[2 * (size_t)idx + 1] = make_uint4(links, e.need, e.best, installed);
        }
        if (a.chg_nh) {
          if (W <= kSelLaneW) {
            if (put) {
              uint32_t* o = a.chg_nh + (size_t)idx * a.nh_words;
              for (uint32_t w = 0; w < a.nh_words; ++w) {
                uint32_t v = 0;
#pragma unroll
                for (uint32_t k = 0; k < kSelLaneW; ++k)
                  if (w == k) v = acc[k];
                o[w] = v;
              }
            }
          } else {
            for (unsigned long long t = mask; t; t &= t - 1ull) {  // a record by the wave
              const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
              const uint32_t ij = lane_get(idx, j);
              if (ij >= a.chg_cap) continue;
              const uint32_t* src = n_nh + (size_t)(base + j) * W;
              uint32_t* o = a.chg_nh + (size_t)ij * a.nh_words;
              for (uint32_t w = lane; w < a.nh_words; w += 64) o[w] = w < W ? src[w] : 0u;
            }
          }
        }
      }
    }
  }
}

using namespace ospf_int;
using namespace ospf_int::sweep;
using namespace ospf_int::selst;

// the policy columns' contract for a table of A announcer entries
const char* columns_error(size_t A, const uint32_t* pref) {
  if (A && !pref) return "select policy: null pref";
  for (size_t k = 0; k < A; ++k)
    if (pref[k] >= 0x80000000u) return "select policy: a pref >= 2^31";
  return nullptr;
}

}  // namespace

int ospf_int::selst::policy_delta_launch(ospf_selstate* st, ospf_sweep* sw, bool compare,
                                         uint32_t nh_words, bool want_nh, uint32_t cap,
                                         uint32_t cap_reb) {
  ospf_ctx* c = st->c;
  const uint32_t V = st->V, P = st->P;
  const ospf_selstate::Buf& nb = st->b[st->cur ^ 1];
  const ospf_selstate::Buf& ob = st->b[st->cur];
  const size_t A = st->t_nodes.size();
  PdArgs a{};
  a.rows = sw->d_sel_rows;
  a.roots = st->d_roots;
  a.n_roots = V;
  a.P = P;
  a.hop = (sw->opts.flags & OSPF_HOP_COUNT) ? 1u : 0u;
  a.cap = std::max(1u, c->max_dn);
  a.t = Table{st->d_tab, st->d_tab + P + 1, st->d_pol, st->t_mnh.empty() ? nullptr : st->d_pol + A,
              c->g.nt_bits};
  a.row_ptr = c->g.row_ptr;
  a.colx = c->g.colx;
  a.w = c->g.w;
  a.didx = c->g.didx;
  a.n_data = nb.data;
  a.n_off = nb.off;
  a.n_dn_off = nb.dn_off;
  a.n_dn = nb.dn;
  if (compare) {
    a.o_data = ob.data;
    a.o_off = ob.off;
    a.o_w = ob.w;
    a.o_dn_off = ob.dn_off;
    a.o_dn = ob.dn;
    a.changes = st->d_chg;
    a.chg_nh = want_nh ? st->d_chg_nh : nullptr;
    a.nh_words = nh_words;
    a.chg_cap = cap;
    a.rebased = st->d_reb;
    a.cap_rebased = cap_reb;
  }
  a.counters = st->d_cnt;
  // a wave per 64 prefixes of the root, at most 4; roots beyond the grid by
  // stride; LDS: two words per slot while a root's links are built
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  const size_t lds = (size_t)a.cap * 8;
  if (lds > c->lds_limit)
    return stfail(st, OSPF_E_RANGE, "selstate: the widest root's link counts do not fit the LDS");
  hipLaunchKernelGGL(seldelta_policy_kernel, dim3(std::min(V, 1u << 20)), dim3(64u * waves), lds,
                     nullptr, a);
  STCHK(st, hipGetLastError());
  return OSPF_OK;
}

extern "C" {

int ospf_selstate_create_policy(ospf_ctx* c, const ospf_select_ptable* t, ospf_selstate** out) {
  if (!c || !out) return OSPF_E_INVAL;
  *out = nullptr;
  if (!c->loaded) return fail(c, OSPF_E_NOGRAPH, "no graph loaded");
  if (const char* bad = select_ptable_check(t, c->info.n_nodes)) return fail(c, OSPF_E_INVAL, bad);
  const ospf_select_table plain{t->n_prefixes, t->offsets, t->nodes};
  return create(c, &plain, t, out);
}

int ospf_selstate_update_policy(ospf_selstate* st, ospf_sweep* sw, uint32_t nh_words,
                                ospf_select_pchange* changes, uint32_t* nh, uint32_t cap,
                                uint32_t* n_changes, uint32_t* rebased_roots, uint32_t cap_rebased,
                                uint32_t* n_rebased) {
  if (!st || !sw || !st->c || !n_changes || !n_rebased || (cap && !changes) ||
      (cap_rebased && !rebased_roots))
    return OSPF_E_INVAL;
  *n_changes = *n_rebased = 0;
  if (injected(st->c)) return stfail(st, OSPF_E_DEVICE, st->c->err);
  if (!st->policy)
    return stfail(st, OSPF_E_INVAL, "selstate: update_policy on a state without a policy table");
  if (!st->primed) return stfail(st, OSPF_E_INVAL, "selstate: update before prime");
  if (const char* bad = sweep_error(st, sw)) return stfail(st, OSPF_E_INVAL, bad);
  if (nh_words < max_words(sw))
    return stfail(st, OSPF_E_INVAL, "selstate: nh_words below a root's next-hop words");
  uint32_t counts[2];
  const bool want_nh = nh != nullptr && cap != 0;
  const int rc = write_shadow(st, sw, true, nh_words, want_nh, cap, cap_rebased, counts);
  if (rc) return rc;
  *n_changes = counts[0];
  *n_rebased = counts[1];
  if (counts[0] > cap || counts[1] > cap_rebased)
    return stfail(st, OSPF_E_RANGE, "selstate: " + std::to_string(counts[0]) + " changes, " +
                                        std::to_string(counts[1]) +
                                        " rebased roots: above the caller's capacity");
  static_assert(sizeof(ospf_select_pchange) == 2 * sizeof(uint4), "policy records are two uint4");
  if (counts[0]) {
    STCHK(st, hipMemcpy(changes, st->d_chg, (size_t)counts[0] * sizeof(ospf_select_pchange),
                        hipMemcpyDeviceToHost));
    if (want_nh)
      STCHK(st, hipMemcpy(nh, st->d_chg_nh, (size_t)counts[0] * nh_words * 4, hipMemcpyDeviceToHost));
  }
  if (counts[1])
    STCHK(st, hipMemcpy(rebased_roots, st->d_reb, (size_t)counts[1] * 4, hipMemcpyDeviceToHost));
  st->cur ^= 1;  // commit
  committed(st, sw);
  return OSPF_OK;
}

int ospf_selstate_copy_policy(ospf_selstate* st, const uint32_t* roots, uint32_t n,
                              uint32_t nh_words, const ospf_select_pout* out) {
  if (!st || !st->c || (n && !roots) || !out) return OSPF_E_INVAL;
  if (injected(st->c)) return stfail(st, OSPF_E_DEVICE, st->c->err);
  if (!st->policy)
    return stfail(st, OSPF_E_INVAL, "selstate: copy_policy on a state without a policy table");
  if (!st->primed) return stfail(st, OSPF_E_INVAL, "selstate: copy before prime");
  const ospf_selstate::Buf& b = st->b[st->cur];
  const size_t P = st->P;
  for (uint32_t i = 0; i < n; ++i) {
    if (roots[i] >= st->V) return stfail(st, OSPF_E_INVAL, "selstate: root id outside the graph");
    if (out->nh && b.h_w[roots[i]] > nh_words)
      return stfail(st, OSPF_E_INVAL, "selstate: nh_words below a root's next-hop words");
  }
  uint32_t* const col[5] = {out->metric, out->count, out->links, out->need, out->best};
  if (!n || !P || (!out->nh && !col[0] && !col[1] && !col[2] && !col[3] && !col[4])) return OSPF_OK;
  STCHK(st, hipSetDevice(st->c->device));
  // every block off the device first: a failed copy leaves the caller's buffers as they were
  std::vector<std::vector<uint32_t>> blk(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i];
    blk[i].resize(P * (5u + b.h_w[r]));
    STCHK(st, hipMemcpy(blk[i].data(), b.data + b.h_off[r], blk[i].size() * 4, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t W = b.h_w[roots[i]];
    for (int k = 0; k < 5; ++k)
      if (col[k]) std::memcpy(col[k] + i * P, blk[i].data() + k * P, P * 4);
    if (out->nh) {
      uint32_t* dst = out->nh + i * P * nh_words;
      std::memset(dst, 0, P * nh_words * 4);
      for (size_t p = 0; p < P; ++p)
        std::memcpy(dst + p * nh_words, blk[i].data() + 5 * P + p * W, (size_t)W * 4);
    }
  }
  return OSPF_OK;
}

int ospf_selstate_set_policy(ospf_selstate* st, const uint32_t* pref, const uint32_t* min_nexthop) {
  if (!st || !st->c) return OSPF_E_INVAL;
  if (injected(st->c)) return stfail(st, OSPF_E_DEVICE, st->c->err);
  if (!st->policy)
    return stfail(st, OSPF_E_INVAL, "selstate: set_policy on a state without a policy table");
  const size_t A = st->t_nodes.size();
  if (const char* bad = columns_error(A, pref)) return stfail(st, OSPF_E_INVAL, bad);
  if (A) {
    // both columns in one copy: it either replaces them or leaves them
    std::vector<uint32_t> both(2 * A, 0u);
    std::copy(pref, pref + A, both.begin());
    if (min_nexthop) std::copy(min_nexthop, min_nexthop + A, both.begin() + A);
    STCHK(st, hipSetDevice(st->c->device));
    STCHK(st, hipDeviceSynchronize());
    STCHK(st, hipMemcpy(st->d_pol, both.data(), both.size() * 4, hipMemcpyHostToDevice));
    st->t_pref.assign(pref, pref + A);
    if (min_nexthop) st->t_mnh.assign(min_nexthop, min_nexthop + A);
    else st->t_mnh.clear();
  }
  ++st->serial;  // a resolved UCMP result is stale, as after an update
  return OSPF_OK;
}

}  // extern "C"
