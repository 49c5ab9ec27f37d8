// spf_seldelta.hip — the route selections a re-sweep changed, on the device
// (gfx950): the counterpart of DecisionRouteDb::calculateUpdate
// (openr/decision/SpfSolver.cpp:24-59) for ospf_sweep_select's route DB.
//
// An ospf_selstate keeps the selection of one prefix table for every root,
// resident and in each root's own width: per root a block metric[P], count[P],
// nh[P][W_root] (SoA, no padding), indexed by NODE ID (a sweep's row order
// changes between plans), in two buffers. seldelta_kernel computes the sweep's
// selection exactly as select_kernel does (the per-prefix device functions of
// spf_select_dev.h), stores it into the shadow buffer, loads the stored entry
// and appends the entries that differ to a change list; the host commits by
// swapping the buffers.
//
// Shape: select_kernel's -- a workgroup per root (grid-stride), its waves
// striding over the table in chunks of 64 prefixes. Per chunk
//   * W <= kSelLaneW: a prefix's result sits in its own lane; metric / count
//     are one coalesced store each, the words one contiguous [n][W] region
//     written cooperatively; the old entry is loaded and compared in the lane;
//   * W > kSelLaneW: prefix_by_words writes the words (a lane per word); the
//     same lanes then compare them with the old words, a ballot makes the
//     verdict wave-uniform and parks it in the prefix's lane;
//   * the chunk's changed entries take their list positions from ONE
//     atomicAdd of the wave (ballot + popcount prefix); the counter always
//     counts, a record is written only below the caller's capacity.
// A root whose distinct-neighbour list differs from the stored one (its bits
// mean other neighbours) is "rebased": reported once, its entries not
// compared, its shadow entries written all the same. Every wave of the block
// compares the whole list itself (the two lists are a few cache lines, read
// once from L2 by the other waves): the verdict is wave-uniform without LDS
// or a barrier, and lane 0 of wave 0 alone appends the root.
// No LDS, no scratch, no inline assembly; plain vector stores and atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "spf_select_dev.h"
#include "spf_selstate.h"
#include "sweep_impl.h"

namespace {

using namespace ospf_sel;

struct SdArgs {
  const ospf_int::SelRow* rows;  // the sweep's rows, owned-roots order
  const uint32_t* roots;         // node id of each row
  uint32_t n_roots, P;
  const uint32_t* off;    // the prefix table (CSR)
  const uint32_t* nodes;
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
  uint4* changes;      // ospf_select_change records
  uint32_t* chg_nh;    // [cap][nh_words] or null
  uint32_t nh_words, cap;
  uint32_t* rebased;
  uint32_t cap_rebased;
};

__global__ __launch_bounds__(256) void seldelta_kernel(const SdArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P;
  const uint32_t* __restrict__ off = a.off;
  const uint32_t* __restrict__ nodes = a.nodes;
  for (uint32_t ri = blockIdx.x; ri < a.n_roots; ri += gridDim.x) {
    const uint32_t* __restrict__ dist = a.rows[ri].dist;
    const uint32_t* __restrict__ nh = a.rows[ri].nh;
    const uint32_t W = a.rows[ri].W;
    const uint32_t r = a.roots[ri];
    uint32_t* n_m = a.n_data + a.n_off[r];
    uint32_t* n_c = n_m + P;
    uint32_t* n_nh = n_c + P;
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
    const uint32_t* o_c = nullptr;
    const uint32_t* o_nh = nullptr;
    if (cmp) {
      o_m = a.o_data + a.o_off[r];
      o_c = o_m + P;
      o_nh = o_c + P;
    }
    for (uint32_t base = wv * 64u; base < P; base += nwv * 64u) {
      const uint32_t p = base + lane;
      const bool in = p < P;
      const uint32_t n = min(64u, P - base);  // prefixes of this chunk
      uint32_t lo = 0, hi = 0;
      if (in) {
        lo = off[p];
        hi = off[p + 1];
      }
      uint32_t m = kInf, cnt = 0;
      uint32_t acc[kSelLaneW];
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
      bool ch = false;  // this lane's prefix differs from the stored entry
      if (W <= kSelLaneW) {
        const bool mine = in && hi - lo <= kSelShort;
        const unsigned long long wide = __ballot(in && !mine);
        if (mine) prefix_by_lane(dist, nh, W, nodes, lo, hi, m, cnt, acc);
        // the chunk's long prefixes, one at a time by the wave; the result
        // parked in the prefix's own lane
        for (unsigned long long t = wide; t; t &= t - 1ull) {
          const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
          uint32_t wm, wc, wa[kSelLaneW];
          prefix_by_lanes(dist, nh, W, nodes, lane_get(lo, j), lane_get(hi, j), lane, true, wm,
                          wc, wa);
          if (lane == j) {
            m = wm;
            cnt = wc;
#pragma unroll
            for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = wa[w];
          }
        }
        // [n][W] words of the chunk, contiguous: word i of the region is word
        // i % W of prefix i / W
        uint32_t* dst = n_nh + (size_t)base * W;
        if (W == 1u) {
          if (in) dst[lane] = acc[0];
        } else {
          const uint32_t total = n * W;
          for (uint32_t i0 = 0; i0 < total; i0 += 64) {  // wave-uniform trips (shuffles)
            const uint32_t i = i0 + lane;
            const bool ok = i < total;
            const uint32_t pl = ok ? i / W : 0u;
            const uint32_t w = i - pl * W;
            uint32_t v = 0;
#pragma unroll
            for (uint32_t k = 0; k < kSelLaneW; ++k)
              if (k < W) {
                const uint32_t t = lane_get(acc[k], pl);
                if (w == k) v = t;
              }
            if (ok) dst[i] = v;
          }
        }
        if (cmp && in) {
          const uint32_t* ow = o_nh + (size_t)p * W;
#pragma unroll
          for (uint32_t w = 0; w < kSelLaneW; ++w)
            if (w < W) ch |= ow[w] != acc[w];
        }
      } else {
        for (uint32_t j = 0; j < n; ++j) {
          uint32_t wm, wc;
          uint32_t* mine = n_nh + (size_t)(base + j) * W;
          prefix_by_words(dist, nh, W, nodes, lane_get(lo, j), lane_get(hi, j), lane, W, mine, wm,
                          wc);
          bool diff = false;
          if (cmp) {  // each lane the words it has just written
            const uint32_t* ow = o_nh + (size_t)(base + j) * W;
            for (uint32_t w = lane; w < W; w += 64) diff |= mine[w] != ow[w];
          }
          const bool any = __ballot(diff) != 0ull;
          if (lane == j) {
            m = wm;
            cnt = wc;
            ch = any;
          }
        }
      }
      if (in) {
        n_m[p] = m;
        n_c[p] = cnt;
        if (cmp) ch |= o_m[p] != m || o_c[p] != cnt;
      }
      // append the chunk's changed entries: one atomicAdd of the wave
      const unsigned long long mask = __ballot(ch);
      if (mask) {
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t b0 = 0;
        if (lane == leader) b0 = atomicAdd(&a.counters[0], (uint32_t)__popcll(mask));
        b0 = lane_get(b0, leader);
        const uint32_t idx = b0 + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const bool put = ch && idx < a.cap;
        if (put) a.changes[idx] = make_uint4(r, p, m, cnt);
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
              if (ij >= a.cap) continue;
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

}  // namespace

namespace {

using namespace ospf_int;
using namespace ospf_int::sweep;
using namespace ospf_int::selst;

void release(ospf_selstate* st) {
  if (!st->c) return;
  (void)hipSetDevice(st->c->device);
  (void)hipDeviceSynchronize();
  if (st->release_ucmp) st->release_ucmp(st);
  for (auto& b : st->b) {
    (void)hipFree(b.data);
    (void)hipFree(b.off);
    (void)hipFree(b.w);
    (void)hipFree(b.dn_off);
    (void)hipFree(b.dn);
    b = ospf_selstate::Buf{};
  }
  (void)hipFree(st->d_tab);
  (void)hipFree(st->d_pol);
  (void)hipFree(st->d_roots);
  (void)hipFree(st->d_cnt);
  (void)hipFree(st->d_chg);
  (void)hipFree(st->d_chg_nh);
  (void)hipFree(st->d_reb);
  st->d_tab = st->d_pol = st->d_roots = st->d_cnt = st->d_chg_nh = st->d_reb = nullptr;
  st->d_chg = nullptr;
  st->chg_cap = st->chg_nh_words = st->reb_cap = 0;
  st->device_bytes = 0;
  st->primed = false;
}

}  // namespace

int ospf_int::selst::write_shadow(ospf_selstate* st, ospf_sweep* sw, bool compare,
                                  uint32_t nh_words, bool want_nh, uint32_t cap, uint32_t cap_reb,
                                  uint32_t counts[2]) {
  ospf_ctx* c = st->c;
  const uint32_t V = st->V, P = st->P;
  ospf_selstate::Buf& nb = st->b[st->cur ^ 1];
  const ospf_selstate::Buf& ob = st->b[st->cur];
  counts[0] = counts[1] = 0;
  STCHK(st, hipSetDevice(c->device));
  STCHK(st, hipDeviceSynchronize());  // the rows, whichever streams ran the sweep
  if (const int rc = select_rows(sw)) return stfail(st, rc, "selstate: " + sw->err);
  // block offsets by node id, in this sweep's widths
  nb.h_off.resize(V);
  nb.h_w.resize(V);
  uint64_t words = 0;
  for (uint32_t r = 0; r < V; ++r) {
    nb.h_off[r] = words;
    nb.h_w[r] = sw->row_w[r];
    words += (uint64_t)P * (st->hdr + sw->row_w[r]);
  }
  int rc;
  if ((rc = grow(st, &nb.data, &nb.data_words, words))) return rc;
  size_t dn_have = nb.dn_words;
  if ((rc = grow(st, &nb.dn, &dn_have, c->h_dn.size()))) return rc;
  nb.dn_words = dn_have;
  STCHK(st, hipMemcpy(nb.off, nb.h_off.data(), (size_t)V * 8, hipMemcpyHostToDevice));
  STCHK(st, hipMemcpy(nb.w, nb.h_w.data(), (size_t)V * 4, hipMemcpyHostToDevice));
  STCHK(st, hipMemcpy(nb.dn_off, c->h_dn_off.data(), ((size_t)V + 1) * 4, hipMemcpyHostToDevice));
  if (!c->h_dn.empty())
    STCHK(st, hipMemcpy(nb.dn, c->h_dn.data(), c->h_dn.size() * 4, hipMemcpyHostToDevice));
  STCHK(st, hipMemcpy(st->d_roots, sw->roots.data(), (size_t)V * 4, hipMemcpyHostToDevice));
  if (compare) {
    // a policy record is two uint4
    if ((rc = grow(st, &st->d_chg, &st->chg_cap, (size_t)cap * (st->policy ? 2u : 1u)))) return rc;
    if (want_nh && (rc = grow(st, &st->d_chg_nh, &st->chg_nh_words, (size_t)cap * nh_words))) return rc;
    if ((rc = grow(st, &st->d_reb, &st->reb_cap, cap_reb))) return rc;
  }
  const uint32_t zero[2] = {0, 0};
  STCHK(st, hipMemcpy(st->d_cnt, zero, sizeof(zero), hipMemcpyHostToDevice));
  if (!V || !P) return OSPF_OK;  // no entry: nothing to store or compare
  if (st->policy) {
    if ((rc = policy_delta_launch(st, sw, compare, nh_words, want_nh, cap, cap_reb))) return rc;
    STCHK(st, hipDeviceSynchronize());
    STCHK(st, hipMemcpy(counts, st->d_cnt, 8, hipMemcpyDeviceToHost));
    return OSPF_OK;
  }
  SdArgs a{};
  a.rows = sw->d_sel_rows;
  a.roots = st->d_roots;
  a.n_roots = V;
  a.P = P;
  a.off = st->d_tab;
  a.nodes = st->d_tab + P + 1;
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
    a.cap = cap;
    a.rebased = st->d_reb;
    a.cap_rebased = cap_reb;
  }
  a.counters = st->d_cnt;
  // a wave per 64 prefixes of the root, at most 4; roots beyond the grid by stride
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  hipLaunchKernelGGL(seldelta_kernel, dim3(std::min(V, 1u << 20)), dim3(64u * waves), 0, nullptr, a);
  STCHK(st, hipGetLastError());
  STCHK(st, hipDeviceSynchronize());
  STCHK(st, hipMemcpy(counts, st->d_cnt, 8, hipMemcpyDeviceToHost));
  return OSPF_OK;
}

const char* ospf_int::selst::sweep_error(const ospf_selstate* st, const ospf_sweep* sw) {
  if (sw->c != st->c) return "selstate: the sweep belongs to another context";
  if (!sw->ran) return "selstate: the sweep has not run";
  if (sw->V != st->V) return "selstate: the sweep's graph has another node count";
  if (sw->roots.size() != sw->V)
    return "selstate: the sweep owns a part of the roots (several parts are not supported)";
  if (sw->gen != st->c->graph_gen || st->c->mask.on)
    return "selstate: the graph changed since the sweep was created";
  return nullptr;
}

void ospf_int::selst::committed(ospf_selstate* st, const ospf_sweep* sw) {
  st->gen = sw->gen;
  st->hop = (sw->opts.flags & OSPF_HOP_COUNT) != 0;
  ++st->serial;
}

uint32_t ospf_int::selst::max_words(const ospf_sweep* sw) {
  uint32_t mw = 0;
  for (uint32_t r : sw->roots) mw = std::max(mw, sw->row_w[r]);
  return mw;
}

int ospf_int::selst::create(ospf_ctx* c, const ospf_select_table* t, const ospf_select_ptable* pol,
                            ospf_selstate** out) {
  const uint32_t V = c->info.n_nodes;
  ospf_selstate* st = new (std::nothrow) ospf_selstate();
  if (!st) return OSPF_E_NOMEM;
  st->c = c;
  st->V = V;
  st->P = t->n_prefixes;
  const uint32_t P = st->P;
  if (P) {
    st->t_off.assign(t->offsets, t->offsets + P + 1);
    st->t_nodes.assign(t->nodes, t->nodes + t->offsets[P]);
  } else {
    st->t_off.assign(1, 0u);
  }
  if (pol) {
    st->policy = true;
    st->hdr = 5;
    const size_t A = st->t_nodes.size();
    if (A) st->t_pref.assign(pol->pref, pol->pref + A);
    if (A && pol->min_nexthop) st->t_mnh.assign(pol->min_nexthop, pol->min_nexthop + A);
  }
  auto setup = [&]() -> int {
    STCHK(st, hipSetDevice(c->device));
    size_t have = 0;
    int rc;
    if ((rc = grow(st, &st->d_tab, &have, st->t_off.size() + st->t_nodes.size()))) return rc;
    STCHK(st, hipMemcpy(st->d_tab, st->t_off.data(), st->t_off.size() * 4, hipMemcpyHostToDevice));
    if (!st->t_nodes.empty())
      STCHK(st, hipMemcpy(st->d_tab + P + 1, st->t_nodes.data(), st->t_nodes.size() * 4,
                          hipMemcpyHostToDevice));
    if (st->policy) {
      const size_t A = st->t_nodes.size();
      if ((rc = grow(st, &st->d_pol, &(have = 0), 2 * A))) return rc;
      if (A) STCHK(st, hipMemcpy(st->d_pol, st->t_pref.data(), A * 4, hipMemcpyHostToDevice));
      if (!st->t_mnh.empty())
        STCHK(st, hipMemcpy(st->d_pol + A, st->t_mnh.data(), A * 4, hipMemcpyHostToDevice));
    }
    if ((rc = grow(st, &st->d_roots, &(have = 0), V))) return rc;
    if ((rc = grow(st, &st->d_cnt, &(have = 0), 2))) return rc;
    for (auto& b : st->b) {
      if ((rc = grow(st, &b.off, &(have = 0), V))) return rc;
      if ((rc = grow(st, &b.w, &(have = 0), V))) return rc;
      if ((rc = grow(st, &b.dn_off, &(have = 0), (size_t)V + 1))) return rc;
    }
    return OSPF_OK;
  };
  if (const int rc = setup()) {
    release(st);
    delete st;
    return rc;
  }
  c->live_selstates.push_back(st);
  c->release_selstate = [](ospf_selstate* x) {  // ospf_close: release now, detach
    release(x);
    x->c = nullptr;
  };
  *out = st;
  return OSPF_OK;
}

extern "C" {

int ospf_selstate_create(ospf_ctx* c, const ospf_select_table* t, ospf_selstate** out) {
  if (!c || !out) return OSPF_E_INVAL;
  *out = nullptr;
  if (!c->loaded) return fail(c, OSPF_E_NOGRAPH, "no graph loaded");
  if (const char* bad = select_table_check(t, c->info.n_nodes)) return fail(c, OSPF_E_INVAL, bad);
  return create(c, t, nullptr, out);
}

int ospf_selstate_destroy(ospf_selstate* st) {
  if (!st) return OSPF_E_INVAL;
  if (st->c) {
    auto& l = st->c->live_selstates;
    l.erase(std::remove(l.begin(), l.end(), st), l.end());
    release(st);
  }
  delete st;
  return OSPF_OK;
}

const char* ospf_selstate_last_error(const ospf_selstate* st) {
  return st ? st->err.c_str() : "null select state";
}

uint64_t ospf_selstate_device_bytes(const ospf_selstate* st) { return st ? st->device_bytes : 0; }

int ospf_selstate_prime(ospf_selstate* st, ospf_sweep* sw) {
  if (!st || !sw || !st->c) return OSPF_E_INVAL;
  if (injected(st->c)) return stfail(st, OSPF_E_DEVICE, st->c->err);
  if (const char* bad = sweep_error(st, sw)) return stfail(st, OSPF_E_INVAL, bad);
  uint32_t counts[2];
  const int rc = write_shadow(st, sw, false, 0, false, 0, 0, counts);
  if (rc) return rc;
  st->cur ^= 1;
  st->primed = true;
  committed(st, sw);
  return OSPF_OK;
}

int ospf_selstate_update(ospf_selstate* st, ospf_sweep* sw, uint32_t nh_words,
                         ospf_select_change* changes, uint32_t* nh, uint32_t cap,
                         uint32_t* n_changes, uint32_t* rebased_roots, uint32_t cap_rebased,
                         uint32_t* n_rebased) {
  if (!st || !sw || !st->c || !n_changes || !n_rebased || (cap && !changes) ||
      (cap_rebased && !rebased_roots))
    return OSPF_E_INVAL;
  *n_changes = *n_rebased = 0;
  if (injected(st->c)) return stfail(st, OSPF_E_DEVICE, st->c->err);
  if (st->policy)
    return stfail(st, OSPF_E_INVAL, "selstate: a policy state is updated by ospf_selstate_update_policy");
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
  static_assert(sizeof(ospf_select_change) == sizeof(uint4), "change records are stored as uint4");
  if (counts[0]) {
    STCHK(st, hipMemcpy(changes, st->d_chg, (size_t)counts[0] * sizeof(uint4), hipMemcpyDeviceToHost));
    if (want_nh)
      STCHK(st, hipMemcpy(nh, st->d_chg_nh, (size_t)counts[0] * nh_words * 4, hipMemcpyDeviceToHost));
  }
  if (counts[1])
    STCHK(st, hipMemcpy(rebased_roots, st->d_reb, (size_t)counts[1] * 4, hipMemcpyDeviceToHost));
  st->cur ^= 1;  // commit
  committed(st, sw);
  return OSPF_OK;
}

int ospf_selstate_copy(ospf_selstate* st, const uint32_t* roots, uint32_t n, uint32_t nh_words,
                       uint32_t* metric, uint32_t* count, uint32_t* nh) {
  if (!st || !st->c || (n && !roots)) return OSPF_E_INVAL;
  if (injected(st->c)) return stfail(st, OSPF_E_DEVICE, st->c->err);
  if (!st->primed) return stfail(st, OSPF_E_INVAL, "selstate: copy before prime");
  const ospf_selstate::Buf& b = st->b[st->cur];
  const size_t P = st->P;
  for (uint32_t i = 0; i < n; ++i) {
    if (roots[i] >= st->V) return stfail(st, OSPF_E_INVAL, "selstate: root id outside the graph");
    if (nh && b.h_w[roots[i]] > nh_words)
      return stfail(st, OSPF_E_INVAL, "selstate: nh_words below a root's next-hop words");
  }
  if (!n || !P || (!metric && !count && !nh)) return OSPF_OK;
  STCHK(st, hipSetDevice(st->c->device));
  std::vector<uint32_t> blk;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i], W = b.h_w[r];
    blk.resize(P * (st->hdr + W));
    STCHK(st, hipMemcpy(blk.data(), b.data + b.h_off[r], blk.size() * 4, hipMemcpyDeviceToHost));
    if (metric) std::memcpy(metric + i * P, blk.data(), P * 4);
    if (count) std::memcpy(count + i * P, blk.data() + P, P * 4);
    if (nh) {
      uint32_t* dst = nh + i * P * nh_words;
      std::memset(dst, 0, P * nh_words * 4);
      for (size_t p = 0; p < P; ++p)
        std::memcpy(dst + p * nh_words, blk.data() + st->hdr * P + p * W, (size_t)W * 4);
    }
  }
  return OSPF_OK;
}

}  // extern "C"
