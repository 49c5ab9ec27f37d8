// spf_selpolicy_dev.h — the per-prefix device functions of route selection
// under the reference's best-route policy (spf_selpolicy.hip: policy_kernel,
// the one-shot selection; spf_seldelta_policy.hip: seldelta_policy_kernel,
// the resident selection and its delta; spf_selsrmpls.hip: srmpls_kernel, the
// same selection with per-destination next hops). Per (root r, prefix p) createRouteForPrefix
// (openr/decision/SpfSolver.cpp:197-458) before it takes the minimum
//   R  = the announcers r reaches                                  (:229-244)
//   S  = those of R in the best (path pref, source pref, distance) class
//        (selectBestRoutes -> selectRoutes(SHORTEST_DISTANCE), :649-676)
//   S' = the undrained ones of S, or S when all of S are drained
//        (maybeFilterDrainedNodes, :709-731)
//   L  = those of S' at the smallest distance m    (getNextHopsWithMetric)
// is ONE unsigned minimum of a 64-bit key over R,
//   key = pref << 33 | drained << 32 | dist        (pref < 2^31: the class
//         rank, smaller wins; drained: the node's no-transit bit),
// with kmin the smallest key: L = {key == kmin}, S' = {key >> 32 == kmin >>
// 32}, S = {key >> 33 == kmin >> 33}. Beside the metric / count / next-hop
// words of L an entry carries need = max min_nexthop over S' (the maximum
// over allNodeAreas of getMinNextHopThreshold, :693-707) and best = r when
// r is in S, else the smallest id of S (selectBestNodeArea: picked before the
// drain filter, which never moves it, :724-728).
// The same three strategies per prefix as spf_select_dev.h: a short prefix by
// its own lane (one pass), a long one by the wave with a lane per announcer,
// any prefix of a wide root with a lane per next-hop word. A wave's 64-bit
// minimum is two dependent 32-bit unsigned reductions, the high word first.
// Device code only; not a public header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_select_dev.h"

namespace ospf_selpol {

using ospf_sel::kInf;
using ospf_sel::kSelLaneW;
using ospf_sel::lane_get;
using ospf_sel::wave_min;
using ospf_sel::wave_or;

constexpr uint64_t kNoKey = ~0ull;  // above every key (pref < 2^31, dist != kInf)

// the prefix table with its policy columns, and what a root's entry reads of
// the graph
struct Table {
  const uint32_t* off;      // [P + 1]
  const uint32_t* nodes;    // announcer ids, ascending per prefix
  const uint32_t* pref;     // parallel to nodes, < 2^31
  const uint32_t* mnh;      // parallel to nodes (0: unset), or null: all unset
  const uint32_t* nt_bits;  // the loaded graph's no-transit bitmap
};

// what one (root, prefix) entry holds beside its next-hop words
struct Entry {
  uint32_t m = kInf, cnt = 0, need = 0, best = kInf;
};

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}

// unsigned 64-bit wave minimum: the high words first, then the low words of
// the lanes that hold the smallest high word
__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
  const uint32_t hi = wave_min((uint32_t)(v >> 32));
  const uint32_t lo = wave_min((uint32_t)(v >> 32) == hi ? (uint32_t)v : 0xFFFFFFFFu);
  return ((uint64_t)hi << 32) | lo;
}

// key of announcer entry k (node id) at distance d != kInf
__device__ __forceinline__ uint64_t key_of(const Table& t, uint32_t k, uint32_t id, uint32_t d) {
  const uint32_t drained = (t.nt_bits[id >> 5] >> (id & 31u)) & 1u;
  return ((uint64_t)t.pref[k] << 33) | ((uint64_t)drained << 32) | d;
}

// key of entry k as this root sees it (kNoKey: not reached)
__device__ __forceinline__ uint64_t key_at(const Table& t, const uint32_t* __restrict__ dist,
                                           uint32_t k, uint32_t& id) {
  id = t.nodes[k];
  const uint32_t d = dist[id];
  return d == kInf ? kNoKey : key_of(t, k, id, d);
}

// best of a class: the root when it is a member, else the smallest member
__device__ __forceinline__ uint32_t best_of(uint32_t smallest, bool has_root, uint32_t r) {
  return has_root ? r : smallest;
}

// A short prefix by its own lane (W <= kSelLaneW), one pass over its
// announcers: a smaller key restarts what its changed high bits invalidate
// (the class: best; the drained bit: need; the whole key: count and words).
__device__ __forceinline__ void policy_by_lane(const Table& t, const uint32_t* __restrict__ dist,
                                               const uint32_t* __restrict__ nh, uint32_t W,
                                               uint32_t r, uint32_t lo, uint32_t hi, bool want_nh,
                                               Entry& e, uint32_t (&acc)[kSelLaneW]) {
  uint64_t kmin = kNoKey;
  uint32_t smallest = kInf;
  bool has_root = false;
  for (uint32_t k = lo; k < hi; ++k) {
    uint32_t id;
    const uint64_t key = key_at(t, dist, k, id);
    if (key == kNoKey) continue;
    if (key < kmin) {
      if ((key >> 33) != (kmin >> 33)) {
        smallest = kInf;
        has_root = false;
      }
      if ((key >> 32) != (kmin >> 32)) e.need = 0;
      e.cnt = 0;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
      kmin = key;
    }
    if ((key >> 33) == (kmin >> 33)) {
      smallest = min(smallest, id);
      has_root = has_root || id == r;
    }
    if ((key >> 32) == (kmin >> 32) && t.mnh) e.need = max(e.need, t.mnh[k]);
    if (key == kmin) {
      ++e.cnt;
      if (want_nh) {
        const uint32_t* row = nh + (size_t)id * W;
#pragma unroll
        for (uint32_t w = 0; w < kSelLaneW; ++w)
          if (w < W) acc[w] |= row[w];
      }
    }
  }
  if (kmin != kNoKey) {
    e.m = (uint32_t)kmin;
    e.best = best_of(smallest, has_root, r);
  }
}

// pass 1 of a wave's prefix: the smallest key (kNoKey: none reached)
__device__ __forceinline__ uint64_t policy_min(const Table& t, const uint32_t* __restrict__ dist,
                                               uint32_t lo, uint32_t hi, uint32_t lane) {
  uint64_t m = kNoKey;
  for (uint32_t k = lo + lane; k < hi; k += 64) {
    uint32_t id;
    const uint64_t key = key_at(t, dist, k, id);
    m = key < m ? key : m;
  }
  return wave_min64(m);
}

// the lanes' shares of an entry's need / best, reduced over the wave
__device__ __forceinline__ void policy_reduce(uint32_t need, uint32_t smallest, bool has_root,
                                              uint32_t r, uint64_t kmin, Entry& e) {
  e.m = (uint32_t)kmin;
  e.need = wave_max(need);
  e.best = best_of(wave_min(smallest), __ballot(has_root) != 0ull, r);
}

// one reached entry's share of need / best under the smallest key kmin: its
// id into the class's smallest id and root flag when it is of S, its
// threshold into need when it is of S'
__device__ __forceinline__ void class_fold(const Table& t, uint64_t key, uint64_t kmin, uint32_t k,
                                           uint32_t id, uint32_t r, uint32_t& need,
                                           uint32_t& smallest, bool& has_root) {
  if (key != kNoKey && (key >> 33) == (kmin >> 33)) {
    smallest = min(smallest, id);
    has_root = has_root || id == r;
  }
  if (key != kNoKey && (key >> 32) == (kmin >> 32) && t.mnh) need = max(need, t.mnh[k]);
}

// A long prefix by the whole wave, a lane per announcer (W <= kSelLaneW):
// wave-uniform entry and words. Pass 2 re-reads the ids and folds count,
// words, need and best into the one walk.
__device__ __forceinline__ void policy_by_lanes(const Table& t, const uint32_t* __restrict__ dist,
                                                const uint32_t* __restrict__ nh, uint32_t W,
                                                uint32_t r, uint32_t lo, uint32_t hi, uint32_t lane,
                                                bool want_nh, Entry& e,
                                                uint32_t (&acc)[kSelLaneW]) {
  e = Entry{};
#pragma unroll
  for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
  const uint64_t kmin = policy_min(t, dist, lo, hi, lane);
  if (kmin == kNoKey) return;  // wave-uniform
  uint32_t need = 0, smallest = kInf, cnt = 0;
  bool has_root = false;
  for (uint32_t k0 = lo; k0 < hi; k0 += 64) {  // wave-uniform trips (ballot)
    const uint32_t k = k0 + lane;
    uint32_t id = 0;
    uint64_t key = kNoKey;
    if (k < hi) key = key_at(t, dist, k, id);
    const bool tight = key == kmin;
    class_fold(t, key, kmin, k, id, r, need, smallest, has_root);
    cnt += (uint32_t)__popcll(__ballot(tight));
    if (tight && want_nh) {
      const uint32_t* row = nh + (size_t)id * W;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w)
        if (w < W) acc[w] |= row[w];
    }
  }
  e.cnt = cnt;
  policy_reduce(need, smallest, has_root, r, kmin, e);
  if (want_nh) {
#pragma unroll
    for (uint32_t w = 0; w < kSelLaneW; ++w)
      if (w < W) acc[w] = wave_or(acc[w]);
  }
}

// Any prefix by the whole wave, a lane per next-hop word (W > kSelLaneW):
// writes the prefix's Wout words itself (o_nh: this prefix's words, or null)
// and returns, wave-uniform, the sum of cslot[k] over the set bits k < ns of
// the words (the entry's next-hop links; cslot: the root's per-slot link
// counts in LDS), 0 when `want_links` is false.
__device__ __forceinline__ uint32_t policy_by_words(const Table& t,
                                                    const uint32_t* __restrict__ dist,
                                                    const uint32_t* __restrict__ nh, uint32_t W,
                                                    uint32_t r, uint32_t lo, uint32_t hi,
                                                    uint32_t lane, uint32_t Wout,
                                                    uint32_t* __restrict__ o_nh,
                                                    const uint16_t* cslot, uint32_t ns,
                                                    bool want_links, Entry& e) {
  e = Entry{};
  const uint64_t kmin = policy_min(t, dist, lo, hi, lane);
  uint32_t need = 0, smallest = kInf, cnt = 0, links = 0;
  bool has_root = false;
  // the words wanted by neither output are not gathered; one pass over the
  // first word block still fills the entry
  const uint32_t wend = o_nh ? Wout : want_links ? W : 1u;
  for (uint32_t wb = 0; wb < wend; wb += 64) {
    const uint32_t w = wb + lane;
    uint32_t acc = 0;
    if (kmin != kNoKey && wb < W) {
      for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint32_t id = 0;
        uint64_t key = kNoKey;
        if (k < hi) key = key_at(t, dist, k, id);
        unsigned long long mask = __ballot(key == kmin);
        if (wb == 0) {
          cnt += (uint32_t)__popcll(mask);
          class_fold(t, key, kmin, k, id, r, need, smallest, has_root);
        }
        while (mask) {  // wave-uniform
          const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1u;
          mask &= mask - 1ull;
          const uint32_t a = lane_get(id, j);
          if ((o_nh || want_links) && w < W) acc |= nh[(size_t)a * W + w];
        }
      }
    }
    if (want_links)
      for (uint32_t bits = acc; bits; bits &= bits - 1u) {
        const uint32_t b = 32u * w + (uint32_t)__ffs((int)bits) - 1u;
        if (b < ns) links += cslot[b];
      }
    if (o_nh && w < Wout) o_nh[w] = acc;
  }
  if (kmin != kNoKey) {
    e.cnt = cnt;
    policy_reduce(need, smallest, has_root, r, kmin, e);
  }
  return want_links ? wave_sum(links) : 0u;
}

// c[0 .. ns) of root r into LDS as u16 (the first ns halves of `lds`); lds
// holds 2 * a.cap words. Block-wide, with barriers. `a`: a kernel's arguments
// with the loaded graph's row_ptr / colx / w / didx, hop and cap (LDS slots).
// A count always fits its half: a slot counts entries of one parallel group,
// and the load (ospf_load_graph, ospf_update_rows) refuses a group of more
// than OSPF_MAX_PARALLEL_LINKS = 0xFFFF entries with OSPF_E_RANGE. The min()
// of the pack below is therefore never the smaller side; `links` is the plain
// sum of c(r, k) that include/openr_spf.h defines.
template <class Args>
__device__ __forceinline__ void build_links(const Args& a, uint32_t r, uint32_t ns,
                                            uint32_t* lds) {
  uint32_t* minw = lds;
  uint32_t* c32 = lds + a.cap;
  const uint32_t lo = a.row_ptr[r], hi = a.row_ptr[r + 1];
  __syncthreads();  // the previous root's counts are read no more
  for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) {
    minw[i] = kInf;
    c32[i] = 0;
  }
  __syncthreads();
  if (!a.hop) {
    for (uint32_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
      const uint32_t d = a.didx[e];
      if (!(a.colx[e] & 0x80000000u) && d < ns) atomicMin(&minw[d], a.w[e]);
    }
    __syncthreads();
  }
  for (uint32_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
    const uint32_t d = a.didx[e];
    if ((a.colx[e] & 0x80000000u) || d >= ns) continue;
    if (a.hop || a.w[e] == minw[d]) atomicAdd(&c32[d], 1u);
  }
  __syncthreads();
  // pack slot i's count into half i of the minw words (dead by now; the u32
  // counts lie behind them and are not overwritten)
  uint16_t* c16 = reinterpret_cast<uint16_t*>(lds);
  for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) c16[i] = (uint16_t)min(c32[i], 0xFFFFu);
  __syncthreads();
}

// the next-hop links of an entry whose words one lane holds (W <= kSelLaneW)
__device__ __forceinline__ uint32_t links_of(const uint32_t (&acc)[kSelLaneW], uint32_t W,
                                             const uint16_t* cslot, uint32_t ns) {
  uint32_t links = 0;
#pragma unroll
  for (uint32_t w = 0; w < kSelLaneW; ++w)
    if (w < W)
      for (uint32_t bits = acc[w]; bits; bits &= bits - 1u) {
        const uint32_t b = 32u * w + (uint32_t)__ffs((int)bits) - 1u;
        if (b < ns) links += cslot[b];
      }
  return links;
}

// The [n][Wout] next-hop words of a chunk of n <= 64 prefixes whose words the
// prefixes' own lanes hold (W <= kSelLaneW), written cooperatively by the
// wave: every word once, zero padding included (select_kernel's store).
__device__ __forceinline__ void store_chunk_words(uint32_t* __restrict__ dst, bool aligned16,
                                                  const uint32_t (&acc)[kSelLaneW], uint32_t W,
                                                  uint32_t Wout, uint32_t n, uint32_t lane,
                                                  bool in) {
  if (Wout == 1u) {
    if (in) dst[lane] = acc[0];
  } else if (!(Wout & 3u) && aligned16) {
    // 16-B stores: quad q of the region is quad q % (Wout / 4) of prefix
    // q / (Wout / 4); a root's words are the first quad, the rest padding
    const uint32_t W4 = Wout >> 2, total = n * W4;
    for (uint32_t i0 = 0; i0 < total; i0 += 64) {  // wave-uniform trips (shuffles)
      const uint32_t i = i0 + lane;
      const bool ok = i < total;
      const uint32_t pl = ok ? i / W4 : 0u;
      const bool first = i == pl * W4;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (0 < W) v.x = lane_get(acc[0], pl);
      if (1 < W) v.y = lane_get(acc[1], pl);
      if (2 < W) v.z = lane_get(acc[2], pl);
      if (3 < W) v.w = lane_get(acc[3], pl);
      if (!first) v = make_uint4(0u, 0u, 0u, 0u);
      if (ok) reinterpret_cast<uint4*>(dst)[i] = v;
    }
  } else {
    const uint32_t total = n * Wout;
    for (uint32_t i0 = 0; i0 < total; i0 += 64) {  // wave-uniform trips (shuffles)
      const uint32_t i = i0 + lane;
      const bool ok = i < total;
      const uint32_t pl = ok ? i / Wout : 0u;
      const uint32_t w = i - pl * Wout;
      uint32_t v = 0;
#pragma unroll
      for (uint32_t k = 0; k < kSelLaneW; ++k)
        if (k < W) {
          const uint32_t x = lane_get(acc[k], pl);
          if (w == k) v = x;
        }
      if (ok) dst[i] = v;
    }
  }
}

}  // namespace ospf_selpol
