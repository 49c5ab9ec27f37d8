// spf_selareas_dev.h — the per-prefix device functions of route selection
// across several areas (spf_selareas.hip: areas_kernel, the one-shot
// selection; spf_seldelta_areas.hip: areas_delta_kernel, the resident
// selection and its delta). The rule is spelled out at
// ospf_areas_select_policy in include/openr_spf.h and the four walks per
// (global root, prefix) in spf_selareas.hip's banner; the three strategies per
// prefix are those of spf_selpolicy_dev.h: a short prefix by its own lane, a
// long one by the wave with a lane per entry, the words of a wide area with a
// lane per word. Device code only; not a public header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_selpolicy_dev.h"

namespace ospf_selareas {

using namespace ospf_sel;
using namespace ospf_selpol;

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxAreas = 32;

// the table on the device: entries (global node, area) with the node's id in
// its own area beside them
struct Tab {
  const uint32_t* off;   // [P + 1]
  const uint32_t* node;  // global ids
  const uint32_t* area;
  const uint32_t* loc;   // the node's id in the entry's area
  const uint32_t* pref;
  const uint32_t* mnh;   // or null: all unset
};

// an area of the block's root (LDS)
struct RootArea {
  const uint32_t* dist;  // the root's rows in the area
  const uint32_t* nh;
  const uint32_t* lid;
  const uint32_t* nt;
  uint32_t* o_nh;        // the root's [P][Wout] words, or null
  uint32_t W, Wout;
  uint32_t la;           // the root's id in the area, kNone: not in it
  uint32_t ns, coff;     // neighbour slots, and where their link counts start
};

// build_links' view of an area
struct LinkArgs {
  const uint32_t* row_ptr;
  const uint32_t* colx;
  const uint32_t* w;
  const uint16_t* didx;
  uint32_t hop, cap;
};

// what a (root, prefix) cell holds beside the per-area words
struct Sel {
  uint32_t m = kInf, need = 0, best = kNone;
  uint32_t win = 0;  // the winning areas; 0: R is empty
  uint32_t cls = 0;  // the high word of the smallest key: S' = {key >> 32 == cls}
  uint32_t sp = 0;   // by-lane: bit i = entry lo + i is in S'
};

// key of entry k as the root sees it in the entry's own area (kNoKey: the root
// is not in that area, or does not reach the node there)
__device__ __forceinline__ uint64_t key_at(const Tab& t, const RootArea* ra, uint32_t k) {
  const RootArea& x = ra[t.area[k]];
  if (x.la == kNone) return kNoKey;
  const uint32_t ln = t.loc[k];
  const uint32_t d = x.dist[ln];
  if (d == kInf) return kNoKey;
  const uint32_t drained = (x.nt[ln >> 5] >> (ln & 31u)) & 1u;
  return ((uint64_t)t.pref[k] << 33) | ((uint64_t)drained << 32) | d;
}

__device__ __forceinline__ bool in_sp(uint64_t key, uint32_t cls) {
  return key != kNoKey && (uint32_t)(key >> 32) == cls;
}

// entry k's node looked up in area a (x = ra[a]): its id there (kNone: absent)
// and the root's distance to it (kInf: absent or not reached)
__device__ __forceinline__ uint32_t dist_in(const Tab& t, const RootArea& x, uint32_t a, uint32_t k,
                                            uint32_t& ln) {
  ln = t.area[k] == a ? t.loc[k] : x.lid[t.node[k]];
  return ln == kNone ? kInf : x.dist[ln];
}

// area a's metric m_a into the cell: the smallest wins, ties share
__device__ __forceinline__ void take_area(Sel& s, uint32_t a, uint32_t ma) {
  if (ma < s.m) {
    s.m = ma;
    s.win = 0;
  }
  if (ma == s.m && ma != kInf) s.win |= 1u << a;
}

// walks 1-3 of a short prefix by its own lane
__device__ __forceinline__ Sel sel_by_lane(const Tab& t, const RootArea* ra, uint32_t g, uint32_t lo,
                                           uint32_t hi) {
  Sel s;
  uint64_t kmin = kNoKey;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint64_t key = key_at(t, ra, k);
    kmin = key < kmin ? key : kmin;
  }
  if (kmin == kNoKey) return s;
  s.cls = (uint32_t)(kmin >> 32);
  uint32_t first = kNone, first_root = kNone, own = 0;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint64_t key = key_at(t, ra, k);
    if (key == kNoKey) continue;
    if ((key >> 33) == (kmin >> 33)) {
      first = min(first, k - lo);
      if (t.node[k] == g) first_root = min(first_root, k - lo);
    }
    if (in_sp(key, s.cls)) {
      s.sp |= 1u << (k - lo);
      own |= 1u << t.area[k];
      if (t.mnh) s.need = max(s.need, t.mnh[k]);
    }
  }
  s.best = first_root != kNone ? first_root : first;
  for (uint32_t as = own; as; as &= as - 1u) {
    const uint32_t a = (uint32_t)__ffs((int)as) - 1u;
    uint32_t ma = kInf;
    for (uint32_t b = s.sp; b; b &= b - 1u) {
      uint32_t ln;
      ma = min(ma, dist_in(t, ra[a], a, lo + (uint32_t)__ffs((int)b) - 1u, ln));
    }
    take_area(s, a, ma);
  }
  return s;
}

// walk 4 of a short prefix by its own lane in a winning area a (W <= kSelLaneW):
// the nodes of S' at the metric, each once (the entries of one node are
// neighbours in the (node, area) order)
__device__ __forceinline__ void area_by_lane(const Tab& t, const RootArea& x, uint32_t a,
                                             uint32_t lo, const Sel& s, bool want_words,
                                             uint32_t& cnt, uint32_t (&acc)[kSelLaneW]) {
  uint32_t prev = kNone;
  for (uint32_t b = s.sp; b; b &= b - 1u) {
    const uint32_t k = lo + (uint32_t)__ffs((int)b) - 1u;
    uint32_t ln;
    if (dist_in(t, x, a, k, ln) != s.m) continue;
    const uint32_t n = t.node[k];
    if (n == prev) continue;
    prev = n;
    ++cnt;
    if (want_words) {
      const uint32_t* row = x.nh + (size_t)ln * x.W;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w)
        if (w < x.W) acc[w] |= row[w];
    }
  }
}

// walks 1-3 of any prefix by the whole wave, a lane per entry: wave-uniform
__device__ __forceinline__ Sel sel_by_wave(const Tab& t, const RootArea* ra, uint32_t g, uint32_t lo,
                                           uint32_t hi, uint32_t lane) {
  Sel s;
  uint64_t kmin = kNoKey;
  for (uint32_t k = lo + lane; k < hi; k += 64) {
    const uint64_t key = key_at(t, ra, k);
    kmin = key < kmin ? key : kmin;
  }
  kmin = wave_min64(kmin);
  if (kmin == kNoKey) return s;  // wave-uniform
  s.cls = (uint32_t)(kmin >> 32);
  uint32_t first = kNone, first_root = kNone, own = 0, need = 0;
  for (uint32_t k = lo + lane; k < hi; k += 64) {
    const uint64_t key = key_at(t, ra, k);
    if (key == kNoKey) continue;
    if ((key >> 33) == (kmin >> 33)) {
      first = min(first, k - lo);
      if (t.node[k] == g) first_root = min(first_root, k - lo);
    }
    if (in_sp(key, s.cls)) {
      own |= 1u << t.area[k];
      if (t.mnh) need = max(need, t.mnh[k]);
    }
  }
  s.need = wave_max(need);
  first = wave_min(first);
  first_root = wave_min(first_root);
  s.best = first_root != kNone ? first_root : first;
  own = wave_or(own);
  for (uint32_t as = own; as; as &= as - 1u) {  // wave-uniform
    const uint32_t a = (uint32_t)__ffs((int)as) - 1u;
    uint32_t ma = kInf;
    for (uint32_t k = lo + lane; k < hi; k += 64)
      if (in_sp(key_at(t, ra, k), s.cls)) {
        uint32_t ln;
        ma = min(ma, dist_in(t, ra[a], a, k, ln));
      }
    take_area(s, a, wave_min(ma));
  }
  return s;
}

// One 64-entry step of walk 4 by the wave in area a: the lane's entry k (when
// below hi) is `fresh` when it is in S', at the metric in a and the first entry
// of its node there. `carry` is the node of the last entry at the metric so far
// (wave-uniform). Returns the ballot of the entries at the metric.
__device__ __forceinline__ unsigned long long tight_step(const Tab& t, const RootArea* ra,
                                                         uint32_t a, uint32_t k, uint32_t hi,
                                                         const Sel& s, uint32_t lane,
                                                         uint32_t& carry, uint32_t& ln,
                                                         bool& fresh) {
  uint32_t n = kNone;
  bool tight = false;
  ln = kNone;
  if (k < hi && in_sp(key_at(t, ra, k), s.cls)) {
    tight = dist_in(t, ra[a], a, k, ln) == s.m;
    n = t.node[k];
  }
  const unsigned long long mask = __ballot(tight);
  const unsigned long long below = mask & ((1ull << lane) - 1ull);
  const uint32_t src = below ? 63u - (uint32_t)__clzll((long long)below) : 0u;
  const uint32_t pn = lane_get(n, src);  // every lane shuffles
  fresh = tight && (below ? pn : carry) != n;
  if (mask) carry = lane_get(n, 63u - (uint32_t)__clzll((long long)mask));
  return mask;
}

// walk 4 of any prefix by the wave in a winning area a of <= kSelLaneW words:
// wave-uniform count and words
__device__ __forceinline__ void area_by_wave(const Tab& t, const RootArea* ra, uint32_t a,
                                             uint32_t lo, uint32_t hi, const Sel& s, uint32_t lane,
                                             bool want_words, uint32_t& cnt,
                                             uint32_t (&acc)[kSelLaneW]) {
  const RootArea& x = ra[a];
  uint32_t carry = kNone;
  for (uint32_t k0 = lo; k0 < hi; k0 += 64) {  // wave-uniform trips (ballot)
    uint32_t ln;
    bool fresh;
    tight_step(t, ra, a, k0 + lane, hi, s, lane, carry, ln, fresh);
    cnt += (uint32_t)__popcll(__ballot(fresh));
    if (fresh && want_words) {
      const uint32_t* row = x.nh + (size_t)ln * x.W;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w)
        if (w < x.W) acc[w] |= row[w];
    }
  }
  if (want_words) {
#pragma unroll
    for (uint32_t w = 0; w < kSelLaneW; ++w)
      if (w < x.W) acc[w] = wave_or(acc[w]);
  }
}

// walk 4 of any prefix by the wave in an area a of more than kSelLaneW words,
// a lane per word: writes the prefix's Wout words itself (o_nh: this prefix's
// words, or null; zero when a is no winning area) and returns, wave-uniform,
// the count in `cnt` and the links of the words (0 when not wanted).
__device__ __forceinline__ uint32_t area_by_words(const Tab& t, const RootArea* ra, uint32_t a,
                                                  uint32_t lo, uint32_t hi, const Sel& s,
                                                  uint32_t lane, uint32_t* __restrict__ o_nh,
                                                  const uint16_t* cslot, bool want_links,
                                                  uint32_t& cnt) {
  const RootArea& x = ra[a];
  const bool won = (s.win >> a) & 1u;  // wave-uniform
  uint32_t links = 0;
  // the words wanted by neither output are not gathered; one pass over the
  // first word block still counts
  const uint32_t wend = o_nh ? x.Wout : want_links ? x.W : 1u;
  for (uint32_t wb = 0; wb < wend; wb += 64) {
    const uint32_t w = wb + lane;
    uint32_t acc = 0;
    if (won && wb < x.W) {
      uint32_t carry = kNone;
      for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
        uint32_t ln;
        bool fresh;
        tight_step(t, ra, a, k0 + lane, hi, s, lane, carry, ln, fresh);
        unsigned long long mask = __ballot(fresh);
        if (wb == 0) cnt += (uint32_t)__popcll(mask);
        while (mask) {  // wave-uniform
          const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1u;
          mask &= mask - 1ull;
          const uint32_t id = lane_get(ln, j);
          if ((o_nh || want_links) && w < x.W) acc |= x.nh[(size_t)id * x.W + w];
        }
      }
    }
    if (want_links)
      for (uint32_t bits = acc; bits; bits &= bits - 1u) {
        const uint32_t b = 32u * w + (uint32_t)__ffs((int)bits) - 1u;
        if (b < x.ns) links += cslot[x.coff + b];
      }
    if (o_nh && w < x.Wout) o_nh[w] = acc;
  }
  return want_links ? wave_sum(links) : 0u;
}

}  // namespace ospf_selareas
