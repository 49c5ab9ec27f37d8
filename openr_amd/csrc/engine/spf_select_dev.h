// spf_select_dev.h — the per-prefix device functions of anycast route
// selection, shared by spf_select.hip (select_kernel: the expanded [n][P][Wout]
// outputs) and spf_seldelta.hip (seldelta_kernel: the resident selection in
// each root's own width and its diff). Three strategies per prefix:
//   * a prefix of <= kSelShort announcers is one lane's (the kernels walk it
//     inline);
//   * prefix_by_lanes: a longer prefix by the whole wave, a lane per announcer
//     (roots of <= kSelLaneW next-hop words);
//   * prefix_by_words: any prefix by the whole wave, a lane per next-hop WORD
//     (roots of more words).
// Device code only; not a public header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ospf_sel {

constexpr uint32_t kInf = 0xFFFFFFFFu;  // OSPF_DIST_INF
constexpr uint32_t kSelShort = 8;       // lane-per-prefix up to this many announcers
constexpr uint32_t kSelLaneW = 4;       // lane-per-announcer up to this many next-hop words
static_assert(kSelLaneW == 4, "the 16-B store path packs a root's words into one quad");

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
  return v;
}

__device__ __forceinline__ uint32_t lane_get(uint32_t v, uint32_t src) {
  return (uint32_t)__shfl((int)v, (int)src);
}

// pass 1 of a wave's prefix: the smallest gathered distance (kInf: none reached)
__device__ __forceinline__ uint32_t prefix_min(const uint32_t* __restrict__ dist,
                                               const uint32_t* __restrict__ nodes, uint32_t lo,
                                               uint32_t hi, uint32_t lane) {
  uint32_t m = kInf;
  for (uint32_t k = lo + lane; k < hi; k += 64) m = min(m, dist[nodes[k]]);
  return wave_min(m);
}

// A short prefix by its own lane (W <= kSelLaneW), its announcers walked
// serially: select_kernel's inline walk as a function (m = kInf, cnt = 0 and
// acc = 0 on entry).
__device__ __forceinline__ void prefix_by_lane(const uint32_t* __restrict__ dist,
                                               const uint32_t* __restrict__ nh, uint32_t W,
                                               const uint32_t* __restrict__ nodes, uint32_t lo,
                                               uint32_t hi, uint32_t& m, uint32_t& cnt,
                                               uint32_t (&acc)[kSelLaneW]) {
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t id = nodes[k];
    const uint32_t d = dist[id];
    if (d < m) {
      m = d;
      cnt = 0;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
    }
    if (d == m && d != kInf) {
      ++cnt;
      const uint32_t* row = nh + (size_t)id * W;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w)
        if (w < W) acc[w] |= row[w];
    }
  }
}

// A long prefix by the whole wave, a lane per announcer (W <= kSelLaneW):
// wave-uniform metric, count and words.
__device__ __forceinline__ void prefix_by_lanes(const uint32_t* __restrict__ dist,
                                                const uint32_t* __restrict__ nh, uint32_t W,
                                                const uint32_t* __restrict__ nodes, uint32_t lo,
                                                uint32_t hi, uint32_t lane, bool want_nh,
                                                uint32_t& m, uint32_t& cnt,
                                                uint32_t (&acc)[kSelLaneW]) {
  m = prefix_min(dist, nodes, lo, hi, lane);
  cnt = 0;
#pragma unroll
  for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
  if (m == kInf) return;
  for (uint32_t k0 = lo; k0 < hi; k0 += 64) {  // wave-uniform trips (ballot)
    const uint32_t k = k0 + lane;
    uint32_t id = 0;
    bool tight = false;
    if (k < hi) {
      id = nodes[k];
      tight = dist[id] == m;
    }
    cnt += (uint32_t)__popcll(__ballot(tight));
    if (tight && want_nh) {
      const uint32_t* row = nh + (size_t)id * W;
#pragma unroll
      for (uint32_t w = 0; w < kSelLaneW; ++w)
        if (w < W) acc[w] |= row[w];
    }
  }
  if (want_nh) {
#pragma unroll
    for (uint32_t w = 0; w < kSelLaneW; ++w)
      if (w < W) acc[w] = wave_or(acc[w]);
  }
}

// Any prefix by the whole wave, a lane per next-hop word (W > kSelLaneW):
// writes the prefix's Wout words itself (o_nh: this prefix's words, or null).
__device__ __forceinline__ void prefix_by_words(const uint32_t* __restrict__ dist,
                                                const uint32_t* __restrict__ nh, uint32_t W,
                                                const uint32_t* __restrict__ nodes, uint32_t lo,
                                                uint32_t hi, uint32_t lane, uint32_t Wout,
                                                uint32_t* __restrict__ o_nh, uint32_t& m,
                                                uint32_t& cnt) {
  m = prefix_min(dist, nodes, lo, hi, lane);
  cnt = 0;
  // without words wanted one pass over the first word block still counts
  const uint32_t wend = o_nh ? Wout : 1u;
  for (uint32_t wb = 0; wb < wend; wb += 64) {
    const uint32_t w = wb + lane;
    uint32_t acc = 0;
    if (m != kInf && wb < W) {
      for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint32_t id = 0;
        bool tight = false;
        if (k < hi) {
          id = nodes[k];
          tight = dist[id] == m;
        }
        unsigned long long mask = __ballot(tight);
        if (wb == 0) cnt += (uint32_t)__popcll(mask);
        while (mask) {  // wave-uniform
          const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1u;
          mask &= mask - 1ull;
          const uint32_t a = lane_get(id, j);
          if (o_nh && w < W) acc |= nh[(size_t)a * W + w];
        }
      }
    }
    if (o_nh && w < Wout) o_nh[w] = acc;
  }
}

}  // namespace ospf_sel
