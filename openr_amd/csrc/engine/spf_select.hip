// spf_select.hip — anycast route selection over a sweep's resident rows
// (gfx950): SpfSolver::getNextHopsWithMetric (openr/decision/SpfSolver.cpp:
// 1043-1089) for every owned root of a sweep and every prefix of a table, in
// one launch. Per (root, prefix): the smallest distance over the prefix's
// reached announcers (:1064-1077), the number of announcers at that distance
// (minCostNodes) and the OR of their next-hop words (:1080-1086).
//
// Shape: a workgroup per root (grid-stride), so every gather of the block
// lands in the root's own two rows; its waves stride over the prefix table in
// chunks of 64 prefixes. Inside a chunk
//   * a prefix of <= kSelShort announcers (loopbacks, a pod's aggregate) is
//     one lane's: it walks its announcers serially;
//   * a longer prefix is the whole wave's: a lane per announcer and 64-stride,
//     pass 1 a wave min of the gathered distances, pass 2 re-reads the ids
//     (ascending: a coalesced load), the tight lanes load their W words, the
//     count is ballot + popcount and the words are OR-reduced across the wave;
//     its result is parked in the registers of the prefix's own lane.
//   The chunk's metric / count words are then one coalesced store per array
//   and its next-hop words one contiguous [64][Wout] region written
//   cooperatively (every word once, zero padding included; no atomics).
//   * roots with more than kSelLaneW next-hop words (a fabric's spines) take
//     every prefix by the wave with a lane per WORD instead: the tight
//     announcers are walked by ballot bit and each one's W words are one
//     coalesced load, OR-ed into the lane's word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spf_internal.h"
#include "spf_select_dev.h"

namespace {

using namespace ospf_sel;  // the per-prefix device functions (spf_select_dev.h)

__global__ __launch_bounds__(256) void select_kernel(
    const ospf_int::SelRow* __restrict__ rows, uint32_t n_roots,
    const uint32_t* __restrict__ off, const uint32_t* __restrict__ nodes, uint32_t P,
    uint32_t Wout, uint32_t* __restrict__ o_metric, uint32_t* __restrict__ o_count,
    uint32_t* __restrict__ o_nh) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  for (uint32_t ri = blockIdx.x; ri < n_roots; ri += gridDim.x) {
    const uint32_t* __restrict__ dist = rows[ri].dist;
    const uint32_t* __restrict__ nh = rows[ri].nh;
    const uint32_t W = rows[ri].W;
    const size_t ob = (size_t)ri * P;
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
      if (W <= kSelLaneW) {
        uint32_t acc[kSelLaneW];
#pragma unroll
        for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
        const bool mine = in && hi - lo <= kSelShort;
        const unsigned long long wide = __ballot(in && !mine);
        if (mine) {  // this lane's own short prefix
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
              if (o_nh) {
                const uint32_t* row = nh + (size_t)id * W;
#pragma unroll
                for (uint32_t w = 0; w < kSelLaneW; ++w)
                  if (w < W) acc[w] |= row[w];
              }
            }
          }
        }
        // the chunk's long prefixes, one at a time by the wave; the result
        // parked in the prefix's own lane
        for (unsigned long long t = wide; t; t &= t - 1ull) {
          const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
          uint32_t wm, wc, wa[kSelLaneW];
          prefix_by_lanes(dist, nh, W, nodes, lane_get(lo, j), lane_get(hi, j), lane,
                          o_nh != nullptr, wm, wc, wa);
          if (lane == j) {
            m = wm;
            cnt = wc;
#pragma unroll
            for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = wa[w];
          }
        }
        if (o_nh) {
          uint32_t* __restrict__ dst = o_nh + (ob + base) * Wout;
          if (Wout == 1u) {
            if (in) dst[lane] = acc[0];
          } else if (!(Wout & 3u) && !((uintptr_t)o_nh & 15u)) {
            // 16-B stores: quad q of the region is quad q % (Wout / 4) of
            // prefix q / (Wout / 4); a root's words (<= kSelLaneW = 4) are
            // the first quad, every other quad is padding
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
            // [n][Wout] words of the chunk, contiguous: word i of the region
            // is word i % Wout of prefix i / Wout
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
                  const uint32_t t = lane_get(acc[k], pl);
                  if (w == k) v = t;
                }
              if (ok) dst[i] = v;
            }
          }
        }
      } else {
        for (uint32_t j = 0; j < n; ++j) {
          uint32_t wm, wc;
          prefix_by_words(dist, nh, W, nodes, lane_get(lo, j), lane_get(hi, j), lane, Wout,
                          o_nh ? o_nh + (ob + base + j) * Wout : nullptr, wm, wc);
          if (lane == j) {
            m = wm;
            cnt = wc;
          }
        }
      }
      if (in) {
        if (o_metric) o_metric[ob + p] = m;
        if (o_count) o_count[ob + p] = cnt;
      }
    }
  }
}

}  // namespace

namespace ospf_int {

int select_launch(ospf_ctx* c, const SelRow* d_rows, uint32_t n_roots, const uint32_t* d_off,
                  const uint32_t* d_nodes, uint32_t n_prefixes, uint32_t nh_words,
                  uint32_t* d_metric, uint32_t* d_count, uint32_t* d_nh, void* stream) {
  if (!n_roots || !n_prefixes) return OSPF_OK;
  // a wave per 64 prefixes of the root, at most 4; roots beyond the grid by stride
  const uint32_t waves = std::min(4u, (n_prefixes + 63u) / 64u);
  const uint32_t grid = std::min(n_roots, 1u << 20);
  hipLaunchKernelGGL(select_kernel, dim3(grid), dim3(64u * waves), 0, (hipStream_t)stream, d_rows,
                     n_roots, d_off, d_nodes, n_prefixes, nh_words, d_metric, d_count, d_nh);
  HIPCHK(c, hipGetLastError());
  return OSPF_OK;
}

}  // namespace ospf_int
