// spf_selsrmpls.hip — route selection for prefixes forwarded as SR_MPLS over a
// sweep's resident rows (gfx950): selectBestPathsSpf with perDestination = true
// (openr/decision/SpfSolver.cpp:772-845, getNextHopsWithMetric :1043-1089,
// getNextHopsThrift :1163-1285). The route is a set of (next hop, destination)
// pairs, so the next-hop words of the selected announcers are kept apart, one
// row of words per table ENTRY, instead of ORed into one bitset per prefix as
// policy_kernel (spf_selpolicy.hip) does for an IP route; and an announcing
// root whose own entry has a prepend label routes to the other announcers
// (filteredBestNodeAreas, :794-802). The rule is spelled out at
// ospf_sweep_select_srmpls in include/openr_spf.h; key, Entry, the class fold,
// c(r, k) in LDS and the chunk store are spf_selpolicy_dev.h's.
//
// Shape: policy_kernel's. A workgroup per root (grid-stride), c(r, k) built
// once per root in LDS, the waves striding over chunks of 64 prefixes. A
// prefix is two passes:
//   1. sr_entry: the smallest key over R (it names S and S', so need and best)
//      and the smallest key over D (the root's flagged entry skipped), then
//      need / best / count under them. A prefix of <= kSelShort entries is its
//      own lane's, a longer one the wave's with a lane per entry; either way
//      the result is parked in the prefix's lane.
//   2. the per-entry write. The entries of a chunk's prefixes are one
//      contiguous range of the table, so the wave walks it with a lane per
//      entry: the entry's owner is found among the lanes' offsets, its row
//      words are gathered masked by key_i == the owner's minimum over D, their
//      links summed through the LDS slots and stored, the words stored by
//      store_chunk_words (16-B stores when aligned). The prefix's `links` is
//      its segment of a wave prefix sum of the entries' links.
//   A root of more than kSelLaneW words takes pass 2 with a lane per word.
// Every word of a wanted output is written once by plain vector stores; no
// memset, no global atomics, no scratch.
//
// Out of scope (include/openr_spf.h says so too): this selection in
// ospf_selstate_* / ospf_areastate_*, several areas, ospf_msweep, KSP2, label
// validity and PUSH stacks, static MPLS next hops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "spf_selpolicy_dev.h"
#include "sweep_impl.h"

namespace {

using namespace ospf_sel;
using namespace ospf_selpol;

struct SrArgs {
  const ospf_int::SelRow* rows;  // [n_roots], owned-roots order
  const uint32_t* roots;         // [n_roots] their node ids
  uint32_t n_roots, P, A, Wout, hop;
  uint32_t cap;                  // LDS slots (>= every root's distinct neighbours)
  Table t;
  const uint32_t* flags;         // parallel to t.nodes, or null: all 0
  // the loaded graph: the root's CSR row
  const uint32_t* row_ptr;
  const uint32_t* colx;
  const uint32_t* w;
  const uint16_t* didx;
  const uint32_t* dn_off;
  uint32_t *o_metric, *o_count, *o_links, *o_need, *o_best, *o_dlinks, *o_dnh;
};

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o);
    if (lane >= (uint32_t)o) v += u;
  }
  return v;
}

// entry k is the root's own and leaves D (filteredBestNodeAreas)
__device__ __forceinline__ bool self_prepend(const uint32_t* flags, uint32_t k, uint32_t id,
                                             uint32_t r) {
  return id == r && flags && (flags[k] & OSPF_SEL_SELF_PREPEND);
}

// Pass 1 of a prefix: its Entry (m and cnt over D, need and best over S' and
// S) and, returned, the smallest key over D -- kNoKey when D is empty, so that
// no entry's key matches it. kWave: by the whole wave with a lane per entry,
// wave-uniform result; else by the calling lane alone.
template <bool kWave>
__device__ __forceinline__ uint64_t sr_entry(const Table& t, const uint32_t* flags,
                                             const uint32_t* __restrict__ dist, uint32_t r,
                                             uint32_t lo, uint32_t hi, uint32_t lane, Entry& e) {
  e = Entry{};
  const uint32_t k0 = kWave ? lo + lane : lo, step = kWave ? 64u : 1u;
  uint64_t kmin = kNoKey, kd = kNoKey;
  for (uint32_t k = k0; k < hi; k += step) {
    uint32_t id;
    const uint64_t key = key_at(t, dist, k, id);
    kmin = key < kmin ? key : kmin;
    if (!self_prepend(flags, k, id, r)) kd = key < kd ? key : kd;
  }
  if (kWave) {
    kmin = wave_min64(kmin);
    kd = wave_min64(kd);
  }
  if (kmin == kNoKey) return kNoKey;  // R is empty
  // D is a part of S': a smallest key outside S' means D is empty
  if ((kd >> 32) != (kmin >> 32)) kd = kNoKey;
  uint32_t need = 0, smallest = kInf, cnt = 0;
  bool has_root = false;
  for (uint32_t k = k0; k < hi; k += step) {
    uint32_t id;
    const uint64_t key = key_at(t, dist, k, id);
    class_fold(t, key, kmin, k, id, r, need, smallest, has_root);
    cnt += key != kNoKey && key == kd && !self_prepend(flags, k, id, r);
  }
  if (kWave) {
    policy_reduce(need, smallest, has_root, r, kmin, e);
    cnt = wave_sum(cnt);
  } else {
    e.need = need;
    e.best = best_of(smallest, has_root, r);
  }
  e.m = kd == kNoKey ? kInf : (uint32_t)kd;
  e.cnt = cnt;
  return kd;
}

// Pass 2 of a chunk of n <= 64 prefixes of a root of W <= kSelLaneW words, by
// the wave with a lane per entry. lo / hi: the lane's prefix's entry range
// (lanes >= n: empty), kd: its smallest key over D. Writes dst_links / dst_nh
// of the chunk's entries (pointers at this root's first entry, or null) and
// returns the lane's prefix's `links` (0 unless want_sum).
__device__ __forceinline__ uint32_t sr_write_by_lane(
    const Table& t, const uint32_t* __restrict__ dist, const uint32_t* __restrict__ nh, uint32_t W,
    uint32_t r, uint32_t lo, uint32_t hi, uint64_t kd, uint32_t n, uint32_t lane, uint32_t Wout,
    uint32_t* __restrict__ o_dlinks, uint32_t* __restrict__ o_dnh, bool aligned16,
    const uint16_t* cslot, uint32_t ns, bool want_sum) {
  const uint32_t kb = lane_get(lo, 0), ke = lane_get(hi, n - 1u);
  if (lane >= n) lo = hi = ke;  // hi ascends over all 64 lanes
  const uint32_t kdlo = (uint32_t)kd, kdhi = (uint32_t)(kd >> 32);
  uint32_t links = 0;
  for (uint32_t k0 = kb; k0 < ke; k0 += 64) {  // wave-uniform trips (shuffles)
    const uint32_t k = k0 + lane;
    const bool ok = k < ke;
    // the entry's prefix: the first lane whose range ends behind k
    const uint32_t kk = ok ? k : ke - 1u;
    uint32_t j = 0;
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1)
      if (lane_get(hi, j + s - 1u) <= kk) j += s;
    const uint64_t okd = ((uint64_t)lane_get(kdhi, j) << 32) | lane_get(kdlo, j);
    uint32_t acc[kSelLaneW];
#pragma unroll
    for (uint32_t w = 0; w < kSelLaneW; ++w) acc[w] = 0;
    if (ok) {
      uint32_t id;
      const uint64_t key = key_at(t, dist, k, id);
      if (key != kNoKey && key == okd && id != r) {
        const uint32_t* row = nh + (size_t)id * W;
#pragma unroll
        for (uint32_t w = 0; w < kSelLaneW; ++w)
          if (w < W) acc[w] = row[w];
      }
    }
    const uint32_t dl = want_sum ? links_of(acc, W, cslot, ns) : 0u;
    if (o_dlinks && ok) o_dlinks[k] = dl;
    if (o_dnh)
      store_chunk_words(o_dnh + (size_t)k0 * Wout, aligned16, acc, W, Wout, min(64u, ke - k0),
                        lane, ok);
    if (want_sum) {
      // the prefix's entries of this batch are lanes [s - k0, e - k0)
      const uint32_t scan = wave_scan(dl, lane);
      const uint32_t s = max(lo, k0), e = min(hi, k0 + 64u);
      const bool some = s < e;
      const uint32_t upto = lane_get(scan, some ? e - 1u - k0 : 0u);
      const uint32_t before = lane_get(scan, some && s > k0 ? s - 1u - k0 : 0u);
      if (some) links += upto - (s > k0 ? before : 0u);
    }
  }
  return links;
}

// Pass 2 of one prefix of a root of W > kSelLaneW words, by the wave with a
// lane per next-hop word; the same outputs, `links` wave-uniform.
__device__ __forceinline__ uint32_t sr_write_by_words(
    const Table& t, const uint32_t* __restrict__ dist, const uint32_t* __restrict__ nh, uint32_t W,
    uint32_t r, uint32_t lo, uint32_t hi, uint64_t kd, uint32_t lane, uint32_t Wout,
    uint32_t* __restrict__ o_dlinks, uint32_t* __restrict__ o_dnh, const uint16_t* cslot,
    uint32_t ns, bool want_sum) {
  uint32_t links = 0;
  for (uint32_t k0 = lo; k0 < hi; k0 += 64) {  // wave-uniform trips (ballot, shuffles)
    const uint32_t k = k0 + lane;
    const bool ok = k < hi;
    uint32_t id = 0;
    uint64_t key = kNoKey;
    if (ok) key = key_at(t, dist, k, id);
    const bool tight = key != kNoKey && key == kd && id != r;
    uint32_t dl = 0;
    if (want_sum)
      for (unsigned long long mask = __ballot(tight); mask; mask &= mask - 1ull) {  // wave-uniform
        const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1u;
        const uint32_t* row = nh + (size_t)lane_get(id, j) * W;
        uint32_t part = 0;
        for (uint32_t w = lane; w < W; w += 64)
          for (uint32_t bits = row[w]; bits; bits &= bits - 1u) {
            const uint32_t b = 32u * w + (uint32_t)__ffs((int)bits) - 1u;
            if (b < ns) part += cslot[b];
          }
        part = wave_sum(part);
        if (lane == j) dl = part;
      }
    if (o_dlinks && ok) o_dlinks[k] = dl;
    links += dl;
    if (o_dnh) {
      // the batch's entries' words as one flat region, a lane per word
      const uint32_t total = min(64u, hi - k0) * Wout;
      uint32_t* __restrict__ dst = o_dnh + (size_t)k0 * Wout;
      for (uint32_t x0 = 0; x0 < total; x0 += 64) {  // wave-uniform trips (shuffles)
        const uint32_t x = x0 + lane;
        const bool in = x < total;
        const uint32_t i = in ? x / Wout : 0u, w = x - i * Wout;
        const uint32_t a = lane_get(id, i);
        const bool take = lane_get((uint32_t)tight, i) != 0u && in && w < W;
        const uint32_t v = take ? nh[(size_t)a * W + w] : 0u;
        if (in) dst[x] = v;
      }
    }
  }
  return want_sum ? wave_sum(links) : 0u;
}

__global__ __launch_bounds__(256) void srmpls_kernel(const SrArgs a) {
  extern __shared__ uint32_t lds[];
  const uint16_t* cslot = reinterpret_cast<const uint16_t*>(lds);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P, Wout = a.Wout;
  const bool want_sum = a.o_links != nullptr || a.o_dlinks != nullptr;
  const bool pass2 = want_sum || a.o_dnh != nullptr;
  const bool aligned16 = !((uintptr_t)a.o_dnh & 15u);
  for (uint32_t ri = blockIdx.x; ri < a.n_roots; ri += gridDim.x) {
    const uint32_t* __restrict__ dist = a.rows[ri].dist;
    const uint32_t* __restrict__ nh = a.rows[ri].nh;
    const uint32_t W = a.rows[ri].W;
    const uint32_t r = a.roots[ri];
    const uint32_t ns = min(a.dn_off[r + 1] - a.dn_off[r], a.cap);
    const size_t ob = (size_t)ri * P, eb = (size_t)ri * a.A;
    uint32_t* o_dlinks = a.o_dlinks ? a.o_dlinks + eb : nullptr;
    uint32_t* o_dnh = a.o_dnh ? a.o_dnh + eb * Wout : nullptr;
    if (want_sum) build_links(a, r, ns, lds);  // block-uniform
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
      uint64_t kd = kNoKey;
      uint32_t links = 0;
      if (W <= kSelLaneW) {
        const bool mine = in && hi - lo <= kSelShort;
        if (mine) kd = sr_entry<false>(a.t, a.flags, dist, r, lo, hi, 0u, e);
        // the chunk's long prefixes, one at a time by the wave; the result
        // parked in the prefix's own lane
        for (unsigned long long t = __ballot(in && !mine); t; t &= t - 1ull) {
          const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
          Entry we;
          const uint64_t wk =
              sr_entry<true>(a.t, a.flags, dist, r, lane_get(lo, j), lane_get(hi, j), lane, we);
          if (lane == j) {
            e = we;
            kd = wk;
          }
        }
        if (pass2)
          links = sr_write_by_lane(a.t, dist, nh, W, r, lo, hi, kd, n, lane, Wout, o_dlinks, o_dnh,
                                   aligned16, cslot, ns, want_sum);
      } else {
        for (uint32_t j = 0; j < n; ++j) {
          Entry we;
          const uint32_t jlo = lane_get(lo, j), jhi = lane_get(hi, j);
          const uint64_t wk = sr_entry<true>(a.t, a.flags, dist, r, jlo, jhi, lane, we);
          uint32_t wl = 0;
          if (pass2)
            wl = sr_write_by_words(a.t, dist, nh, W, r, jlo, jhi, wk, lane, Wout, o_dlinks, o_dnh,
                                   cslot, ns, want_sum);
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

// device outputs of one call (only the wanted ones of `want`), freed by the
// destructor
struct SrOut {
  ospf_select_sout o{};
  ~SrOut() {
    for (uint32_t* p : {o.metric, o.count, o.links, o.need, o.best, o.dst_links, o.dst_nh})
      if (p) (void)hipFree(p);
  }
  bool alloc(size_t cells, size_t ents, uint32_t W, const ospf_select_sout* want) {
    auto get = [](bool wanted, uint32_t** p, size_t words) {
      return !wanted || !words || hipMalloc((void**)p, words * 4) == hipSuccess;
    };
    return get(want->metric, &o.metric, cells) && get(want->count, &o.count, cells) &&
           get(want->links, &o.links, cells) && get(want->need, &o.need, cells) &&
           get(want->best, &o.best, cells) && get(want->dst_links, &o.dst_links, ents) &&
           get(want->dst_nh, &o.dst_nh, ents * W);
  }
};

// the call's contract: OSPF_OK, or the error with its reason set
int sr_check(ospf_sweep* s, const ospf_select_stable* t, uint32_t nh_words) {
  ospf_ctx* c = s->c;
  if (!s->ran) return sfail(s, OSPF_E_INVAL, "sweep: select before the first run");
  const ospf_select_ptable pt{t->n_prefixes, t->offsets, t->nodes, t->pref, t->min_nexthop};
  if (const char* bad = select_ptable_check(&pt, s->V)) return sfail(s, OSPF_E_INVAL, bad);
  const size_t A = t->n_prefixes ? t->offsets[t->n_prefixes] : 0u;
  if (t->flags)
    for (size_t k = 0; k < A; ++k)
      if (t->flags[k] & ~OSPF_SEL_SELF_PREPEND)
        return sfail(s, OSPF_E_INVAL, "select srmpls: a flag word with unknown bits");
  if (nh_words < policy_row_words(s))
    return sfail(s, OSPF_E_INVAL, "sweep: nh_words below a root's next-hop words");
  // the kernel reads the live CSR and no-transit bits beside the rows
  if (!c || !c->loaded || c->graph_gen != s->gen || c->mask.on || c->info.n_nodes != s->V)
    return sfail(s, OSPF_E_INVAL, "select srmpls: the graph changed since the sweep was created");
  if (A > 0xFFFFFFFFull / std::max(1u, nh_words))
    return sfail(s, OSPF_E_RANGE, "select srmpls: entries x nh_words beyond 2^32 words a root");
  return OSPF_OK;
}

}  // namespace

int ospf_int::sweep::srmpls_queue(ospf_sweep* s, const ospf_select_stable* t, uint32_t nh_words,
                                  const ospf_select_sout* d_out, void* stream) {
  if (const int rc = sr_check(s, t, nh_words)) return rc;
  ospf_ctx* c = s->c;
  const ospf_select_ptable pt{t->n_prefixes, t->offsets, t->nodes, t->pref, t->min_nexthop};
  const uint32_t n = (uint32_t)s->roots.size(), P = t->n_prefixes;
  const size_t A = P ? t->offsets[P] : 0u;
  const bool cells = d_out->metric || d_out->count || d_out->links || d_out->need || d_out->best;
  const bool ents = A && (d_out->dst_links || d_out->dst_nh);
  if (!n || !P || (!cells && !ents)) return OSPF_OK;
  const bool sums = d_out->links || d_out->dst_links;
  const uint32_t cap = std::max(1u, c->max_dn);
  const size_t lds = sums ? (size_t)cap * 8 : 0;
  if (lds > c->lds_limit)
    return sfail(s, OSPF_E_RANGE, "select srmpls: the widest root's link counts do not fit the LDS");
  PolicyTab d{};
  if (const int rc = policy_upload(s, &pt, t->flags, &d)) return rc;
  SrArgs a{};
  a.rows = s->d_sel_rows;
  a.roots = s->d_pol_roots;
  a.n_roots = n;
  a.P = P;
  a.A = (uint32_t)A;
  a.Wout = nh_words;
  a.hop = (s->opts.flags & OSPF_HOP_COUNT) ? 1u : 0u;
  a.cap = cap;
  a.t = Table{d.off, d.nodes, d.pref, d.mnh, c->g.nt_bits};
  a.flags = d.flags;
  a.row_ptr = c->g.row_ptr;
  a.colx = c->g.colx;
  a.w = c->g.w;
  a.didx = c->g.didx;
  a.dn_off = c->g.dn_off;
  a.o_metric = d_out->metric;
  a.o_count = d_out->count;
  a.o_links = d_out->links;
  a.o_need = d_out->need;
  a.o_best = d_out->best;
  a.o_dlinks = A ? d_out->dst_links : nullptr;
  a.o_dnh = A ? d_out->dst_nh : nullptr;
  // policy_kernel's launch shape: a wave per 64 prefixes of the root, at most 4
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  const uint32_t grid = std::min(n, 1u << 20);
  hipLaunchKernelGGL(srmpls_kernel, dim3(grid), dim3(64u * waves), lds, (hipStream_t)stream, a);
  SCHK(s, hipGetLastError());
  SCHK(s, hipEventRecord(s->pol_ev, (hipStream_t)stream));
  return OSPF_OK;
}

extern "C" {

int ospf_sweep_select_srmpls_dev(ospf_sweep* s, const ospf_select_stable* t, uint32_t nh_words,
                                 const ospf_select_sout* d_out, void* stream) {
  if (!s || !t || !d_out) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  return srmpls_queue(s, t, nh_words, d_out, stream);
}

int ospf_sweep_select_srmpls(ospf_sweep* s, const ospf_select_stable* t, uint32_t nh_words,
                             const ospf_select_sout* out) {
  if (!s || !t || !out) return OSPF_E_INVAL;
  if (ospf_int::injected(s->c)) return sfail(s, OSPF_E_DEVICE, s->c->err);
  if (const int rc = sr_check(s, t, nh_words)) return rc;  // before its sizes are used
  const size_t n = s->roots.size(), P = t->n_prefixes, A = P ? t->offsets[P] : 0u;
  const size_t cells = n * P, ents = n * A;
  SrOut d;
  if (cells) {
    SCHK(s, hipSetDevice(s->c->device));
    SCHK(s, hipDeviceSynchronize());  // the rows, whichever streams ran the sweep
    if (!d.alloc(cells, ents, std::max(1u, nh_words), out)) {
      (void)hipGetLastError();
      return sfail(s, OSPF_E_NOMEM, "select srmpls: hipMalloc of the outputs");
    }
  }
  const int rc = srmpls_queue(s, t, nh_words, &d.o, nullptr);
  if (rc || !cells) return rc;
  // into buffers of this call first: a failed copy leaves the caller's as they were
  std::vector<uint32_t> h[7];
  uint32_t* const src[7] = {d.o.metric, d.o.count, d.o.links, d.o.need,
                            d.o.best,   d.o.dst_links, d.o.dst_nh};
  uint32_t* const dst[7] = {out->metric, out->count, out->links, out->need,
                            out->best,   out->dst_links, out->dst_nh};
  for (int i = 0; i < 7; ++i) {
    if (!src[i]) continue;
    h[i].resize(i < 5 ? cells : i == 5 ? ents : ents * nh_words);
    SCHK(s, hipMemcpy(h[i].data(), src[i], h[i].size() * 4, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 7; ++i)
    if (src[i]) std::copy(h[i].begin(), h[i].end(), dst[i]);
  return OSPF_OK;
}

}  // extern "C"
