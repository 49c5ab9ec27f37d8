// spf_ucmp.hip — UCMP weights of every root and prefix on the device (gfx950):
// SpfSolver::getNodeUcmpResult -> LinkState::resolveUcmpWeights
// (openr/decision/SpfSolver.cpp:1091-1161, LinkState.cpp:913-1033) over the
// selection an ospf_selstate keeps resident, without a walk per root.
//
// The weight a node advertises in any root's walk is that of its own selection
// (DESIGN.md §3 o'''): W(u) = its leaf weight when u announces the prefix
// (selected metric 0), else the sum over u's selected next hops k of
// c(u, k) * W(k) (prefix-weight propagation) or of S(u, k) (adjacency-weight
// propagation), c = the tight links u - k, S = the sum of u's link weights on
// them. So the walk is a dependency-ordered gather over the state:
//
//   ucmp_links_kernel   c per (node, distinct neighbour) slot from the loaded
//                       CSR (up entries at the smallest metric towards the
//                       neighbour; every up entry under hop count): a block per
//                       node, atomicMin then atomicAdd on the node's own slots.
//   ucmp_round_kernel   round 0 settles the announcers (leaf weight, or VOID
//                       for a zero one) and the entries without a reached
//                       announcer (NONE), and marks the rest pending; round
//                       t >= 1 computes an entry when every selected next hop's
//                       entry was settled in a round < t. A workgroup per node,
//                       lane = prefix (chunks of 64), so the gathers W[k][p]
//                       of lanes that share a next hop coalesce. Roots of
//                       <= kSelLaneW words walk their set bits in the prefix's
//                       lane; wider roots take a prefix per wave, a lane per
//                       word and a wave reduction. The pending entries of a
//                       wave are counted with one atomicAdd; the host repeats
//                       rounds until the counter reads zero.
//   ucmp_view_kernel    the per-link view of some roots: per set next-hop bit
//                       W(k) divided by the gcd of the root's next-hop weights.
//
// An entry's tag holds its status and the round that settled it; a round
// trusts only tags of earlier rounds (earlier launches), so an entry settled
// by another workgroup in the same launch reads as pending whether or not its
// store is visible yet: the result and the round count (the hop depth of the
// deepest selected path) do not depend on scheduling.
// Over a policy state (spf_seldelta_policy.hip: five header columns before an
// entry's words) an announcer need not select itself, so a selected next hop
// whose no-transit bit is set counts with its leaf weight and is never waited
// for (drained_leaf; DESIGN.md §3 (q''')).
// No LDS, no scratch, no inline assembly; plain vector stores and atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "spf_select_dev.h"
#include "spf_selstate.h"

namespace {

using namespace ospf_sel;

constexpr uint32_t kPending = 0xFFFFFFFFu;  // tag of an entry not settled yet
constexpr uint32_t kRoundMask = 0x3FFFFFFFu;
constexpr uint64_t kI63 = 0x7FFFFFFFFFFFFFFFull;

__device__ __forceinline__ uint32_t make_tag(uint32_t status, uint32_t round) {
  return (status << 30) | round;
}

// ---------------------------------------------------------------- tight links
struct LinkArgs {
  ospf::DevGraph g;
  uint32_t hop;
  uint32_t* minw;  // [slots], kInf on entry
  uint32_t* c;     // [slots], 0 on entry
};

__global__ __launch_bounds__(256) void ucmp_links_kernel(const LinkArgs a) {
  for (uint32_t u = blockIdx.x; u < a.g.V; u += gridDim.x) {
    const uint32_t lo = a.g.row_ptr[u], hi = a.g.row_ptr[u + 1];
    const uint32_t s0 = a.g.dn_off[u], ns = a.g.dn_off[u + 1] - s0;
    if (!a.hop) {
      for (uint32_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
        const uint32_t d = a.g.didx[e];
        if (!(a.g.colx[e] & 0x80000000u) && d < ns) atomicMin(&a.minw[s0 + d], a.g.w[e]);
      }
      __threadfence();
      __syncthreads();  // the node's slots are this block's alone
    }
    for (uint32_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
      const uint32_t d = a.g.didx[e];
      if ((a.g.colx[e] & 0x80000000u) || d >= ns) continue;
      if (a.hop || a.g.w[e] == __hip_atomic_load(&a.minw[s0 + d], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
        atomicAdd(&a.c[s0 + d], 1u);
    }
  }
}

// ---------------------------------------------------------------- the rounds
struct RoundArgs {
  uint32_t V, P, round, adj;
  uint32_t hdr;     // header columns before an entry's words: 2, or 5 in a policy state
  uint32_t policy;  // the drained-leaf rule applies (a policy state)
  const uint32_t* nt_bits;  // the loaded graph's no-transit bitmap
  const uint32_t* data;  // the committed selection: root blocks
  const uint64_t* off;
  const uint32_t* w;
  const uint32_t* dn_off;
  const uint32_t* dn;
  const uint32_t* t_off;  // the prefix table
  const uint32_t* t_nodes;
  const int64_t* leaf_w;  // parallel to t_nodes
  const uint32_t* c;      // per distinct-neighbour slot
  const int64_t* S;       // per distinct-neighbour slot (adj)
  int64_t* W;             // [V][P]
  uint32_t* tag;          // [V][P]
  uint32_t* pending;      // entries still pending after this round
};

// One selected next hop's share of an entry, accumulated overflow-safe.
struct Acc {
  uint64_t sum = 0;
  bool wait = false, isvoid = false, ovf = false;
  __device__ __forceinline__ void add(uint64_t x) {
    sum += x;  // both < 2^63
    if (sum > kI63) {
      ovf = true;
      sum = 0;
    }
  }
};

// node u's position in prefix p's sorted announcer list (the last entry <= u;
// the prefix has announcers)
__device__ __forceinline__ uint32_t leaf_pos(const uint32_t* t_off, const uint32_t* t_nodes,
                                             uint32_t p, uint32_t u) {
  uint32_t lo = t_off[p], hi = t_off[p + 1];
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (t_nodes[mid] <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Under the policy a next hop k whose no-transit bit is set is a leaf of the
// entry (nothing transits k, so k is the destination) but need not select
// itself in its own entry: its leaf weight for p, read from the table. False
// when the rule does not apply to k.
__device__ __forceinline__ bool drained_leaf(const uint32_t* nt_bits, const uint32_t* t_off,
                                             const uint32_t* t_nodes, const int64_t* leaf_w,
                                             uint32_t k, uint32_t p, int64_t& w) {
  if (!((nt_bits[k >> 5] >> (k & 31u)) & 1u) || t_off[p] == t_off[p + 1]) return false;
  const uint32_t at = leaf_pos(t_off, t_nodes, p, k);
  if (t_nodes[at] != k) return false;
  w = leaf_w[at];
  return true;
}

// next hop `slot` (node k) of prefix p into acc
__device__ __forceinline__ void take_hop(const RoundArgs& a, uint32_t slot, uint32_t k, uint32_t p,
                                         Acc& acc) {
  const size_t i = (size_t)k * a.P + p;
  int64_t wk = 0;
  if (a.policy && drained_leaf(a.nt_bits, a.t_off, a.t_nodes, a.leaf_w, k, p, wk)) {
    if (wk <= 0) {  // never waited for; a zero leaf weight voids the entry
      acc.isvoid = true;
      return;
    }
  } else {
    const uint32_t tg = a.tag[i];
    if (tg == kPending || (tg & kRoundMask) >= a.round) {
      acc.wait = true;
      return;
    }
    const uint32_t st = tg >> 30;
    if (st == OSPF_UCMP_VOID) acc.isvoid = true;
    if (st == OSPF_UCMP_OVERFLOW) acc.ovf = true;
    if (st != OSPF_UCMP_OK) return;  // (NONE cannot be a selected next hop's)
    wk = a.W[i];
  }
  if (a.adj) {
    acc.add((uint64_t)a.S[slot]);
  } else {
    const uint64_t w = (uint64_t)wk, c = a.c[slot];
    const uint64_t lo = w * c;
    if (__umul64hi(w, c) || lo > kI63) acc.ovf = true;
    else acc.add(lo);
  }
}

__device__ __forceinline__ uint32_t status_of(const Acc& acc) {
  return acc.isvoid ? OSPF_UCMP_VOID : acc.ovf ? OSPF_UCMP_OVERFLOW : OSPF_UCMP_OK;
}

__global__ __launch_bounds__(256) void ucmp_round_kernel(const RoundArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const uint32_t P = a.P;
  for (uint32_t u = blockIdx.x; u < a.V; u += gridDim.x) {
    const uint32_t* __restrict__ m_ = a.data + a.off[u];
    const uint32_t* __restrict__ nh = m_ + a.hdr * (size_t)P;
    const uint32_t W = a.w[u];
    const uint32_t s0 = a.dn_off[u], ns = a.dn_off[u + 1] - s0;
    int64_t* Wu = a.W + (size_t)u * P;
    uint32_t* Tu = a.tag + (size_t)u * P;
    for (uint32_t base = wv * 64u; base < P; base += nwv * 64u) {
      const uint32_t p = base + lane;
      const bool in = p < P;
      bool todo = false;  // this lane's entry is pending on entry to the round
      if (a.round == 0) {
        if (in) {
          const uint32_t m = m_[p];
          uint32_t tg = kPending;
          int64_t w = 0;
          if (m == kInf) {
            tg = make_tag(OSPF_UCMP_NONE, 0);
          } else if (m == 0) {  // u announces: its position in the prefix's sorted list
            w = a.leaf_w[leaf_pos(a.t_off, a.t_nodes, p, u)];
            tg = make_tag(w > 0 ? OSPF_UCMP_OK : OSPF_UCMP_VOID, 0);
          }
          Wu[p] = w;
          Tu[p] = tg;
          todo = tg == kPending;
        }
      } else {
        todo = in && Tu[p] == kPending;
        if (W <= kSelLaneW) {
          if (todo) {
            Acc acc;
            const uint32_t* wd = nh + (size_t)p * W;
            for (uint32_t x = 0; x < W && !acc.wait; ++x)
              for (uint32_t bits = wd[x]; bits && !acc.wait; bits &= bits - 1u) {
                const uint32_t b = 32u * x + (uint32_t)__ffs((int)bits) - 1u;
                if (b < ns) take_hop(a, s0 + b, a.dn[s0 + b], p, acc);
              }
            if (!acc.wait) {
              const uint32_t st = status_of(acc);
              Wu[p] = st == OSPF_UCMP_OK ? (int64_t)acc.sum : 0;
              Tu[p] = make_tag(st, a.round);
              todo = false;
            }
          }
        } else {
          // a pending prefix at a time by the wave: a lane per next-hop word
          for (unsigned long long t = __ballot(todo); t; t &= t - 1ull) {
            const uint32_t j = (uint32_t)__ffsll((long long)t) - 1u;
            const uint32_t pj = base + j;
            const uint32_t* wd = nh + (size_t)pj * W;
            Acc acc;
            for (uint32_t x = lane; x < W && !acc.wait; x += 64)
              for (uint32_t bits = wd[x]; bits && !acc.wait; bits &= bits - 1u) {
                const uint32_t b = 32u * x + (uint32_t)__ffs((int)bits) - 1u;
                if (b < ns) take_hop(a, s0 + b, a.dn[s0 + b], pj, acc);
              }
            const bool wait = __ballot(acc.wait) != 0ull;
            if (wait) continue;  // wave-uniform
#pragma unroll
            for (int o = 32; o; o >>= 1) acc.add((uint64_t)__shfl_xor((unsigned long long)acc.sum, o));
            acc.isvoid = __ballot(acc.isvoid) != 0ull;
            acc.ovf = __ballot(acc.ovf) != 0ull;
            if (lane == j) {
              const uint32_t st = status_of(acc);
              Wu[pj] = st == OSPF_UCMP_OK ? (int64_t)acc.sum : 0;
              Tu[pj] = make_tag(st, a.round);
              todo = false;
            }
          }
        }
      }
      const unsigned long long left = __ballot(todo);
      if (left && lane == (uint32_t)__ffsll((long long)left) - 1u)
        atomicAdd(a.pending, (uint32_t)__popcll(left));
    }
  }
}

// ---------------------------------------------------------------- the view
struct ViewArgs {
  uint32_t n, P, fill;  // 0: count the weights of each entry; 1: write; 2: write, no weights
  uint32_t hdr, policy;  // as RoundArgs
  const uint32_t* nt_bits;
  const uint32_t* t_off;
  const uint32_t* t_nodes;
  const int64_t* leaf_w;
  const uint32_t* roots;
  const uint32_t* data;
  const uint64_t* off;
  const uint32_t* w;
  const uint32_t* dn_off;
  const uint32_t* dn;
  const int64_t* W;
  const uint32_t* tag;
  uint32_t* cnt;          // [n * P]      (fill 0)
  const uint64_t* o_off;  // [n * P + 1]  (fill 1)
  int64_t* o_adv;
  uint8_t* o_status;
  int64_t* o_wt;
};

__device__ __forceinline__ uint64_t gcd64(uint64_t x, uint64_t y) {
  while (y) {
    const uint64_t t = x % y;
    x = y;
    y = t;
  }
  return x;
}

// the weight next hop k of prefix p carries in a root's link view
__device__ __forceinline__ uint64_t hop_weight(const ViewArgs& a, uint32_t k, uint32_t p) {
  int64_t w;
  if (a.policy && drained_leaf(a.nt_bits, a.t_off, a.t_nodes, a.leaf_w, k, p, w)) return (uint64_t)w;
  return (uint64_t)a.W[(size_t)k * a.P + p];
}

// A thread per (root, prefix), lane = prefix: the entry's next-hop words twice
// (gcd, then the quotients), the gathers W[k][p] coalesced as in the rounds.
__global__ __launch_bounds__(256) void ucmp_view_kernel(const ViewArgs a) {
  const uint32_t P = a.P;
  for (uint32_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    const uint32_t r = a.roots[i];
    const uint32_t* nh = a.data + a.off[r] + a.hdr * (size_t)P;
    const uint32_t W = a.w[r];
    const uint32_t s0 = a.dn_off[r], ns = a.dn_off[r + 1] - s0;
    for (uint32_t p = threadIdx.x; p < P; p += blockDim.x) {
      const size_t e = (size_t)i * P + p;
      const uint32_t st = a.tag[(size_t)r * P + p] >> 30;
      const uint32_t* wd = nh + (size_t)p * W;
      if (!a.fill) {
        uint32_t k = 0;
        if (st == OSPF_UCMP_OK)
          for (uint32_t x = 0; x < W; ++x) {
            uint32_t bits = wd[x];
            if (32u * x + 32u > ns) bits &= ns > 32u * x ? (1u << (ns - 32u * x)) - 1u : 0u;
            k += (uint32_t)__popc(bits);
          }
        a.cnt[e] = k;
        continue;
      }
      a.o_adv[e] = a.W[(size_t)r * P + p];
      a.o_status[e] = (uint8_t)st;
      if (st != OSPF_UCMP_OK || a.fill == 2) continue;
      uint64_t g = 0;
      for (uint32_t x = 0; x < W; ++x)
        for (uint32_t bits = wd[x]; bits; bits &= bits - 1u) {
          const uint32_t b = 32u * x + (uint32_t)__ffs((int)bits) - 1u;
          if (b < ns) g = gcd64(g, hop_weight(a, a.dn[s0 + b], p));
        }
      int64_t* out = a.o_wt + a.o_off[e];
      for (uint32_t x = 0; x < W; ++x)
        for (uint32_t bits = wd[x]; bits; bits &= bits - 1u) {
          const uint32_t b = 32u * x + (uint32_t)__ffs((int)bits) - 1u;
          if (b >= ns) continue;
          const uint64_t w = hop_weight(a, a.dn[s0 + b], p);
          *out++ = (int64_t)(g > 1 ? w / g : w);
        }
    }
  }
}

}  // namespace

// ---------------------------------------------------------------- the result
struct ospf_ucmp {
  struct Res {
    int64_t* W = nullptr;
    uint32_t* tag = nullptr;
    size_t w_cells = 0, t_cells = 0;
  } r[2];
  int cur = 0;          // the committed result
  bool valid = false;
  uint64_t serial = 0;  // the selection (ospf_selstate::serial) it was resolved over
  uint32_t rounds = 0;
  // a run's inputs and scratch (kept between runs)
  uint32_t *c = nullptr, *minw = nullptr, *pending = nullptr;
  int64_t *S = nullptr, *leaf_w = nullptr;
  size_t c_cap = 0, minw_cap = 0, pending_cap = 0, s_cap = 0, lw_cap = 0;
};

namespace {

using namespace ospf_int;
using namespace ospf_int::selst;

void release_ucmp(ospf_selstate* st) {
  ospf_ucmp* u = st->ucmp;
  if (!u) return;
  for (auto& r : u->r) {
    (void)hipFree(r.W);
    (void)hipFree(r.tag);
  }
  (void)hipFree(u->c);
  (void)hipFree(u->minw);
  (void)hipFree(u->pending);
  (void)hipFree(u->S);
  (void)hipFree(u->leaf_w);
  delete u;
  st->ucmp = nullptr;
}

// a device buffer of one call, freed on return
struct Tmp {
  void* p = nullptr;
  ~Tmp() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

// what keeps the state from being resolved or viewed now (null: nothing)
const char* state_error(const ospf_selstate* st) {
  if (!st->primed) return "ucmp: the state is not primed";
  if (st->gen != st->c->graph_gen || st->c->mask.on)
    return "ucmp: the graph changed since the state's selection was stored (ospf_selstate_update)";
  if (st->c->info.n_nodes != st->V) return "ucmp: the graph has another node count";
  return nullptr;
}

uint32_t grid_for(uint32_t n) { return std::max(1u, std::min(n, 1u << 20)); }

}  // namespace

extern "C" {

int ospf_selstate_ucmp(ospf_selstate* st, uint32_t algo, const int64_t* leaf_weight,
                       const int64_t* link_weight_sum, uint32_t n_slots, uint32_t* rounds) {
  if (!st || !st->c) return OSPF_E_INVAL;
  ospf_ctx* c = st->c;
  if (rounds) *rounds = 0;
  if (injected(c)) return stfail(st, OSPF_E_DEVICE, c->err);
  if (const char* bad = state_error(st)) return stfail(st, OSPF_E_INVAL, bad);
  if (algo != OSPF_UCMP_ADJ && algo != OSPF_UCMP_PREFIX)
    return stfail(st, OSPF_E_INVAL, "ucmp: algo is neither OSPF_UCMP_ADJ nor OSPF_UCMP_PREFIX");
  const bool adj = algo == OSPF_UCMP_ADJ;
  const uint32_t V = st->V, P = st->P;
  const size_t nnz = st->t_nodes.size(), slots = c->h_dn.size();
  if (nnz && !leaf_weight) return stfail(st, OSPF_E_INVAL, "ucmp: no leaf weights");
  if (adj && !link_weight_sum)
    return stfail(st, OSPF_E_INVAL, "ucmp: adjacency-weight propagation needs the link weight sums");
  if (link_weight_sum && n_slots != slots)
    return stfail(st, OSPF_E_INVAL, "ucmp: " + std::to_string(n_slots) + " link weight sums for " +
                                        std::to_string(slots) + " distinct-neighbour slots");
  for (size_t i = 0; i < nnz; ++i)
    if (leaf_weight[i] < 0) return stfail(st, OSPF_E_INVAL, "ucmp: a negative leaf weight");
  if (adj)
    for (size_t i = 0; i < slots; ++i)
      if (link_weight_sum[i] < 0) return stfail(st, OSPF_E_INVAL, "ucmp: a negative link weight sum");
  if (!st->ucmp) {
    st->ucmp = new (std::nothrow) ospf_ucmp();
    if (!st->ucmp) return stfail(st, OSPF_E_NOMEM, "ucmp: out of host memory");
    st->release_ucmp = release_ucmp;
  }
  ospf_ucmp* u = st->ucmp;
  ospf_ucmp::Res& nr = u->r[u->cur ^ 1];  // the shadow result: committed at the end
  const ospf_selstate::Buf& b = st->b[st->cur];
  const size_t cells = (size_t)V * P;
  STCHK(st, hipSetDevice(c->device));
  int rc;
  if ((rc = grow(st, &nr.W, &nr.w_cells, cells))) return rc;
  if ((rc = grow(st, &nr.tag, &nr.t_cells, cells))) return rc;
  if ((rc = grow(st, &u->pending, &u->pending_cap, 1))) return rc;
  if ((rc = grow(st, &u->leaf_w, &u->lw_cap, nnz))) return rc;
  if (nnz) STCHK(st, hipMemcpy(u->leaf_w, leaf_weight, nnz * 8, hipMemcpyHostToDevice));
  if (adj) {
    if ((rc = grow(st, &u->S, &u->s_cap, slots))) return rc;
    if (slots) STCHK(st, hipMemcpy(u->S, link_weight_sum, slots * 8, hipMemcpyHostToDevice));
  } else {
    if ((rc = grow(st, &u->c, &u->c_cap, slots))) return rc;
    if ((rc = grow(st, &u->minw, &u->minw_cap, slots))) return rc;
  }
  if (!cells) {  // no entry: an empty result
    u->cur ^= 1;
    u->valid = true;
    u->serial = st->serial;
    u->rounds = 0;
    return OSPF_OK;
  }
  if (!adj && slots) {
    STCHK(st, hipMemset(u->c, 0, slots * 4));
    STCHK(st, hipMemset(u->minw, 0xFF, slots * 4));
    LinkArgs la{c->g, st->hop ? 1u : 0u, u->minw, u->c};
    hipLaunchKernelGGL(ucmp_links_kernel, dim3(grid_for(V)), dim3(256), 0, nullptr, la);
    STCHK(st, hipGetLastError());
  }
  RoundArgs a{};
  a.V = V;
  a.P = P;
  a.adj = adj ? 1u : 0u;
  a.hdr = st->hdr;
  a.policy = st->policy ? 1u : 0u;
  a.nt_bits = c->g.nt_bits;
  a.data = b.data;
  a.off = b.off;
  a.w = b.w;
  a.dn_off = b.dn_off;
  a.dn = b.dn;
  a.t_off = st->d_tab;
  a.t_nodes = st->d_tab + P + 1;
  a.leaf_w = u->leaf_w;
  a.c = u->c;
  a.S = u->S;
  a.W = nr.W;
  a.tag = nr.tag;
  a.pending = u->pending;
  const uint32_t waves = std::min(4u, (P + 63u) / 64u);
  uint32_t left = 0, last = 0xFFFFFFFFu, done = 0;
  for (uint32_t round = 0;; ++round) {
    if (round > kRoundMask) return stfail(st, OSPF_E_RANGE, "ucmp: more rounds than a tag holds");
    a.round = round;
    STCHK(st, hipMemset(u->pending, 0, 4));
    hipLaunchKernelGGL(ucmp_round_kernel, dim3(grid_for(V)), dim3(64u * waves), 0, nullptr, a);
    STCHK(st, hipGetLastError());
    STCHK(st, hipMemcpy(&left, u->pending, 4, hipMemcpyDeviceToHost));
    if (round && left < last) done = round;
    if (!left) break;
    // every round settles the entries whose next hops were settled before it:
    // a round that settles nothing means next hops that never settle -- a
    // selection that is not the graph's
    if (round && left == last)
      return stfail(st, OSPF_E_DEVICE, "ucmp: " + std::to_string(left) +
                                           " entries wait for next hops that never settle");
    last = left;
  }
  u->cur ^= 1;
  u->valid = true;
  u->serial = st->serial;
  u->rounds = done;
  if (rounds) *rounds = done;
  return OSPF_OK;
}

int ospf_selstate_ucmp_copy(ospf_selstate* st, const uint32_t* roots, uint32_t n,
                            int64_t* advertised, uint8_t* status, uint64_t* off, int64_t* wt,
                            uint64_t cap, uint64_t* n_wt) {
  if (!st || !st->c || (n && !roots) || !n_wt) return OSPF_E_INVAL;
  ospf_ctx* c = st->c;
  *n_wt = 0;
  if (injected(c)) return stfail(st, OSPF_E_DEVICE, c->err);
  if (const char* bad = state_error(st)) return stfail(st, OSPF_E_INVAL, bad);
  const ospf_ucmp* u = st->ucmp;
  if (!u || !u->valid) return stfail(st, OSPF_E_INVAL, "ucmp: copy before a run (ospf_selstate_ucmp)");
  if (u->serial != st->serial)
    return stfail(st, OSPF_E_INVAL, "ucmp: the selection changed since the weights were resolved");
  const size_t P = st->P, cells = (size_t)n * P;
  for (uint32_t i = 0; i < n; ++i)
    if (roots[i] >= st->V) return stfail(st, OSPF_E_INVAL, "ucmp: root id outside the graph");
  if (cells && (!advertised || !status))
    return stfail(st, OSPF_E_INVAL, "ucmp: advertised and status are required");
  const bool links = off != nullptr;  // without off: the advertised weights and statuses only
  if (!cells) {
    if (off) off[0] = 0;
    return OSPF_OK;
  }
  const ospf_selstate::Buf& b = st->b[st->cur];
  const ospf_ucmp::Res& res = u->r[u->cur];
  STCHK(st, hipSetDevice(c->device));
  Tmp d_roots, d_cnt, d_off, d_adv, d_st, d_wt;
  auto want = [&](Tmp& t, size_t bytes) { return dev_malloc(c, &t.p, std::max<size_t>(bytes, 8)) == hipSuccess; };
  const size_t lcells = links ? cells : 0;  // the counts and offsets are the link view's
  if (!want(d_roots, (size_t)n * 4) || !want(d_cnt, lcells * 4) || !want(d_off, (lcells + 1) * 8) ||
      !want(d_adv, cells * 8) || !want(d_st, cells))
    return stfail(st, OSPF_E_NOMEM, "ucmp: hipMalloc of the view's buffers");
  STCHK(st, hipMemcpy(d_roots.p, roots, (size_t)n * 4, hipMemcpyHostToDevice));
  ViewArgs a{};
  a.n = n;
  a.P = (uint32_t)P;
  a.hdr = st->hdr;
  a.policy = st->policy ? 1u : 0u;
  a.nt_bits = c->g.nt_bits;
  a.t_off = st->d_tab;
  a.t_nodes = st->d_tab + P + 1;
  a.leaf_w = u->leaf_w;
  a.roots = d_roots.as<uint32_t>();
  a.data = b.data;
  a.off = b.off;
  a.w = b.w;
  a.dn_off = b.dn_off;
  a.dn = b.dn;
  a.W = res.W;
  a.tag = res.tag;
  a.cnt = d_cnt.as<uint32_t>();
  const uint32_t threads = (uint32_t)std::min<size_t>(256, (P + 63) / 64 * 64);
  std::vector<uint64_t> h_off(lcells + 1, 0);
  if (links) {
    hipLaunchKernelGGL(ucmp_view_kernel, dim3(grid_for(n)), dim3(threads), 0, nullptr, a);
    STCHK(st, hipGetLastError());
    std::vector<uint32_t> cnt(cells);
    STCHK(st, hipMemcpy(cnt.data(), d_cnt.p, cells * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cells; ++i) h_off[i + 1] = h_off[i] + cnt[i];
  }
  const uint64_t total = h_off[lcells];
  *n_wt = total;
  if (total > cap || (total && !wt))
    return stfail(st, OSPF_E_RANGE, "ucmp: " + std::to_string(total) +
                                        " next-hop weights: above the caller's capacity");
  if (!want(d_wt, total * 8)) return stfail(st, OSPF_E_NOMEM, "ucmp: hipMalloc of the weights");
  STCHK(st, hipMemcpy(d_off.p, h_off.data(), (lcells + 1) * 8, hipMemcpyHostToDevice));
  a.fill = links ? 1 : 2;
  a.o_off = d_off.as<uint64_t>();
  a.o_adv = d_adv.as<int64_t>();
  a.o_status = d_st.as<uint8_t>();
  a.o_wt = d_wt.as<int64_t>();
  hipLaunchKernelGGL(ucmp_view_kernel, dim3(grid_for(n)), dim3(threads), 0, nullptr, a);
  STCHK(st, hipGetLastError());
  // into buffers of this call first: a failed copy leaves the caller's as they were
  std::vector<int64_t> h_adv(cells), h_wt(total);
  std::vector<uint8_t> h_st(cells);
  STCHK(st, hipMemcpy(h_adv.data(), d_adv.p, cells * 8, hipMemcpyDeviceToHost));
  STCHK(st, hipMemcpy(h_st.data(), d_st.p, cells, hipMemcpyDeviceToHost));
  if (total) STCHK(st, hipMemcpy(h_wt.data(), d_wt.p, total * 8, hipMemcpyDeviceToHost));
  std::copy(h_adv.begin(), h_adv.end(), advertised);
  std::copy(h_st.begin(), h_st.end(), status);
  if (links) std::copy(h_off.begin(), h_off.end(), off);
  if (total) std::copy(h_wt.begin(), h_wt.end(), wt);
  return OSPF_OK;
}

int ospf_selstate_ucmp_info(const ospf_selstate* st, uint32_t* rounds, uint32_t* n_slots) {
  if (!st || !st->c) return OSPF_E_INVAL;
  if (rounds) *rounds = st->ucmp && st->ucmp->valid ? st->ucmp->rounds : 0;
  if (n_slots) *n_slots = (uint32_t)st->c->h_dn.size();
  return OSPF_OK;
}

}  // extern "C"
