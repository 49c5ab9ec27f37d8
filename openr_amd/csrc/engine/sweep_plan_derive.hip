// sweep_plan_derive.hip — the DERIVE planner of a sweep (sweep_impl.h): unit
// metric / hop count, the headline fabric path. Host code only: leaf groups,
// twin classes, the wide next-hop plan, then plan_derive's stages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "sweep_impl.h"

using namespace ospf_int;
using namespace ospf_int::sweep;

namespace {

// stable sort on host threads: chunks stable-sorted in parallel, then merged
// pairwise (left run first: stable)

template <class T, class Less>
void par_stable_sort(std::vector<T>& v, Less less) {
  const uint32_t n = (uint32_t)v.size();
  const uint32_t hw = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  uint32_t C = 1;
  while (C * 2 <= hw && n / (C * 2) >= 4096u) C *= 2;
  if (C == 1) {
    std::stable_sort(v.begin(), v.end(), less);
    return;
  }
  std::vector<uint32_t> b(C + 1);
  for (uint32_t k = 0; k <= C; ++k) b[k] = (uint32_t)((uint64_t)n * k / C);
  par_for(C, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t k = lo; k < hi; ++k) std::stable_sort(v.begin() + b[k], v.begin() + b[k + 1], less);
  }, 1);
  std::vector<T> tmp(n);
  for (uint32_t w = 1; w < C; w *= 2) {
    const uint32_t pairs = C / (2 * w);
    par_for(pairs, [&](uint32_t lo, uint32_t hi) {
      for (uint32_t q = lo; q < hi; ++q) {
        const uint32_t a0 = b[2 * q * w], a1 = b[2 * q * w + w], a2 = b[2 * q * w + 2 * w];
        std::merge(v.begin() + a0, v.begin() + a1, v.begin() + a1, v.begin() + a2, tmp.begin() + a0, less);
      }
    }, 1);
    v.swap(tmp);
  }
}

// OSPF_SWEEP_TIMING: sub-phases of a plan phase on stderr
struct SubLaps {
  const char* phase;
  bool on = knob_flag(Knob::OSPF_SWEEP_TIMING);
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  explicit SubLaps(const char* p) : phase(p) {}
  void operator()(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "sweep_create plan/%s/%s %.2f ms\n", phase, what,
            std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};
// ---------------------------------------------------------------- plans
// Usable-slot signature of a leaf root (bit k: an up link to its k-th
// distinct neighbour), from the context's padded host shadows.
uint32_t usable_slots(const ospf_ctx* c, uint32_t r) {
  uint32_t use = 0;
  const uint32_t* dn = c->h_dn.data() + c->h_dn_off[r];
  const uint32_t K = c->h_dn_off[r + 1] - c->h_dn_off[r];
  for (uint32_t e = c->h_prow[r]; e < c->h_prow[r + 1]; ++e) {
    const uint32_t cx = c->h_pcolx[e];
    if ((cx & 0x80000000u) || cx == r) continue;
    const uint32_t k = (uint32_t)(std::lower_bound(dn, dn + K, cx) - dn);
    if (k < 32u) use |= 1u << k;
  }
  return use;
}

// Leaf roots ordered so that roots with the same slot table (distinct
// neighbours + usable links: the racks of a pod) are adjacent, cut into
// groups of <= kLeafMaxG; returns the group offsets.
std::vector<uint32_t> leaf_groups(const ospf_ctx* c, const Facts& f, std::vector<uint32_t>& roots) {
  SubLaps lap("leaf groups");
  std::vector<uint32_t> use(roots.size());
  par_for((uint32_t)roots.size(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo; i < hi; ++i) use[i] = usable_slots(c, roots[i]);
  });
  std::vector<uint32_t> ord(roots.size());
  std::iota(ord.begin(), ord.end(), 0u);
  auto same_nbrs = [&](uint32_t a, uint32_t b) { return f.same_nbrs(a, b); };
  par_stable_sort(ord, [&](uint32_t x, uint32_t y) {
    const uint32_t a = roots[x], b = roots[y];
    if (f.nbrs(a) != f.nbrs(b)) return f.first(a) != f.first(b) ? f.first(a) < f.first(b)
                                                                 : f.nbrs(a) < f.nbrs(b);
    const int cmp = std::lexicographical_compare(
                        f.dn->begin() + (*f.dn_off)[a], f.dn->begin() + (*f.dn_off)[a + 1],
                        f.dn->begin() + (*f.dn_off)[b], f.dn->begin() + (*f.dn_off)[b + 1])
                        ? -1
                        : (same_nbrs(a, b) ? 0 : 1);
    if (cmp) return cmp < 0;
    return use[x] < use[y];
  });
  lap("sort");
  std::vector<uint32_t> out(roots.size()), uo(roots.size());
  for (size_t i = 0; i < ord.size(); ++i) {
    out[i] = roots[ord[i]];
    uo[i] = use[ord[i]];
  }
  roots.swap(out);
  std::vector<uint32_t> grp{0u};
  for (uint32_t i = 1; i <= roots.size(); ++i) {
    const uint32_t g0 = grp.back();
    if (i == roots.size() || i - g0 >= ospf::kLeafMaxG || uo[i] != uo[g0] ||
        !same_nbrs(roots[i], roots[g0]))
      grp.push_back(i);
  }
  return grp;
}

// Twin classes (spf_twin.hip): nodes with the same usable distinct
// neighbours and the same transit bit. cls[v] = class id, rep / sec = the
// smallest two members of each class (sec = kNone for a class of one).
struct Twins {
  std::vector<uint32_t> cls, rep, sec;
};
Twins twin_classes(const ospf_ctx* c) {
  SubLaps lap("twin classes");
  const uint32_t V = c->info.n_nodes;
  std::vector<uint32_t> off(V + 1, 0);
  std::vector<uint64_t> key(V);
  // each node's usable distinct neighbours (sorted, unique): counted, then
  // written and hashed, both on host threads
  auto nbrs_of = [&](uint32_t u, uint32_t* out) {  // -> count (out may be null)
    uint32_t m = 0, prev = 0xFFFFFFFFu;
    bool sorted = true;
    for (uint32_t e = c->h_prow[u]; e < c->h_prow[u + 1]; ++e) {
      const uint32_t x = c->h_pcolx[e];
      if ((x & 0x80000000u) || x == u || x == prev) continue;
      sorted &= prev == 0xFFFFFFFFu || x > prev;
      if (out) out[m] = x;
      prev = x;
      ++m;
    }
    if (out && !sorted) {  // (rows are sorted by neighbour id; kept exact either way)
      std::sort(out, out + m);
      m = (uint32_t)(std::unique(out, out + m) - out);
    }
    return m;
  };
  std::vector<uint32_t> cnt(V);
  ospf_int::par_for_rows(V, c->h_prow.data(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t u = lo; u < hi; ++u) cnt[u] = nbrs_of(u, nullptr);
  });
  for (uint32_t u = 0; u < V; ++u) off[u + 1] = off[u] + cnt[u];
  // (uninitialized: every slot is written below; a zero fill of ~10 MB of
  // fresh pages cost more than the pass)
  std::unique_ptr<uint32_t[]> lst_buf(new uint32_t[std::max<uint32_t>(off[V], 1)]);
  uint32_t* const lst = lst_buf.get();
  ospf_int::par_for_rows(V, c->h_prow.data(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t u = lo; u < hi; ++u) {
      const uint32_t m = nbrs_of(u, lst + off[u]);
      for (uint32_t i = m; i < cnt[u]; ++i) lst[off[u] + i] = 0xFFFFFFFFu;  // (dups of an unsorted row)
      cnt[u] = m;
      const bool tr = !((c->h_nt[u >> 5] >> (u & 31)) & 1u);
      // (independent mixes, summed: no dependent chain through a spine's row;
      // a hash only -- classes are split by exact equality below)
      uint64_t h = tr ? 0x9E3779B97F4A7C15ull : 0xC2B2AE3D27D4EB4Full;
      for (uint32_t i = 0; i < m; ++i) h += ospf::digest_mix(lst[off[u] + i] ^ (i * 0x9E3779B97F4A7C15ull));
      key[u] = h;
    }
  });
  lap("lists + keys");
  auto same = [&](uint32_t a, uint32_t b) {
    const bool ta = !((c->h_nt[a >> 5] >> (a & 31)) & 1u), tb = !((c->h_nt[b >> 5] >> (b & 31)) & 1u);
    return ta == tb && cnt[a] == cnt[b] &&
           std::equal(lst + off[a], lst + off[a] + cnt[a], lst + off[b]);
  };
  // nodes by (key, id): the stable order by key
  std::vector<std::pair<uint64_t, uint32_t>> kv(V);
  for (uint32_t u = 0; u < V; ++u) kv[u] = {key[u], u};
  par_stable_sort(kv, [](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) {
    return x < y;
  });
  std::vector<uint32_t> ord(V);
  for (uint32_t u = 0; u < V; ++u) ord[u] = kv[u].second;
  lap("key sort");
  Twins t;
  t.cls.assign(V, kNone);
  for (size_t i = 0; i < V;) {
    size_t j = i;
    while (j < V && key[ord[j]] == key[ord[i]]) ++j;
    // within a hash run, split by exact equality (collisions are rare)
    for (size_t p = i; p < j; ++p) {
      const uint32_t u = ord[p];
      if (t.cls[u] != kNone) continue;
      const uint32_t id = (uint32_t)t.rep.size();
      t.rep.push_back(u);
      t.sec.push_back(kNone);
      t.cls[u] = id;
      for (size_t q = p + 1; q < j; ++q) {
        const uint32_t w = ord[q];
        if (t.cls[w] != kNone || !same(u, w)) continue;
        t.cls[w] = id;
      }
    }
    i = j;
  }
  lap("classes");
  // representative = smallest member, second = the next one
  for (uint32_t u = 0; u < V; ++u) {
    const uint32_t id = t.cls[u];
    if (u < t.rep[id]) {
      t.sec[id] = t.rep[id];
      t.rep[id] = u;
    } else if (u != t.rep[id] && (t.sec[id] == kNone || u < t.sec[id])) {
      t.sec[id] = u;
    }
  }
  return t;
}

// Host plan of the wide next-hop kernel (nh_wide_plan_kernel) for a class
// of roots (in order): runs of <= kWideG roots with the same distinct
// neighbours, each run's slot table over level-row positions, each root's
// usable-slot words.
struct WideHost {
  std::vector<uint32_t> run, soff, slots, keep, own;
};
int wide_plan_build(ospf_ctx* c, const Facts& f, const std::vector<uint32_t>& roots, uint32_t W,
                    const std::vector<uint32_t>& pos, WideHost& h) {
  const uint32_t n = (uint32_t)roots.size();
  h = WideHost{};
  h.keep.assign((size_t)n * W, 0u);
  auto same = [&](uint32_t a, uint32_t b) { return f.same_nbrs(a, b); };
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i];
    if (pos[r] == kNone) return fail(c, OSPF_E_RANGE, "wide plan: a root without a level row");
    if (f.nbrs(r) > 32u * W || f.nbrs(r) > 2048u) return fail(c, OSPF_E_RANGE, "wide plan: too many neighbours");
    h.own.push_back(pos[r]);
  }
  // each root's usable slots, on host threads (rows ascend by neighbour id:
  // a cursor over the distinct neighbours, a search only if one is missed)
  par_for(n, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t r = roots[i];
      const uint32_t* dn = f.dn->data() + (*f.dn_off)[r];
      const uint32_t K = f.nbrs(r);
      uint32_t k = 0;
      for (uint32_t e = c->h_prow[r]; e < c->h_prow[r + 1]; ++e) {
        const uint32_t x = c->h_pcolx[e];
        if ((x & 0x80000000u) || x == r) continue;
        while (k < K && dn[k] < x) ++k;
        if (k >= K || dn[k] != x) k = (uint32_t)(std::lower_bound(dn, dn + K, x) - dn);
        h.keep[(size_t)i * W + (k >> 5)] |= 1u << (k & 31u);
      }
    }
  }, 16);
  for (uint32_t i = 0; i < n; ++i)
    if (i == 0 || i - h.run.back() >= 64u || !same(roots[h.run.back()], roots[i])) h.run.push_back(i);
  h.run.push_back(n);
  h.soff.push_back(0u);
  for (size_t q = 0; q + 1 < h.run.size(); ++q) {
    const uint32_t r0 = roots[h.run[q]], K = f.nbrs(r0);
    const uint32_t* dn = f.dn->data() + (*f.dn_off)[r0];
    for (uint32_t k = 0; k < K; ++k) {
      bool used = false;
      for (uint32_t i = h.run[q]; i < h.run[q + 1] && !used; ++i)
        used = (h.keep[(size_t)i * W + (k >> 5)] >> (k & 31u)) & 1u;
      uint32_t v = kNone;
      if (used) {
        const uint32_t x = dn[k];
        if ((c->h_nt[x >> 5] >> (x & 31)) & 1u) {
          v = 0x80000000u | x;
        } else {
          v = pos[x];
          if (v == kNone) return fail(c, OSPF_E_RANGE, "wide plan: a neighbour without a level row");
        }
      }
      h.slots.push_back(v);
    }
    h.soff.push_back((uint32_t)h.slots.size());
  }
  return OSPF_OK;
}
// DERIVE (spf_levels.hip, spf_twin.hip, spf_leaf.hip, spf_msbfs.hip derive
// kernels), unit metric / hop count. The part's roots split into leaves (an
// independent set of nodes with <= 32 distinct neighbours: a fabric's racks)
// and the cover.
// (A) levels: the distance-only 128-root BFS for the seed rows -- the cover
//     rows the part needs (its cover roots, their neighbours, the leaves'
//     neighbours) that no twin class derives, plus the leaf representatives
//     of the classes the derived rows and the twin next-hop launches read --
//     ordered by each node's smallest neighbour so a traversal shares frontiers;
// (A') twin levels: the other cover rows from the representative rows of
//     their neighbours' twin classes (ospf_twin_levels_dev: a fabric switch
//     from one rack row of its pod and one spine row of its plane), no
//     traversal; without twins every cover row is a BFS row and the leaf
//     representatives come first in (B) instead;
// (B) the leaves' level, dist and next-hop rows from their neighbours' level
//     rows (next-hop rows only for BFS'd representatives), groups of leaves
//     with one slot table reading each tile once;
// (C) one next-hop launch per width class of cover roots, roots ordered by
//     their largest neighbour (their neighbours' level rows stay in L2 / MALL),
//     on their own streams beside (B).
// OSPF_SWEEP_TIMING: host phases of a plan on stderr
struct PlanLaps {
  bool on = knob_flag(Knob::OSPF_SWEEP_TIMING);
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "sweep_create plan/%s %.2f ms\n", what,
            std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// a width class of cover roots (next-hop words W), roots by largest neighbour
struct Cls {
  uint32_t cap, W;
  std::vector<uint32_t> roots;
  bool twin = false, reads_leaf = false;
};

// The device side of the plan: what the units' launches read. A unit's fn
// takes a copy of this, never the DerivePlan.
struct DeriveDev {
  uint32_t V = 0, hop = 0;
  uint32_t DP = 0, pitch = 0;  // pitch of dist / leaf next-hop rows (words), of level rows (bytes)
  uint32_t *d_clo = nullptr, *d_pos = nullptr, *dist = nullptr, *d_l = nullptr, *lnh = nullptr;
  uint32_t *d_grp_r = nullptr, *d_grp = nullptr, *d_lout = nullptr;
  uint32_t *d_tcls = nullptr, *d_trep = nullptr, *d_tsec = nullptr;
  uint8_t* lev = nullptr;
  ospf_digest* ldg = nullptr;
};

// Host state of plan_derive, shared by its stages (in the order they fill
// it). Not copyable: a unit's fn that named it would not compile.
struct DerivePlan {
  ospf_sweep* const s;
  ospf_ctx* const c;
  const Facts& f;
  const std::vector<uint32_t>& mine;
  const uint32_t V;
  PlanLaps lap;
  DerivePlan(ospf_sweep* sw, const Facts& facts, const std::vector<uint32_t>& part)
      : s(sw), c(sw->c), f(facts), mine(part), V(sw->V) {}
  DerivePlan(const DerivePlan&) = delete;
  // leaf set and closure
  std::vector<uint8_t> leaf, in_l;             // a leaf; an owned leaf
  std::vector<uint32_t> own_l, own_c, nb_c, extra_l;  // extra_l: leaves the cover next hops read
  // width and twin classes
  std::vector<Cls> cls;
  Twins tw;
  std::vector<uint32_t> ccls, ccnt, cs;        // classes_of: every node's, the last asked
  bool all_leaf_rows = false;                  // a class reads every neighbour's row (not twins)
  // cover rows and the twin-levels set
  std::vector<uint32_t> need_l;
  std::vector<uint8_t> in_a, in_d, seed;       // a cover row; derived by twin levels; a BFS'd leaf
  uint32_t n_cover = 0;
  bool twin_lv = false;
  // rows and stages
  std::vector<uint32_t> reps, rest, grp_r, grp, clo, drv, pos, dgo, sg, lsg;
  std::vector<int> stage_of;                   // stage of a node's derived row
  uint32_t nR = 0, nL = 0, nc = 0, nd = 0, n_dgrp = 0, S = 0, rows = 0;
  // allocations, events, the running digest slot
  DeriveDev dev;
  bool drop_rest = false;
  int ev_a = -1, ev_t = -1, ev_r = -1, ev_b = -1, ev_cov = -1;
  std::vector<int> ev_s;                       // stage k of the derived rows done (the last = ev_t)
  uint32_t slot = 0;
  std::vector<Unit> side, after;               // cover next-hop units before / after the leaves

  // classes of r's usable transit neighbours (sorted, unique) into cs; false
  // past kTwinMaxC
  static constexpr uint32_t kCS = ospf::kTwinMaxC + 1;
  bool classes_of(uint32_t r) {
    cs.assign(ccls.begin() + (size_t)r * kCS, ccls.begin() + (size_t)r * kCS + ccnt[r]);
    return cs.size() <= ospf::kTwinMaxC;
  }
  // latest stage r's rows need (0 if none)
  int dep_of(uint32_t r, bool self) const {
    int d = self ? stage_of[r] : -1;
    for (uint32_t q = (*f.dn_off)[r]; q < (*f.dn_off)[r + 1]; ++q) d = std::max(d, stage_of[(*f.dn)[q]]);
    return std::max(d, 0);
  }
};

void derive_leaf_closure(DerivePlan& d) {
  if (!knob_flag(Knob::OSPF_SWEEP_NOLEAF)) d.leaf = leaf_set(d.f);
  else d.leaf.assign(d.V, 0);
  d.lap("leaf set");
  for (uint32_t r : d.mine) (d.leaf[r] ? d.own_l : d.own_c).push_back(r);
  // leaves whose rows the cover roots' next hops read
  d.nb_c = closure(d.f, d.own_c);
  d.in_l.assign(d.V, 0);
  for (uint32_t r : d.own_l) d.in_l[r] = 1;
  for (uint32_t v : d.nb_c)
    if (d.leaf[v] && !d.in_l[v]) d.extra_l.push_back(v);
  d.lap("closure");
}

void derive_classes(DerivePlan& d) {
  const Facts& f = d.f;
  ospf_ctx* c = d.c;
  const uint32_t V = d.V;
  // cover classes by capacity, roots by largest neighbour
  for (uint32_t cap : classes_by(d.own_c, [&](uint32_t r) { return f.cap(r); })) {
    Cls k{cap, cap > 16 ? cap / 32 : 1u, {}};
    for (uint32_t r : d.own_c)
      if (f.cap(r) == cap) k.roots.push_back(r);
    locality_order(k.roots, [&](uint32_t v) { return f.last(v); });
    for (uint32_t r : k.roots)
      for (uint32_t q = (*f.dn_off)[r]; q < (*f.dn_off)[r + 1] && !k.reads_leaf; ++q)
        k.reads_leaf = d.leaf[(*f.dn)[q]] != 0;
    d.cls.push_back(std::move(k));
  }
  // twin classes: a class of <= 4-word roots whose usable transit
  // neighbours span few classes reads one row per class (spf_twin.hip), and
  // so can a cover row (twin levels)
  d.lap("width classes");
  if (!knob_flag(Knob::OSPF_SWEEP_NOTWIN)) d.tw = twin_classes(c);
  d.lap("twin classes");
  // classes of r's usable transit neighbours: every node's, once, on host
  // threads: [V][kTwinMaxC + 1] slots and a count (kTwinMaxC + 1: more)
  constexpr uint32_t kCS = DerivePlan::kCS;
  const Twins& tw = d.tw;
  if (!tw.cls.empty()) {
    d.ccls.resize((size_t)V * kCS);
    d.ccnt.resize(V);
    ospf_int::par_for_rows(V, c->h_prow.data(), [&](uint32_t lo, uint32_t hi) {
      std::vector<uint32_t> b;
      for (uint32_t r = lo; r < hi; ++r) {
        // distinct classes, sorted; stops at kCS of them (more is "too many")
        b.clear();
        for (uint32_t e = c->h_prow[r]; e < c->h_prow[r + 1] && b.size() < kCS; ++e) {
          const uint32_t x = c->h_pcolx[e];
          if ((x & 0x80000000u) || x == r || ((c->h_nt[x >> 5] >> (x & 31)) & 1u)) continue;
          const uint32_t k = tw.cls[x];
          const auto it = std::lower_bound(b.begin(), b.end(), k);
          if (it == b.end() || *it != k) b.insert(it, k);
        }
        const uint32_t m = std::min<uint32_t>((uint32_t)b.size(), kCS);
        std::copy(b.begin(), b.begin() + m, d.ccls.begin() + (size_t)r * kCS);
        d.ccnt[r] = m;
      }
    });
  }
  auto twin_ok = [&](const std::vector<uint32_t>& roots) {
    uint64_t slots = 0, classes = 0;
    for (uint32_t r : roots) {
      if (!d.classes_of(r)) return false;
      slots += f.nbrs(r);
      classes += d.cs.size();
    }
    // worth it when a class covers several slots (OSPF_SWEEP_TWIN=1: always)
    return knob_flag(Knob::OSPF_SWEEP_TWIN) || slots >= 3 * std::max<uint64_t>(1, classes);
  };
  for (auto& k : d.cls) {
    k.twin = k.W <= 4 && !tw.cls.empty() && twin_ok(k.roots);
    if (k.reads_leaf && !k.twin) d.all_leaf_rows = true;
  }
  d.all_leaf_rows |= tw.cls.empty() || knob_flag(Knob::OSPF_SWEEP_ALL_LEAF_ROWS);
  d.lap("twin width classes");
}

void derive_cover_rows(DerivePlan& d) {
  const Facts& f = d.f;
  const Twins& tw = d.tw;
  const uint32_t V = d.V;
  d.need_l = d.own_l;
  d.need_l.insert(d.need_l.end(), d.extra_l.begin(), d.extra_l.end());
  // cover rows: own cover roots + every non-leaf neighbour of a needed root
  std::vector<uint8_t>& in_a = d.in_a;
  in_a.assign(V, 0);
  for (uint32_t v : d.own_c) in_a[v] = 1;
  for (uint32_t v : closure(f, d.need_l))
    if (!d.leaf[v]) in_a[v] = 1;
  for (uint32_t v : d.nb_c)
    if (!d.leaf[v]) in_a[v] = 1;
  for (uint32_t v = 0; v < V; ++v) d.n_cover += in_a[v];
  // (A') cover rows derived from twin classes; their classes' representatives
  // are BFS rows (a derived representative leaves the set: repeat until
  // stable), and so are the leaf representatives the twin next hops read
  std::vector<uint8_t>&in_d = d.in_d, &seed = d.seed;
  in_d.assign(V, 0);
  seed.assign(V, 0);
  d.twin_lv = !tw.cls.empty() && !knob_flag(Knob::OSPF_SWEEP_NOTWINLV);
  if (d.twin_lv) {
    for (uint32_t v = 0; v < V; ++v)
      if (in_a[v] && f.nbrs(v) <= 128 && d.classes_of(v)) in_d[v] = 1;
    for (bool changed = true; changed;) {
      changed = false;
      for (uint32_t v = 0; v < V; ++v) {
        if (!in_d[v]) continue;
        d.classes_of(v);
        for (uint32_t k : d.cs)
          if (in_d[tw.rep[k]]) {
            in_d[tw.rep[k]] = 0;
            changed = true;
          }
      }
    }
    auto seed_reps = [&](uint32_t v) {
      d.classes_of(v);
      for (uint32_t k : d.cs)
        if (d.leaf[tw.rep[k]]) seed[tw.rep[k]] = 1;
    };
    for (uint32_t v = 0; v < V; ++v)
      if (in_d[v]) seed_reps(v);
    for (auto& k : d.cls)
      if (k.twin)
        for (uint32_t r : k.roots) seed_reps(r);
    uint32_t nbfs = 0;
    for (uint32_t v = 0; v < V; ++v) nbfs += (in_a[v] && !in_d[v]) || seed[v];
    // worth it when the traversal shrinks to half (OSPF_SWEEP_TWINLV=1: always)
    if (!knob_flag(Knob::OSPF_SWEEP_TWINLV) && 2ull * nbfs > d.n_cover) d.twin_lv = false;
    if (!d.twin_lv) {
      std::fill(in_d.begin(), in_d.end(), 0);
      std::fill(seed.begin(), seed.end(), 0);
    }
  }
  d.lap("cover rows + twin levels set");
}

// The leaves' launch order and groups, the BFS and derived cover rows and
// their positions, the twin-levels groups.
void derive_rows(DerivePlan& d) {
  const Facts& f = d.f;
  const uint32_t V = d.V;
  // leaves: with twin levels, BFS'd representatives first (next-hop rows
  // only), then the others; without, when only twin representatives' level
  // rows are read, the representatives go first in a launch of their own,
  // so the next hops of the cover roots start while the other leaves' rows
  // are written
  // (OSPF_SWEEP_MERGE_REPS: the BFS'd leaf representatives' next hops in
  // their groups' leaf launch -- rows re-derived there, identical -- instead
  // of a launch of their own that reads each one's neighbour rows alone)
  const bool merge_reps = d.twin_lv && knob_flag(Knob::OSPF_SWEEP_MERGE_REPS);
  for (uint32_t x : d.need_l) {
    const bool first = d.twin_lv ? (d.seed[x] != 0 && !merge_reps)
                                 : (!d.all_leaf_rows && d.tw.rep[d.tw.cls[x]] == x);
    (first ? d.reps : d.rest).push_back(x);
  }
  d.grp_r = leaf_groups(d.c, f, d.reps);
  d.grp = leaf_groups(d.c, f, d.rest);
  d.lap("leaf groups");
  d.need_l = d.reps;
  d.need_l.insert(d.need_l.end(), d.rest.begin(), d.rest.end());
  d.nR = (uint32_t)d.reps.size();
  d.nL = (uint32_t)d.need_l.size();
  // rows: BFS rows (cover rows not derived + seed leaves), derived cover
  // rows, then the leaves that are not BFS rows
  std::vector<uint32_t>&clo = d.clo, &drv = d.drv;
  for (uint32_t v = 0; v < V; ++v) {
    if ((d.in_a[v] && !d.in_d[v]) || d.seed[v]) clo.push_back(v);
    else if (d.in_d[v]) drv.push_back(v);
  }
  locality_order(clo, [&](uint32_t v) { return f.first(v); });
  locality_order(drv, [&](uint32_t v) { return f.last(v); });
  const uint32_t nc = d.nc = (uint32_t)clo.size(), nd = d.nd = (uint32_t)drv.size();
  d.pos.assign(V, kNone);
  for (uint32_t i = 0; i < nc; ++i) d.pos[clo[i]] = i;
  for (uint32_t i = 0; i < nd; ++i) d.pos[drv[i]] = nc + i;
  // twin-levels groups: <= 8 consecutive derived rows (a pod's fabric
  // switches) reading <= kTwinMaxC class rows together (OSPF_TWIN_LV_G=4:
  // <= 4 rows, the launch's 4-root kernel with half the per-root registers)
  std::vector<uint32_t>& dgo = d.dgo;
  dgo.assign(1, 0u);
  const uint32_t tlg = knob_int(Knob::OSPF_TWIN_LV_G) == 4 ? 4u : ospf::kTwinLvG;
  if (nd) {
    std::vector<uint32_t> cl;
    for (uint32_t i = 0; i < nd; ++i) {
      d.classes_of(drv[i]);
      std::vector<uint32_t> u = cl;
      u.insert(u.end(), d.cs.begin(), d.cs.end());
      std::sort(u.begin(), u.end());
      u.erase(std::unique(u.begin(), u.end()), u.end());
      if (i > dgo.back() && (i - dgo.back() >= tlg || u.size() > ospf::kTwinMaxC)) {
        dgo.push_back(i);
        u = d.cs;
      }
      cl.swap(u);
    }
    dgo.push_back(nd);
  }
  d.n_dgrp = (uint32_t)dgo.size() - 1;
}

// pipeline stages: the derived rows in S stages of whole groups (blocks of
// pods on a fabric); a leaf group or a twin next-hop root waits only for
// the stage of the derived rows it reads, so the leaves' row stores run
// beside the later stages (OSPF_SWEEP_STAGES; default 1: F100k measured
// 24.2 ms per sweep with one stage, 26.3 with 4, 28.1 with 8 -- the later
// phase is HBM-bound and the staged twin-level launches lose efficiency)
void derive_stages(DerivePlan& d) {
  uint32_t S = 0;
  if (d.nd) {
    S = 1;
    S = (uint32_t)knob_int(Knob::OSPF_SWEEP_STAGES, (int)S);
    S = std::min(S, d.n_dgrp);
  }
  d.S = S;
  std::vector<uint32_t>&sg = d.sg, &lsg = d.lsg, &grp = d.grp, &rest = d.rest;
  sg.assign(S + 1, 0u);  // first group of each stage
  d.stage_of.assign(d.V, -1);
  for (uint32_t k = 0; k <= S; ++k) sg[k] = (uint32_t)((uint64_t)k * d.n_dgrp / std::max(1u, S));
  for (uint32_t k = 0; k < S; ++k)
    for (uint32_t i = d.dgo[sg[k]]; i < d.dgo[sg[k + 1]]; ++i) d.stage_of[d.drv[i]] = (int)k;
  lsg.assign(S + 1, 0u);  // first leaf group of each stage (rest)
  if (S > 1 && d.nL > d.nR) {
    const uint32_t ngr0 = (uint32_t)grp.size() - 1;
    std::vector<uint32_t> gi(ngr0), gdep(ngr0);
    for (uint32_t x = 0; x < ngr0; ++x) {
      gi[x] = x;
      gdep[x] = (uint32_t)d.dep_of(rest[grp[x]], false);
    }
    std::stable_sort(gi.begin(), gi.end(), [&](uint32_t a, uint32_t b) { return gdep[a] < gdep[b]; });
    std::vector<uint32_t> r2, g2{0u};
    for (uint32_t x : gi) {
      r2.insert(r2.end(), rest.begin() + grp[x], rest.begin() + grp[x + 1]);
      g2.push_back((uint32_t)r2.size());
    }
    rest.swap(r2);
    grp.swap(g2);
    d.need_l.resize(d.nR);
    d.need_l.insert(d.need_l.end(), rest.begin(), rest.end());
    for (uint32_t k = 0, x = 0; k <= S; ++k) {
      while (x < ngr0 && gdep[gi[x]] < k) ++x;
      lsg[k] = k == S ? ngr0 : x;
    }
  }
  d.lap("rows + stages");
}

// Every allocation the units read, in the order the pool hands blocks out,
// then the digests and the events.
int derive_alloc(DerivePlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  DeriveDev& v = d.dev;
  const uint32_t V = d.V, nc = d.nc, nd = d.nd, nL = d.nL, nR = d.nR;
  uint32_t rows = nc + nd;
  for (uint32_t i = 0; i < nL; ++i)
    if (d.pos[d.need_l[i]] == kNone) d.pos[d.need_l[i]] = rows++;
  d.rows = rows;
  // level rows (bytes), dist and leaf next-hop rows 128-B aligned (pitch a multiple of 32
  // words): every 1-KB wave store of the row writers then covers whole lines
  // (ospf_probe_store, leaf-shaped rows at V = 100,024: 7.0 TB/s aligned
  // against 5.8 TB/s at the 400,096-B pitch; profiles/r06/a3_*)
  v.V = V;
  v.hop = s->opts.flags & OSPF_HOP_COUNT;
  const uint32_t DP = v.DP = row_pitch(V);
  const uint32_t pitch = v.pitch = DP == V ? (V + 15) / 16 * 16 : (V + 127) / 128 * 128;
  int rc;
  if ((rc = upload(s, &v.d_pos, d.pos)) || (rc = dalloc(s, &v.lev, (size_t)rows * pitch)) ||
      (rc = dalloc(s, &v.dist, (size_t)rows * DP)) || (rc = dalloc(s, &v.ldg, std::max(1u, nc + nd))))
    return rc;
  if (nc && (rc = upload(s, &v.d_clo, d.clo))) return rc;
  if (nL && ((rc = upload(s, &v.d_l, d.need_l)) || (rc = dalloc(s, &v.lnh, (size_t)nL * DP))))
    return rc;
  if (nR && (rc = upload(s, &v.d_grp_r, d.grp_r))) return rc;
  if (nL > nR && (rc = upload(s, &v.d_grp, d.grp))) return rc;
  // level bytes not kept: BFS'd representatives (their BFS rows stay), and
  // the other leaves unless a non-twin class reads every leaf row
  d.drop_rest = !d.all_leaf_rows && nL > nR;
  if (d.drop_rest || (d.twin_lv && nR)) {
    std::vector<uint32_t> lout(std::max(d.drop_rest ? nL - nR : 0u, d.twin_lv ? nR : 0u), kNone);
    if ((rc = upload(s, &v.d_lout, lout))) return rc;
  }
  d.lap("allocations + uploads");
  bool any_twin = nd > 0;
  for (auto& k : d.cls) any_twin |= k.twin;
  if (any_twin && ((rc = upload(s, &v.d_tcls, d.tw.cls)) || (rc = upload(s, &v.d_trep, d.tw.rep)) ||
                   (rc = upload(s, &v.d_tsec, d.tw.sec))))
    return rc;
  s->dig_aux.push_back({v.ldg, std::max(1u, nc + nd)});
  s->n_rows = rows;
  s->trav_edges = (uint64_t)nc * c->info.n_edges;  // the seed BFS rows; the rest is derived
  const uint32_t ndig = (uint32_t)d.own_c.size() + nL;
  if ((rc = dalloc(s, &s->dig_all, ndig))) return rc;
  s->n_dig = ndig;
  // events: levels done, cover rows done (= levels without twin levels),
  // representative leaves done, every leaf done
  d.ev_a = new_event(s), d.ev_t = new_event(s), d.ev_r = new_event(s), d.ev_b = new_event(s);
  if (d.ev_a < 0 || d.ev_t < 0 || d.ev_r < 0 || d.ev_b < 0) return std::min({d.ev_a, d.ev_t, d.ev_r, d.ev_b});
  d.ev_s.resize(d.S);
  for (uint32_t k = 0; k < d.S; ++k) {
    d.ev_s[k] = k + 1 == d.S ? d.ev_t : new_event(s);
    if (d.ev_s[k] < 0) return d.ev_s[k];
  }
  d.ev_cov = nd ? d.ev_t : d.ev_a;
  return OSPF_OK;
}

// (A) the seed BFS, (A') the twin-levels stages: the serial prefix of a run
int derive_levels_units(DerivePlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const DeriveDev v = d.dev;
  const uint32_t V = d.V, nc = d.nc;
  int rc;
  if (nc) {
    Unit lv;
    lv.name = "levels";
    lv.kernel = "ospf_levels_dev (lv_init + lv_level/lv_settle per level + lv_rows: "
                "distance-only 128-root BFS, dist + level rows)";
    lv.stream = 0;
    lv.record = d.ev_a;
    lv.n_roots = nc;
    lv.comp = (uint64_t)nc * 4ull * V + ((nc + 127) / 128) * scan_bytes(c, false);
    if ((rc = upload(s, &s->d_lv_maxd, std::vector<uint32_t>{0u}))) return rc;
    // (s->lv_cap: read at launch time -- the depth the first run reached)
    lv.fn = [=](hipStream_t st) {
      return ospf_int::levels_dev(c, v.d_clo, nc, v.hop, v.dist, v.DP, v.lev, v.pitch, v.ldg, st,
                                  s->lv_cap, s->d_lv_maxd);
    };
    add_unit(s, std::move(lv));
  }
  // the twin next-hop launches write their roots' dist rows (from the level
  // rows they read anyway), off the serial prefix
  std::vector<uint8_t> twin_nh(V, 0);
  for (const auto& k : d.cls)
    if (k.twin)
      for (uint32_t r : k.roots) twin_nh[r] = 1;
  for (uint32_t k = 0; k < d.S; ++k) {
    const uint32_t i0 = d.dgo[d.sg[k]], n = d.dgo[d.sg[k + 1]] - i0;
    std::vector<uint32_t> gk, rk(d.drv.begin() + i0, d.drv.begin() + i0 + n);
    for (uint32_t g = d.sg[k]; g <= d.sg[k + 1]; ++g) gk.push_back(d.dgo[g] - i0);
    // the stage's plan, built once on the host (spf_twin.hip twin_levels_kernel)
    ospf_int::TwinLvHost h;
    if ((rc = ospf_int::twin_lv_build(c, rk, gk, d.pos, d.tw.cls, d.tw.rep, h))) return sfail(s, rc, c->err);
    // roots whose twin next-hop launch writes their dist rows: level rows only here
    if (d.twin_lv)
      for (auto& ri : h.rinfo)
        if (twin_nh[ri.x]) ri.z |= 0x80000000u;
    ospf::TwinLvPlan plan{};
    uint32_t *d_grp2, *d_grow, *d_nbo, *d_nbl;
    uint4* d_rinfo;
    if ((rc = upload(s, &d_grp2, h.grp)) || (rc = upload(s, &d_grow, h.grow)) ||
        (rc = upload(s, &d_nbo, h.nbo)) || (rc = upload(s, &d_nbl, h.nbl)) ||
        (rc = upload(s, &d_rinfo, h.rinfo)))
      return rc;
    plan.n = n;
    plan.ngroups = (uint32_t)h.grp.size() - 1;
    plan.gsz = h.gmax;
    plan.grp = d_grp2;
    plan.grow = d_grow;
    plan.rinfo = d_rinfo;
    plan.nbo = d_nbo;
    plan.nbl = d_nbl;
    plan.lev = v.lev;
    plan.pitch = v.pitch;
    plan.dist = v.dist;
    plan.dpitch = v.DP;
    plan.lev_digest = v.ldg;
    Unit u;
    u.name = d.S > 1 ? "twin_levels_s" + std::to_string(k) : std::string("twin_levels");
    u.kernel = "ospf_twin_levels_dev (twin_levels_kernel: level + dist rows from the neighbour "
               "classes' representative rows)";
    u.stream = 0;
    u.record = d.ev_s[k];
    u.n_roots = n;
    // the unit: the dist rows it writes + its level rows (read by the
    // leaves); the step counts only the dist rows (level rows are
    // intermediate)
    uint64_t nd_rows = 0;
    for (const auto& ri : h.rinfo) nd_rows += (ri.z >> 31) ? 0u : 1u;
    u.comp = nd_rows * 4ull * V + (uint64_t)n * V;
    u.fn = [=](hipStream_t st) { return ospf_int::twin_lv_launch(c, plan, st); };
    add_unit(s, std::move(u), nd_rows * 4ull * V);
  }
  // OSPF_SWEEP_EARLY_START: the serial prefix starts now, the host plans on
  if ((rc = start_early(s))) return rc;
  d.lap("twin levels units");
  return OSPF_OK;
}

// the launch of a twin class's next hops (+ the roots' dist rows with twin levels)
std::function<int(hipStream_t)> twin_nh_fn(ospf_ctx* c, const DeriveDev& dev, bool nh_dist,
                                           const uint32_t* d_roots, uint32_t n, uint32_t W, uint32_t cap,
                                           uint32_t* nh, uint32_t NPW, ospf_digest* dg) {
  const DeriveDev v = dev;
  uint32_t* dd = nh_dist ? v.dist : nullptr;
  return [=](hipStream_t strm) {
    return ospf_int::nh_derive_twin_launch(c, d_roots, n, W, cap, v.lev, v.pitch, v.d_pos, v.ldg, v.d_tcls,
                                           v.d_trep, v.d_tsec, nh, dg, dd, strm, v.DP, NPW);
  };
}

// A twin class with staged twin levels: one launch per stage of the roots'
// own rows (roots ordered by stage), beside the later stages.
void derive_twin_stage_units(DerivePlan& d, const Cls& k, int st, const uint32_t* d_roots, uint32_t* nh,
                             uint32_t NPW, ospf_digest* dg) {
  const uint32_t n = (uint32_t)k.roots.size(), W = k.W, cap = std::min(k.cap, 2048u);
  for (uint32_t q = 0, a0 = 0; q < d.S; ++q) {
    uint32_t a1 = a0;
    while (a1 < n && (uint32_t)d.dep_of(k.roots[a1], true) <= q) ++a1;
    if (a1 == a0) continue;
    Unit u;
    u.name = "derive_cap" + std::to_string(k.cap) + "_s" + std::to_string(q);
    u.kernel = "ospf_nh_derive_twin_dev (nh_twin4_kernel, " + std::to_string(W) +
               " next-hop word" + (W > 1 ? "s)" : ")");
    u.stream = st;
    u.wait = {d.ev_s[q]};
    u.n_roots = a1 - a0;
    u.W = W;
    u.comp = (uint64_t)(a1 - a0) * 4ull * d.V * (W + (d.twin_lv ? 1u : 0u));
    u.fn = twin_nh_fn(d.c, d.dev, d.twin_lv, d_roots + a0, a1 - a0, W, cap, nh + (size_t)a0 * NPW, NPW,
                      dg + a0);
    d.side.push_back(std::move(u));
    a0 = a1;
  }
}

// spines: the planned tile-staged kernel (host-built runs and slot tables)
int derive_wide_unit(DerivePlan& d, const Cls& k, int st, uint32_t* nh, ospf_digest* dg) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const uint32_t n = (uint32_t)k.roots.size(), W = k.W;
  int rc;
  WideHost wh;
  if ((rc = wide_plan_build(c, d.f, k.roots, W, d.pos, wh))) return sfail(s, rc, c->err);
  ospf::WidePlan plan{};
  uint32_t *d_run, *d_soff, *d_slots, *d_keep, *d_own;
  if ((rc = upload(s, &d_run, wh.run)) || (rc = upload(s, &d_soff, wh.soff)) ||
      (rc = upload(s, &d_slots, wh.slots)) || (rc = upload(s, &d_keep, wh.keep)) ||
      (rc = upload(s, &d_own, wh.own)))
    return rc;
  plan.n = n;
  plan.W = W;
  plan.nruns = (uint32_t)wh.run.size() - 1;
  plan.run = d_run;
  plan.soff = d_soff;
  plan.slots = d_slots;
  plan.keep = d_keep;
  plan.own = d_own;
  plan.lev = d.dev.lev;
  plan.pitch = d.dev.pitch;
  plan.lev_digest = d.dev.ldg;
  plan.nh = nh;
  plan.digest = dg;
  Unit u;
  u.name = "derive_cap" + std::to_string(k.cap);
  u.kernel = "nh_wide_plan_kernel (" + std::to_string(W) + " next-hop words: host-planned runs, "
             "16-node tiles staged in LDS)";
  u.stream = st;
  u.wait = {!k.reads_leaf ? d.ev_cov : d.ev_b};
  if (u.wait[0] == d.ev_b && d.nd) u.wait.push_back(d.ev_cov);
  u.n_roots = n;
  u.W = W;
  u.comp = (uint64_t)n * 4ull * d.V * W;
  u.fn = [=](hipStream_t strm) {
    const hipError_t e = ospf::launch_wide_plan(c->g, plan, strm);
    if (e != hipSuccess) return hip_fail(c, e, "launch_wide_plan");
    return (int)OSPF_OK;
  };
  (u.wait[0] == d.ev_b ? d.after : d.side).push_back(std::move(u));
  return OSPF_OK;
}

// (C) cover classes: digest slots 0 .. |own_c|, each class on its own stream.
// Units that wait for leaf rows queue behind the leaves' (`after`).
int derive_cover_units(DerivePlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const DeriveDev v = d.dev;
  const uint32_t V = d.V;
  int rc;
  for (Cls& k : d.cls) {
    const bool staged = k.twin && d.twin_lv && d.S > 1;
    if (staged)
      std::stable_sort(k.roots.begin(), k.roots.end(), [&](uint32_t a, uint32_t b) {
        return d.dep_of(a, true) < d.dep_of(b, true);
      });
    const uint32_t n = (uint32_t)k.roots.size(), W = k.W, cap = std::min(k.cap, 2048u);
    uint32_t *d_roots, *nh;
    // twin classes' next-hop rows 128-B aligned too (nh_twin4_kernel
    // stores each 1,024-node tile's W words as one run)
    const uint32_t NPW = k.twin ? row_pitch(V * W) : V * W;
    if ((rc = upload(s, &d_roots, k.roots)) || (rc = dalloc(s, &nh, (size_t)n * NPW))) return rc;
    ospf_digest* dg = s->dig_all + d.slot;
    own_rows(s, k.roots, d.slot, v.dist, v.DP, nh, NPW, W, &d.pos);
    d.slot += n;
    const int st = new_stream(s);
    if (st < 0) return st;
    if (staged) {
      derive_twin_stage_units(d, k, st, d_roots, nh, NPW, dg);
      continue;
    }
    if (!k.twin && W > 4 && W <= 64 && !knob_flag(Knob::OSPF_DERIVE_WIDE1)) {
      if ((rc = derive_wide_unit(d, k, st, nh, dg))) return rc;
      continue;
    }
    Unit u;
    u.name = "derive_cap" + std::to_string(k.cap);
    u.kernel = std::string(k.twin ? "ospf_nh_derive_twin_dev (" : "ospf_nh_derive_dev (") +
               (k.twin ? "nh_twin4_kernel" : W <= 4 ? "nh_derive16_kernel"
                                                          : "nh_derive_wide_kernel") +
               ", " + std::to_string(W) + " next-hop word" + (W > 1 ? "s)" : ")");
    u.stream = st;
    // twin classes read the representatives' rows (BFS'd with twin levels);
    // the others every neighbour's row
    u.wait = {!k.reads_leaf ? d.ev_cov : k.twin ? (d.twin_lv ? d.ev_cov : d.ev_r) : d.ev_b};
    // every leaf row (ev_b) does not imply every derived cover row when the
    // last leaf stage precedes the last twin-levels stage
    if (u.wait[0] == d.ev_b && d.nd) u.wait.push_back(d.ev_cov);
    u.n_roots = n;
    u.W = W;
    u.comp = (uint64_t)n * 4ull * V * (W + (k.twin && d.twin_lv ? 1u : 0u));
    if (k.twin) {
      u.fn = twin_nh_fn(c, v, d.twin_lv, d_roots, n, W, cap, nh, NPW, dg);
    } else {
      u.fn = [=](hipStream_t strm) {
        return ospf_nh_derive_dev(c, d_roots, n, W, cap, v.lev, v.pitch, v.d_pos, v.ldg, nh, dg, strm);
      };
    }
    (u.wait[0] == d.ev_b || u.wait[0] == d.ev_r ? d.after : d.side).push_back(std::move(u));
  }
  for (auto& x : d.side) add_unit(s, std::move(x));
  d.lap("cover next-hop units");
  return OSPF_OK;
}

// (B) leaves: digest slots after the cover roots'; representatives first
int derive_leaf_units(DerivePlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const DeriveDev v = d.dev;
  const uint32_t V = d.V, nL = d.nL, nR = d.nR, S = d.S;
  const std::vector<uint32_t>& grp = d.grp;
  const bool twin_lv = d.twin_lv;
  int rc;
  if (nL) {
    uint32_t kmax = 1;
    for (uint32_t r : d.need_l) kmax = std::max(kmax, d.f.nbrs(r));
    own_rows(s, d.need_l, d.slot, v.dist, v.DP, v.lnh, v.DP, 1, &d.pos, &d.in_l);
    ospf_digest* dg = s->dig_all + d.slot;
    const uint32_t ngr_r = nR ? (uint32_t)d.grp_r.size() - 1 : 0u;
    const uint32_t ngr = nL > nR ? (uint32_t)grp.size() - 1 : 0u;
    const uint32_t* lo_rest = d.drop_rest ? v.d_lout : nullptr;
    const char* const leaf_kernel = "ospf_leaf_derive2_dev (leaf_derive_kernel: level + dist + next-hop "
                                    "rows of leaf roots from their neighbours' level rows)";
    if (nR) {
      Unit u;
      u.name = twin_lv ? "leaf_seeds" : "leaf_reps";
      u.kernel = twin_lv ? "ospf_leaf_derive2_dev (leaf_derive_kernel: next-hop rows of BFS'd "
                           "leaf representatives)"
                         : "ospf_leaf_derive2_dev (leaf_derive_kernel: twin representatives' level "
                           "+ dist + next-hop rows)";
      if (twin_lv) {  // beside the other leaves, after the cover rows
        const int st = new_stream(s);
        if (st < 0) return st;
        u.stream = st;
        u.wait = {d.ev_cov};
      } else {
        u.stream = 0;
      }
      u.record = d.ev_r;
      u.n_roots = nR;
      u.W = 1;
      u.comp = (uint64_t)nR * (twin_lv ? 4ull : 8ull) * V;
      const uint32_t* lo = twin_lv ? v.d_lout : nullptr;
      uint32_t* dd = twin_lv ? nullptr : v.dist;
      u.fn = [=](hipStream_t strm) {
        return ospf_int::leaf_derive(c, v.d_l, nR, v.d_grp_r, ngr_r, kmax, v.lev, v.pitch, v.d_pos, lo, dd,
                                     v.DP, v.lnh, v.DP, dg, strm);
      };
      add_unit(s, std::move(u));
    }
    if (nL > nR && twin_lv && S > 1) {
      const int lst = new_stream(s);
      if (lst < 0) return lst;
      for (uint32_t q = 0; q < S; ++q) {
        const uint32_t g0 = d.lsg[q], g1 = d.lsg[q + 1];
        if (g1 == g0) continue;
        const uint32_t i0 = grp[g0], n = grp[g1] - i0;
        std::vector<uint32_t> gq;
        for (uint32_t g = g0; g <= g1; ++g) gq.push_back(grp[g] - i0);
        uint32_t* d_gq;
        if ((rc = upload(s, &d_gq, gq))) return rc;
        Unit u;
        u.name = "leaf_s" + std::to_string(q);
        u.kernel = leaf_kernel;
        u.stream = lst;
        u.wait = {d.ev_s[q]};
        if (g1 == (uint32_t)grp.size() - 1) u.record = d.ev_b;
        u.n_roots = n;
        u.W = 1;
        u.comp = (uint64_t)n * 8ull * V;
        const uint32_t* dl = v.d_l + nR + i0;
        uint32_t* nh = v.lnh + (size_t)(nR + i0) * v.DP;
        ospf_digest* dg2 = dg + nR + i0;
        const uint32_t ngq = g1 - g0;
        u.fn = [=](hipStream_t strm) {
          return ospf_int::leaf_derive(c, dl, n, d_gq, ngq, kmax, v.lev, v.pitch, v.d_pos, lo_rest, v.dist,
                                       v.DP, nh, v.DP, dg2, strm);
        };
        add_unit(s, std::move(u));
      }
    } else if (nL > nR) {
      Unit u;
      u.name = "leaf";
      u.kernel = leaf_kernel;
      const uint32_t n = nL - nR;
      if (nR && !twin_lv) {  // beside the cover roots' next hops, on a stream of its own
        const int st = new_stream(s);
        if (st < 0) return st;
        u.stream = st;
        u.wait = {d.ev_a};
      } else {
        u.stream = 0;
      }
      u.record = d.ev_b;
      u.n_roots = n;
      u.W = 1;
      u.comp = (uint64_t)n * 8ull * V;
      const uint32_t* dl = v.d_l + nR;
      uint32_t* nh = v.lnh + (size_t)nR * v.DP;
      ospf_digest* dg2 = dg + nR;
      // (s->leaf_order: read at launch time -- pick_leaf_order sets it after the first run)
      u.fn = [=](hipStream_t strm) {
        return ospf_int::leaf_derive(c, dl, n, v.d_grp, ngr, kmax, v.lev, v.pitch, v.d_pos, lo_rest, v.dist,
                                     v.DP, nh, v.DP, dg2, strm, s->leaf_order);
      };
      add_unit(s, std::move(u));
    }
  }
  d.lap("next-hop + leaf units");
  return OSPF_OK;
}

// the cover units behind the leaves; an event no launch records stands for
// the one before it
void derive_alias_events(DerivePlan& d) {
  auto alias = [&](int from, int to) {
    for (auto& u : d.after)
      for (int& e : u.wait)
        if (e == from) e = to;
  };
  if (!(d.nL > d.nR)) alias(d.ev_b, d.nR ? d.ev_r : d.ev_cov);
  if (!d.nR) alias(d.ev_r, d.ev_cov);
  for (auto& x : d.after) add_unit(d.s, std::move(x));
}

}  // namespace

int ospf_int::sweep::plan_derive(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine) {
  DerivePlan d(s, f, mine);
  int rc;
  derive_leaf_closure(d);
  derive_classes(d);
  derive_cover_rows(d);
  derive_rows(d);
  derive_stages(d);
  if ((rc = derive_alloc(d)) || (rc = derive_levels_units(d)) || (rc = derive_cover_units(d)) ||
      (rc = derive_leaf_units(d)))
    return rc;
  derive_alias_events(d);
  return OSPF_OK;
}
