// sweep_plan_weighted.hip — the planners of a sweep over link metrics
// (sweep_impl.h): WCOVER (the weighted headline: contracted cover graph,
// closure), WMULTI and WDERIVE, with the host plans only WCOVER builds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "sweep_impl.h"

using namespace ospf_int;
using namespace ospf_int::sweep;

namespace {

// Host plan of the weighted run kernel (wnh_runs_kernel) for wide cover
// roots (in order): runs of <= kWrRun roots with the same distinct
// neighbours; per run its slot table over dist-row positions (padded to 32 W),
// per root the smallest metric of its up links per slot.
struct WRunsHost {
  std::vector<uint4> run;
  std::vector<uint32_t> slots, wt, own, rootid;
};
int wruns_build(ospf_ctx* c, const Facts& f, const std::vector<uint32_t>& roots, uint32_t W,
                const std::vector<uint32_t>& pos, WRunsHost& h) {
  const uint32_t n = (uint32_t)roots.size(), KW = 32u * W;
  h = WRunsHost{};
  h.wt.assign((size_t)n * KW, kNone);
  auto same = [&](uint32_t a, uint32_t b) { return f.same_nbrs(a, b); };
  std::vector<uint32_t> first;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i];
    if (pos[r] == kNone) return fail(c, OSPF_E_RANGE, "wruns plan: a root without a row");
    h.own.push_back(pos[r]);
    h.rootid.push_back(r);
    const uint32_t* dn = f.dn->data() + (*f.dn_off)[r];
    const uint32_t K = f.nbrs(r);
    if (K > KW) return fail(c, OSPF_E_RANGE, "wruns plan: too many neighbours");
    for (uint32_t e = c->h_prow[r]; e < c->h_prow[r + 1]; ++e) {
      const uint32_t x = c->h_pcolx[e];
      if ((x & 0x80000000u) || x == r) continue;
      const uint32_t k = (uint32_t)(std::lower_bound(dn, dn + K, x) - dn);
      uint32_t& m = h.wt[(size_t)i * KW + k];
      m = std::min(m, c->h_pw[e]);
    }
    if (i == 0 || i - first.back() >= ospf::kWrRun || !same(roots[first.back()], r)) first.push_back(i);
  }
  first.push_back(n);
  for (size_t q = 0; q + 1 < first.size(); ++q) {
    const uint32_t r0 = roots[first[q]], K = f.nbrs(r0);
    const uint32_t* dn = f.dn->data() + (*f.dn_off)[r0];
    const uint32_t off = (uint32_t)h.slots.size();
    for (uint32_t k = 0; k < KW; ++k) {
      bool used = false;
      for (uint32_t i = first[q]; i < first[q + 1] && k < K && !used; ++i)
        used = h.wt[(size_t)i * KW + k] != kNone;
      uint32_t v = kNone;
      if (used) {
        const uint32_t x = dn[k];
        if ((c->h_nt[x >> 5] >> (x & 31)) & 1u) {
          v = 0x80000000u | x;
        } else {
          v = pos[x];
          if (v == kNone) return fail(c, OSPF_E_RANGE, "wruns plan: a neighbour without a row");
        }
      }
      h.slots.push_back(v);
    }
    h.run.push_back(make_uint4(first[q], first[q + 1] - first[q], off, 0u));
  }
  return OSPF_OK;
}

// Host plan of the weighted hub kernel (wnh_hub_kernel) for narrow cover
// roots (W <= 4, in order): hub rows = the transit neighbours most roots read
// (>= 16 roots, at most kHubMax, most-read first); groups = runs of <= 16
// consecutive roots whose own rows plus non-hub transit neighbours' rows
// number <= kHubLoc. OSPF_E_RANGE when a root alone needs more group rows.
struct HubHost {
  std::vector<uint32_t> hub, loc, ref, wt, ownl, rootid;
  std::vector<uint4> grp;
};
int hub_build(ospf_ctx* c, const Facts& f, const std::vector<uint32_t>& roots, uint32_t W,
              const std::vector<uint32_t>& pos, HubHost& h) {
  const uint32_t n = (uint32_t)roots.size(), KW = 32u * W, V = f.V;
  h = HubHost{};
  h.wt.assign((size_t)n * KW, kNone);
  auto nt = [&](uint32_t x) { return (c->h_nt[x >> 5] >> (x & 31)) & 1u; };
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i];
    const uint32_t* dn = f.dn->data() + (*f.dn_off)[r];
    const uint32_t K = f.nbrs(r);
    if (K > KW) return fail(c, OSPF_E_RANGE, "hub plan: too many neighbours");
    for (uint32_t e = c->h_prow[r]; e < c->h_prow[r + 1]; ++e) {
      const uint32_t x = c->h_pcolx[e];
      if ((x & 0x80000000u) || x == r) continue;
      const uint32_t k = (uint32_t)(std::lower_bound(dn, dn + K, x) - dn);
      uint32_t& m = h.wt[(size_t)i * KW + k];
      m = std::min(m, c->h_pw[e]);
    }
  }
  std::vector<uint32_t> cnt(V, 0u);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t r = roots[i];
    const uint32_t* dn = f.dn->data() + (*f.dn_off)[r];
    for (uint32_t k = 0; k < f.nbrs(r); ++k)
      if (h.wt[(size_t)i * KW + k] != kNone && !nt(dn[k])) ++cnt[dn[k]];
  }
  std::vector<uint32_t> cand;
  for (uint32_t v = 0; v < V; ++v)
    if (cnt[v] >= 16u) cand.push_back(v);
  std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return cnt[a] > cnt[b]; });
  if (cand.size() > ospf::kHubMax) cand.resize(ospf::kHubMax);
  std::vector<uint32_t> hub_of(V, kNone);
  for (uint32_t j = 0; j < cand.size(); ++j) {
    hub_of[cand[j]] = j;
    if (pos[cand[j]] == kNone) return fail(c, OSPF_E_RANGE, "hub plan: a neighbour without a row");
    h.hub.push_back(pos[cand[j]]);
  }
  std::vector<uint32_t> locs;  // the open group's row nodes
  auto need = [&](uint32_t i, std::vector<uint32_t>& out) {
    const uint32_t r = roots[i];
    const uint32_t* dn = f.dn->data() + (*f.dn_off)[r];
    out.assign(1, r);
    for (uint32_t k = 0; k < f.nbrs(r); ++k)
      if (h.wt[(size_t)i * KW + k] != kNone && (nt(dn[k]) || hub_of[dn[k]] == kNone))
        out.push_back(nt(dn[k]) && dn[k] != r ? (0x80000000u | dn[k]) : dn[k]);
  };
  auto close = [&](uint32_t first, uint32_t end) {
    h.grp.push_back(make_uint4(first, end - first, (uint32_t)h.loc.size(), (uint32_t)locs.size()));
    for (uint32_t x : locs) {
      if (x & 0x80000000u) {
        h.loc.push_back(x);
        continue;
      }
      if (pos[x] == kNone) return false;
      h.loc.push_back(pos[x]);
    }
    return true;
  };
  std::vector<uint32_t> nd;
  uint32_t gfirst = 0;
  for (uint32_t i = 0; i < n; ++i) {
    need(i, nd);
    std::vector<uint32_t> merged = locs;
    for (uint32_t x : nd)
      if (std::find(merged.begin(), merged.end(), x) == merged.end()) merged.push_back(x);
    if (i > gfirst && (merged.size() > ospf::kHubLoc || i - gfirst >= ospf::kHubGrpRoots)) {
      if (!close(gfirst, i)) return fail(c, OSPF_E_RANGE, "hub plan: a row is missing");
      gfirst = i;
      locs.clear();
      merged.clear();
      for (uint32_t x : nd)
        if (std::find(merged.begin(), merged.end(), x) == merged.end()) merged.push_back(x);
    }
    if (merged.size() > ospf::kHubLoc) return fail(c, OSPF_E_RANGE, "hub plan: a root needs > 64 group rows");
    locs = merged;
  }
  if (n && !close(gfirst, n)) return fail(c, OSPF_E_RANGE, "hub plan: a row is missing");
  // slot refs and own rows per root
  h.ref.assign((size_t)n * KW, kNone);
  for (const uint4& gr : h.grp) {
    const uint32_t* L = h.loc.data() + gr.z;
    const uint32_t nhub = (uint32_t)h.hub.size();
    for (uint32_t i = gr.x; i < gr.x + gr.y; ++i) {
      const uint32_t r = roots[i];
      const uint32_t* dn = f.dn->data() + (*f.dn_off)[r];
      auto lidx = [&](uint32_t tag) {  // src row or 0x80000000 | node
        for (uint32_t l = 0; l < gr.w; ++l)
          if (L[l] == tag) return nhub + l;
        return kNone;
      };
      h.ownl.push_back(lidx(pos[r]));
      h.rootid.push_back(r);
      for (uint32_t k = 0; k < KW; ++k) {
        uint32_t& rf = h.ref[(size_t)i * KW + k];
        rf = nhub + ospf::kHubLoc;  // the unreached row
        if (k >= f.nbrs(r) || h.wt[(size_t)i * KW + k] == kNone) continue;
        const uint32_t x = dn[k];
        if (nt(x) && x != r) rf = lidx(0x80000000u | x);
        else if (hub_of[x] != kNone) rf = hub_of[x];
        else rf = lidx(pos[x]);
        if (rf == kNone) return fail(c, OSPF_E_RANGE, "hub plan: a slot row is missing");
      }
    }
  }
  return OSPF_OK;
}
// Node tiles for the closure rows (launch_closure_rows): consecutive nodes, a
// tile closed at kLtNodes nodes or when its union of cover indices (a cover
// node's own, a leaf's in-links') would pass kLtU. False when a leaf has
// more than kLtE in-links.
struct NodeTiles {
  std::vector<uint4> tile;
  std::vector<uint32_t> le, u;
};
bool node_tiles(const ospf_ctx* c, NodeTiles& t) {
  const std::vector<uint32_t>& cix = c->h_cix;
  const uint32_t V = (uint32_t)cix.size(), nS = (uint32_t)c->h_ccv.size();
  std::vector<uint32_t> slot(nS, kNone), ul;
  uint32_t first = 0;
  auto close = [&](uint32_t end) {
    if (end == first) return;
    t.tile.push_back(make_uint4(first, end - first, (uint32_t)t.u.size(), (uint32_t)ul.size()));
    for (uint32_t ci : ul) {
      t.u.push_back(ci);
      slot[ci] = kNone;
    }
    ul.clear();
    first = end;
  };
  t.le.assign((size_t)V * ospf::kLtE, 0xFFFFFFFFu);
  for (uint32_t v = 0, l = 0; v < V; ++v) {
    uint32_t ent[ospf::kLtE], ne = 0, fresh = 0;
    if (cix[v] & 0x80000000u) {
      for (uint32_t x = c->h_lrow[l]; x < c->h_lrow[l + 1]; ++x) {
        const uint32_t w = c->h_ladj[x], ci = w & 0xFFFFu;
        if (ci >= nS) continue;  // padding
        if (ne == ospf::kLtE) return false;
        ent[ne++] = w;
        if (slot[ci] == kNone) ++fresh;  // (a repeat counts twice: a bound)
      }
      ++l;
    } else {
      ent[ne++] = cix[v];
      if (slot[cix[v]] == kNone) ++fresh;
    }
    if (v - first == ospf::kLtNodes || ul.size() + fresh > ospf::kLtU) close(v);
    for (uint32_t q = 0; q < ne; ++q) {
      const uint32_t ci = ent[q] & 0xFFFFu;
      if (slot[ci] == kNone) {
        slot[ci] = (uint32_t)ul.size();
        ul.push_back(ci);
      }
      t.le[(size_t)v * ospf::kLtE + q] =
          (cix[v] & 0x80000000u) ? (slot[ci] | (ent[q] & 0xFFFF0000u)) : (slot[ci] | 0x100u);
    }
  }
  close(V);
  return true;
}

// The device side of WCOVER's closure path: what its units' launches read. A
// unit's fn takes a copy of this, never the CoverPlan.
struct ClosureDev {
  uint32_t nS = 0, nsd = 0, ncl = 0, nsn = 0, NW = 0, NWs = 0, KW = 0;
  uint32_t *d_sd = nullptr, *d_srp = nullptr, *d_cl = nullptr, *d_crp = nullptr, *seedC = nullptr,
           *dc = nullptr;
  // next hops of the closure roots: the cover columns' masks out of the
  // closure, rows + digests out of the rows unit (null without)
  uint32_t *dcm = nullptr, *cnh = nullptr;
  ospf_digest* cdg = nullptr;
  // next hops of the part's seeds out of their Dial (null without)
  uint32_t *d_snp = nullptr, *snm = nullptr, *snh = nullptr, *sdf = nullptr, *d_sroots = nullptr,
           *d_srp2 = nullptr;
  ospf_digest* sdg = nullptr;
  // the seeds' rows on a stream of their own, beside the closure and its
  // rows (OSPF_SEED_ROWS_INLINE: inside the Dial's launch)
  bool seed_side = false;
  ospf::ClosurePlan cp{};
};

// Host state of plan_wcover, shared by its stages (in the order they fill
// it). Not copyable: a unit's fn that named it would not compile.
struct CoverPlan {
  ospf_sweep* const s;
  ospf_ctx* const c;
  const Facts& f;
  const std::vector<uint32_t>& mine;
  const std::vector<uint8_t>& leaf;
  const uint32_t V;
  CoverPlan(ospf_sweep* sw, const Facts& facts, const std::vector<uint32_t>& part,
            const std::vector<uint8_t>& leaves)
      : s(sw), c(sw->c), f(facts), mine(part), leaf(leaves), V(sw->V) {}
  CoverPlan(const CoverPlan&) = delete;
  // sets and rows: cover rows [0, nA), then the needed leaves' rows
  std::vector<uint32_t> own_l, own_c, c_der, c_wide, nb_c, need_l, cl, cover_a, pos;
  uint32_t nA = 0, nL = 0, kmax = 1;
  uint32_t *slab = nullptr, *d_pos = nullptr, *d_a = nullptr, *d_l = nullptr, *lnh = nullptr;
  // (A) the closure, when it applies, and whose next hops it carries
  std::vector<uint32_t> seeds, clos, sd_nh;
  ospf_int::ClosureHost ch;
  bool closure = false, cl_nh = false;
  uint32_t NW = 0, NWs = 0;
  ClosureDev cd;
  // digest slots, events
  uint32_t cl_dig0 = 0, sn_dig0 = 0, slot = 0;
  int ev_a = -1;                         // cover rows done
  int seed_rows_ev = -1;                 // the seeds' rows, when on a stream of their own
  std::vector<uint32_t> row_chunk;       // closure root -> its rows chunk
  std::vector<int> rows_ev;              // events of the rows chunks
  std::vector<Unit> narrow;              // cover classes that read leaf rows: after the leaves
};

// the part's leaves and cover roots, the rows it needs, their allocations
int wcover_rows(CoverPlan& d) {
  ospf_sweep* s = d.s;
  const Facts& f = d.f;
  const uint32_t V = d.V;
  for (uint32_t r : d.mine) (d.leaf[r] ? d.own_l : d.own_c).push_back(r);
  for (uint32_t r : d.own_c) (f.nbrs(r) <= 2048 ? d.c_der : d.c_wide).push_back(r);
  locality_order(d.own_l, [&](uint32_t v) { return f.first(v); });
  std::sort(d.own_c.begin(), d.own_c.end());
  d.nb_c = closure(f, d.c_der);
  std::vector<uint8_t> in_l(V, 0);
  for (uint32_t r : d.own_l) in_l[r] = 1;
  std::vector<uint32_t> extra_l;  // leaves the cover next hops read, not owned
  for (uint32_t v : d.nb_c)
    if (d.leaf[v] && !in_l[v]) extra_l.push_back(v);
  locality_order(extra_l, [&](uint32_t v) { return f.first(v); });
  d.need_l = d.own_l;
  d.need_l.insert(d.need_l.end(), extra_l.begin(), extra_l.end());
  d.cl = closure(f, d.need_l);
  std::vector<uint8_t> in_a(V, 0);
  for (uint32_t v : d.own_c) in_a[v] = 1;
  for (uint32_t v : d.cl)
    if (!d.leaf[v]) in_a[v] = 1;
  for (uint32_t v : d.nb_c)
    if (!d.leaf[v]) in_a[v] = 1;
  for (uint32_t v = 0; v < V; ++v)
    if (in_a[v]) d.cover_a.push_back(v);
  const uint32_t nA = d.nA = (uint32_t)d.cover_a.size(), nL = d.nL = (uint32_t)d.need_l.size();
  d.pos.assign(V, kNone);
  for (uint32_t i = 0; i < nA; ++i) d.pos[d.cover_a[i]] = i;
  for (uint32_t i = 0; i < nL; ++i) d.pos[d.need_l[i]] = nA + i;
  int rc;
  if ((rc = dalloc(s, &d.slab, (size_t)(nA + nL) * V)) || (rc = upload(s, &d.d_pos, d.pos)) ||
      (rc = upload(s, &d.d_a, d.cover_a)) || (rc = upload(s, &d.d_l, d.need_l)) ||
      (rc = dalloc(s, &d.lnh, (size_t)nL * V)))
    return rc;
  for (uint32_t r : d.need_l) d.kmax = std::max(d.kmax, f.nbrs(r));
  return OSPF_OK;
}

// (A) plan: cover rows by the closure when the cover splits into seeds and
// small components (the seeds' Dial, the closure's cover columns, then the
// full rows), else every row by the Dial. With one word count <= 4 over
// the closure roots, the closure also carries their next hops (masks of
// first hops per seed term): their next-hop rows then come out of the
// rows unit and no neighbour-row derivation runs for them.
void wcover_choose_closure(CoverPlan& d) {
  ospf_ctx* c = d.c;
  const Facts& f = d.f;
  const uint32_t V = d.V;
  d.closure = !c->cl_seed.empty() && !knob_flag(Knob::OSPF_COVER_NOCLOSURE);
  uint32_t NW = 0;
  if (d.closure) {
    const uint32_t nS = (uint32_t)c->h_ccv.size();
    std::vector<uint32_t> seed_row(nS, kNone);
    for (uint32_t j = 0; j < c->cl_seed.size(); ++j) {
      seed_row[c->cl_seed[j]] = j;
      d.seeds.push_back(c->h_ccv[c->cl_seed[j]]);
    }
    std::vector<uint8_t> is_seed(V, 0);
    for (uint32_t v : d.seeds) is_seed[v] = 1;
    for (uint32_t v : d.cover_a)
      if (!is_seed[v]) d.clos.push_back(v);
    const std::string err0 = c->err;  // a plan that does not apply is no error of the sweep
    NW = d.clos.empty() ? 0u : f.words(d.clos[0]);
    for (uint32_t r : d.clos)
      if (f.words(r) != NW) NW = 0;
    if (NW > ospf::kClMaxNW || knob_flag(Knob::OSPF_CLOSURE_NONH)) NW = 0;
    d.closure = d.clos.size() >= d.seeds.size() &&
                ospf_int::closure_build(c, d.clos, seed_row, d.ch, NW) == OSPF_OK;
    if (!d.closure && NW) {  // the masks do not apply: distances only
      NW = 0;
      d.closure = ospf_int::closure_build(c, d.clos, seed_row, d.ch, 0) == OSPF_OK;
    }
    if (!d.closure) {
      c->err = err0;
      NW = 0;
    }
  }
  d.NW = NW;
  d.cl_nh = d.closure && NW > 0;
  std::vector<uint8_t> nh_by_closure(V, 0);
  if (d.cl_nh)
    for (uint32_t r : d.clos) nh_by_closure[r] = 1;
  // the part's seeds (<= 64 next-hop words): next-hop masks during their
  // Dial, rows + digests after it (cover_spf_kernel seed mode)
  if (d.closure && !knob_flag(Knob::OSPF_SEED_NONH)) {
    std::vector<uint8_t> in_d(V, 0);
    for (uint32_t r : d.c_der) in_d[r] = 1;
    for (uint32_t r : d.seeds)
      if (in_d[r]) {
        d.sd_nh.push_back(r);
        d.NWs = std::max(d.NWs, f.words(r));
      }
    if (d.NWs > ospf::kSeedMaxNW) {
      d.sd_nh.clear();
      d.NWs = 0;
    }
    for (uint32_t r : d.sd_nh) nh_by_closure[r] = 1;
  }
  std::vector<uint32_t> keep;
  for (uint32_t r : d.c_der)
    if (!nh_by_closure[r]) keep.push_back(r);
  d.c_der.swap(keep);
}

// digests: cover classes (owned), then need_l (owned leaves first), then
// the closure roots (next hops by the closure), then the seeds
int wcover_digests(CoverPlan& d) {
  ospf_sweep* s = d.s;
  const uint32_t ncl_dig = d.cl_nh ? (uint32_t)d.clos.size() : 0u;
  const uint32_t nsn = (uint32_t)d.sd_nh.size();
  const uint32_t ndig = (uint32_t)(d.c_der.size() + d.c_wide.size() + d.nL) + ncl_dig + nsn;
  d.cl_dig0 = ndig - nsn - ncl_dig;
  d.sn_dig0 = ndig - nsn;
  const int rc = dalloc(s, &s->dig_all, ndig);
  if (rc) return rc;
  s->n_dig = ndig;
  s->n_rows = d.nA + d.nL;
  d.ev_a = new_event(s);
  return std::min(d.ev_a, 0);
}

// wide cover roots (> 2048 neighbours): their own batch, from the start
int wcover_wide_batch(CoverPlan& d) {
  if (d.c_wide.empty()) return OSPF_OK;
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const Facts& f = d.f;
  std::vector<uint32_t> roots = d.c_wide;
  locality_order(roots, [&](uint32_t v) { return f.first(v); });
  uint32_t W = 1, mx = 1;
  for (uint32_t r : roots) {
    W = std::max(W, f.words(r));
    mx = std::max(mx, f.nbrs(r));
  }
  const uint32_t n = (uint32_t)roots.size();
  ospf_digest* dg = s->dig_all + d.slot;
  uint32_t *d_roots, *dist, *nh;
  const int rc = class_rows(s, roots, W, d.slot, &d_roots, &dist, &nh);
  if (rc) return rc;
  Unit u = batch_unit(c, "cover_batch_w" + std::to_string(W), d_roots, n,
                      OSPF_WANT_DIST | OSPF_WANT_NH | OSPF_WANT_DIGEST, W, mx, dist, nh, dg,
                      (uint64_t)n * 4ull * d.V * (1 + W) + (uint64_t)n * scan_bytes(c, true));
  u.kernel = "ospf_run_batch_dev (" + std::to_string(W) + " next-hop words)";
  const int st = new_stream(s);
  if (st < 0) return st;
  u.stream = st;
  add_unit(s, std::move(u));
  return OSPF_OK;
}

// the closure path's device arrays; the closure roots and the part's seeds
// whose next hops it carries own their rows here
int wcover_closure_alloc(CoverPlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  ClosureDev& v = d.cd;
  const ospf_int::ClosureHost& ch = d.ch;
  const uint32_t V = d.V;
  const uint32_t nS = v.nS = (uint32_t)c->h_ccv.size(), nsd = v.nsd = (uint32_t)d.seeds.size();
  const uint32_t ncl = v.ncl = (uint32_t)d.clos.size(), nsn = v.nsn = (uint32_t)d.sd_nh.size();
  const uint32_t NW = v.NW = d.NW, NWs = v.NWs = d.NWs;
  v.KW = ch.KW;
  std::vector<uint32_t> seed_rp(nsd), clos_rp(ncl);
  for (uint32_t j = 0; j < nsd; ++j) seed_rp[j] = d.pos[d.seeds[j]];  // kNone: not a row here
  for (uint32_t j = 0; j < ncl; ++j) clos_rp[j] = d.pos[d.clos[j]];
  uint32_t *d_jl, *d_cst, *d_mem, *d_dloc, *d_out;
  uint2* d_comp;
  int rc;
  if ((rc = upload(s, &v.d_sd, d.seeds)) || (rc = upload(s, &v.d_srp, seed_rp)) ||
      (rc = upload(s, &v.d_cl, d.clos)) || (rc = upload(s, &v.d_crp, clos_rp)) ||
      (rc = dalloc(s, &v.seedC, (size_t)nsd * nS)) || (rc = dalloc(s, &v.dc, (size_t)ncl * nS)) ||
      (rc = upload(s, &d_comp, ch.comp)) || (rc = upload(s, &d_jl, ch.jl)) ||
      (rc = upload(s, &d_cst, ch.cst)) || (rc = upload(s, &d_mem, ch.mem)) ||
      (rc = upload(s, &d_dloc, ch.dloc)) || (rc = upload(s, &d_out, ch.out)))
    return rc;
  ospf::ClosurePlan& cp = v.cp;
  cp.ncomp = (uint32_t)ch.comp.size();
  cp.nS = nS;
  cp.chunks = (nS + 255u) / 256u;
  cp.comp = d_comp;
  cp.jl = d_jl;
  cp.cst = d_cst;
  cp.mem = d_mem;
  cp.dloc = d_dloc;
  cp.out = d_out;
  cp.seedC = v.seedC;
  cp.dc = v.dc;
  // next hops of the closure roots: masks in, the cover columns' masks out
  // of the closure, rows + digests out of the rows unit
  if (d.cl_nh) {
    uint32_t *d_fh = nullptr, *d_fhl = nullptr;
    if ((rc = upload(s, &d_fh, ch.fh)) || (rc = upload(s, &d_fhl, ch.fhloc)) ||
        (rc = dalloc(s, &v.dcm, (size_t)ncl * nS * NW)) || (rc = dalloc(s, &v.cnh, (size_t)ncl * V * NW)))
      return rc;
    cp.NW = NW;
    cp.fh = d_fh;
    cp.fhloc = d_fhl;
    cp.dcm = v.dcm;
    v.cdg = s->dig_all + d.cl_dig0;
    std::vector<uint8_t> mine_m(V, 0);
    for (uint32_t r : d.mine) mine_m[r] = 1;
    own_rows(s, d.clos, d.cl_dig0, d.slab, V, v.cnh, (size_t)V * NW, NW, &d.pos, &mine_m);
  }
  // next hops of the part's seeds out of their Dial
  v.seed_side = nsn && !knob_flag(Knob::OSPF_SEED_ROWS_INLINE);
  if (nsn) {
    std::vector<uint32_t> snp(nsd, kNone), at(V, kNone), srp2(nsn);
    for (uint32_t k = 0; k < nsn; ++k) {
      at[d.sd_nh[k]] = k;
      srp2[k] = d.pos[d.sd_nh[k]];
    }
    for (uint32_t j = 0; j < nsd; ++j) snp[j] = at[d.seeds[j]];
    if ((rc = upload(s, &v.d_snp, snp)) || (rc = dalloc(s, &v.snm, (size_t)nsn * nS * NWs)) ||
        (rc = dalloc(s, &v.snh, (size_t)nsn * V * NWs)) ||
        (v.seed_side && ((rc = dalloc(s, &v.sdf, (size_t)nsn * nS)) || (rc = upload(s, &v.d_sroots, d.sd_nh)) ||
                         (rc = upload(s, &v.d_srp2, srp2)))))
      return rc;
    v.sdg = s->dig_all + d.sn_dig0;
    own_rows(s, d.sd_nh, d.sn_dig0, d.slab, V, v.snh, (size_t)V * NWs, NWs, &d.pos);
  }
  return OSPF_OK;
}

// the seeds' Dial, their rows beside the closure, then the closure
int wcover_seed_units(CoverPlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const ClosureDev v = d.cd;
  const uint32_t V = d.V, nsn = v.nsn, NWs = v.NWs;
  uint32_t* const slab = d.slab;
  // the seeds' rows: counted once, by the unit that writes them
  const uint64_t rows_b = v.seed_side ? (uint64_t)nsn * 4ull * V * (1 + NWs) : 0;
  {
    Unit u;
    u.name = "cover_seeds";
    u.kernel = nsn ? "cover_spf_kernel (seeds' Dial, next-hop masks at settle; cover columns, "
                     "dist + next-hop rows, digests)"
                   : "cover_spf_kernel (contracted-graph Dial of the closure's seeds, LDS-resident "
                     "distances; their cover columns out)";
    u.stream = 0;
    u.n_roots = v.nsd;
    u.W = NWs;
    const uint64_t all_b = (uint64_t)v.nsd * 4ull * V + scan_bytes(c, true) +
                           (uint64_t)nsn * 4ull * NWs * (V + 2ull * v.nS);
    u.comp = all_b - rows_b;
    u.fn = [=](hipStream_t strm) {
      if (v.sdg && !v.seed_side &&
          ospf::zero_async(v.sdg, (size_t)nsn * sizeof(ospf_digest), strm) != hipSuccess)
        return ospf_int::fail(c, OSPF_E_DEVICE, "zero seed digests");
      ospf::CoverArgs a{};
      a.roots = v.d_sd;
      a.n = v.nsd;
      a.dist = slab;
      a.err = c->d_err;
      a.rowpos = v.d_srp;
      a.dcomp = v.seedC;
      if (nsn) {
        a.nhpos = v.d_snp;
        a.nhm = v.snm;
        a.nh = v.snh;
        a.NW = NWs;
        a.digest = v.sdg;
        a.dfull = v.sdf;  // null: rows inside this launch
      }
      const hipError_t e = ospf::launch_cover_spf(c->g, c->cover, a, (uint32_t)c->n_cu, strm);
      return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_cover_spf");
    };
    if (v.seed_side) {
      u.record = new_event(s);
      if (u.record < 0) return u.record;
    }
    add_unit(s, std::move(u), all_b);
  }
  if (v.seed_side) {  // the seeds' rows beside the closure
    const int ev_seeds = s->units.back().record;
    Unit u;
    u.name = "seed_rows";
    u.kernel = "seed_rows_kernel (the seeds' dist + next-hop rows and digests from their columns "
               "and masks)";
    const int st = new_stream(s);
    if (st < 0) return st;
    u.stream = st;
    u.wait = {ev_seeds};
    d.seed_rows_ev = new_event(s);
    if (d.seed_rows_ev < 0) return d.seed_rows_ev;
    u.record = d.seed_rows_ev;
    u.n_roots = nsn;
    u.W = NWs;
    u.comp = rows_b;
    u.fn = [=](hipStream_t strm) {
      if (v.sdg && ospf::zero_async(v.sdg, (size_t)nsn * sizeof(ospf_digest), strm) != hipSuccess)
        return ospf_int::fail(c, OSPF_E_DEVICE, "zero seed digests");
      const hipError_t e = ospf::launch_seed_rows(c->g, c->cover, v.d_sroots, nsn, v.sdf, v.snm, NWs, slab,
                                                  v.d_srp2, v.snh, v.sdg, c->d_err, (uint32_t)c->n_cu, strm);
      return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_seed_rows");
    };
    add_unit(s, std::move(u), 0);
  }
  Unit u;
  u.name = "cover_closure";
  u.kernel = d.cl_nh ? "closure_nh_kernel<" + std::to_string(v.NW) +
                           "> (cover columns + their next-hop masks of the components' roots "
                           "from the seeds' columns)"
                     : "closure_kernel<" + std::to_string(v.KW) +
                           "> (cover columns of the components' roots from the seeds' columns)";
  u.stream = 0;
  u.n_roots = v.ncl;
  u.comp = (uint64_t)v.ncl * 4ull * v.nS * (1 + v.NW);
  u.fn = [=](hipStream_t strm) {
    const hipError_t e = ospf::launch_closure(v.cp, v.KW, strm);
    return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_closure");
  };
  add_unit(s, std::move(u));
  return OSPF_OK;
}

// opt-in (OSPF_COVER_ROWS_TILED): with next hops, the rows by node tiles x
// root chunks (closure_tile_rows_kernel) instead of a node-order pass per
// root; exact, but measured 2x slower on the weighted F100k (35.3 vs
// 16.9 ms, a27 / a28). False (and nothing allocated) when it does not apply.
int wcover_tiled_rows(CoverPlan& d, ospf::ClosureRowsPlan& rp, bool& tiled) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const ClosureDev& v = d.cd;
  NodeTiles nt;
  tiled = node_tiles(c, nt) && !nt.tile.empty();
  if (!tiled) return OSPF_OK;
  std::vector<uint32_t> rcov(v.ncl);
  for (uint32_t j = 0; j < v.ncl; ++j) rcov[j] = c->h_cix[d.clos[j]];
  uint32_t *d_rcov, *d_tle, *d_tu;
  uint4* d_tile;
  int rc;
  if ((rc = upload(s, &d_rcov, rcov)) || (rc = upload(s, &d_tile, nt.tile)) ||
      (rc = upload(s, &d_tle, nt.le)) || (rc = upload(s, &d_tu, nt.u)))
    return rc;
  rp.nroots = v.ncl;
  rp.nS = v.nS;
  rp.NW = v.NW;
  rp.ntiles = (uint32_t)nt.tile.size();
  rp.roots = v.d_cl;
  rp.rcov = d_rcov;
  rp.rowpos = v.d_crp;
  rp.dc = v.dc;
  rp.dcm = v.dcm;
  rp.dist = d.slab;
  rp.nh = v.cnh;
  rp.digest = v.cdg;
  rp.tile = d_tile;
  rp.tle = d_tle;
  rp.tu = d_tu;
  return OSPF_OK;
}

// the closure roots' full rows from their cover columns
int wcover_rows_units(CoverPlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const ClosureDev v = d.cd;
  const uint32_t V = d.V, ncl = v.ncl, nS = v.nS, NW = v.NW;
  uint32_t* const slab = d.slab;
  // opt-in (OSPF_WCOVER_STAGE): the closure roots' rows in K chunks (in
  // closure order: a fabric's pods), each recording an event, so the leaf
  // rows of the chunks done run beside the next chunk. Measured slower on
  // the weighted F100k (58.5 vs 54.9 ms, a22): the bandwidth-bound leaf
  // launch takes the CUs the latency-bound rows launch needs.
  const uint32_t K = (d.nL && ncl >= 64 && knob_flag(Knob::OSPF_WCOVER_STAGE)) ? 4u : 1u;
  bool tiled = false;
  ospf::ClosureRowsPlan rp{};
  int rc;
  if (d.cl_nh && K == 1 && knob_flag(Knob::OSPF_COVER_ROWS_TILED) && (rc = wcover_tiled_rows(d, rp, tiled)))
    return rc;
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t lo = (uint32_t)((uint64_t)ncl * k / K), hi = (uint32_t)((uint64_t)ncl * (k + 1) / K);
    for (uint32_t j = lo; j < hi; ++j) d.row_chunk[d.clos[j]] = k;
    Unit u;
    u.name = K > 1 ? "cover_rows_s" + std::to_string(k) : std::string("cover_rows");
    u.kernel = tiled ? "closure_tile_rows_kernel (the closure roots' dist + next-hop rows and "
                       "digests by node tiles: cover columns given, leaves by their last hops)"
               : d.cl_nh ? "cover_rows_kernel (full dist + next-hop rows and digests of the closure's "
                           "roots: cover columns given, leaves by their last hop)"
                         : "cover_spf_kernel (full rows of the closure's roots: cover columns "
                           "given, leaves by their last hop)";
    u.stream = 0;
    if (k + 1 == K) {
      u.record = d.ev_a;
    } else {
      u.record = new_event(s);
      if (u.record < 0) return u.record;
    }
    d.rows_ev.push_back(u.record);
    u.n_roots = hi - lo;
    u.W = NW;
    u.comp = (uint64_t)(hi - lo) * 4ull * V * (1 + NW);
    u.fn = [=](hipStream_t strm) {
      if (hi == lo) return OSPF_OK;
      if (v.cdg && ospf::zero_async(v.cdg + lo, (size_t)(hi - lo) * sizeof(ospf_digest), strm) != hipSuccess)
        return ospf_int::fail(c, OSPF_E_DEVICE, "zero closure digests");
      if (tiled) {
        const hipError_t e = ospf::launch_closure_rows(c->g, c->cover, rp, strm);
        return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_closure_rows");
      }
      ospf::CoverArgs a{};
      a.roots = v.d_cl + lo;
      a.n = hi - lo;
      a.dist = slab;
      a.err = c->d_err;
      a.rowpos = v.d_crp + lo;
      a.dload = v.dc + (size_t)lo * nS;
      a.nhload = v.dcm ? v.dcm + (size_t)lo * nS * NW : nullptr;
      a.nh = v.cnh ? v.cnh + (size_t)lo * V * NW : nullptr;
      a.NW = NW;
      a.digest = v.cdg ? v.cdg + lo : nullptr;
      const hipError_t e = ospf::launch_cover_spf(c->g, c->cover, a, (uint32_t)c->n_cu, strm);
      return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_cover_spf");
    };
    add_unit(s, std::move(u));
  }
  return OSPF_OK;
}

// without the closure: every cover row by the Dial
void wcover_dial_unit(CoverPlan& d) {
  ospf_ctx* c = d.c;
  const uint32_t nA = d.nA;
  uint32_t *d_a = d.d_a, *slab = d.slab;
  Unit u;
  u.name = "cover_spf";
  u.kernel = "ospf_cover_dist_dev (cover_spf_kernel: contracted-graph Dial, LDS-resident "
             "distances)";
  u.stream = 0;
  u.record = d.ev_a;
  u.n_roots = nA;
  u.comp = (uint64_t)nA * 4ull * d.V + scan_bytes(c, true);
  u.fn = [=](hipStream_t strm) { return ospf_cover_dist_dev(c, d_a, nA, slab, strm); };
  add_unit(d.s, std::move(u));
}

// opt-in (OSPF_WNH_HUB, W <= 4): u runs wnh_hub_kernel when its plan applies
int wcover_hub_unit(CoverPlan& d, const std::vector<uint32_t>& roots, uint32_t W, uint32_t* nh,
                    ospf_digest* dg, Unit& u) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const uint32_t V = d.V;
  HubHost hh;
  const std::string err0 = c->err;
  if (hub_build(c, d.f, roots, W, d.pos, hh) != OSPF_OK) {
    c->err = err0;  // not applicable: the lanes / wide kernels run
    return OSPF_OK;
  }
  uint4* d_grp;
  uint32_t *d_hub, *d_loc, *d_ref, *d_wt, *d_ownl, *d_rid;
  int rc;
  if ((rc = upload(s, &d_grp, hh.grp)) || (rc = upload(s, &d_hub, hh.hub.empty() ? std::vector<uint32_t>{0u} : hh.hub)) ||
      (rc = upload(s, &d_loc, hh.loc)) || (rc = upload(s, &d_ref, hh.ref)) ||
      (rc = upload(s, &d_wt, hh.wt)) || (rc = upload(s, &d_ownl, hh.ownl)) ||
      (rc = upload(s, &d_rid, hh.rootid)))
    return rc;
  ospf::HubPlan hp{};
  hp.nhub = (uint32_t)hh.hub.size();
  hp.ngroups = (uint32_t)hh.grp.size();
  hp.tiles = (V + ospf::kHubTile - 1) / ospf::kHubTile;
  hp.tchunk = std::min<uint32_t>(8u, hp.tiles);
  // groups per block: <= 32 (512 roots), fewer while the grid is small
  hp.gchunk = 32u;
  while (hp.gchunk > 1u &&
         ((hp.ngroups + hp.gchunk - 1) / hp.gchunk) * ((hp.tiles + hp.tchunk - 1) / hp.tchunk) <
             8u * (uint32_t)c->n_cu)
    hp.gchunk /= 2u;
  hp.W = W;
  hp.nroots = (uint32_t)roots.size();
  hp.hub = d_hub;
  hp.grp = d_grp;
  hp.loc = d_loc;
  hp.ref = d_ref;
  hp.wt = d_wt;
  hp.ownl = d_ownl;
  hp.rootid = d_rid;
  hp.src = d.slab;
  hp.pitch = V;
  hp.nh = nh;
  hp.digest = dg;
  u.kernel = "wnh_hub_kernel<" + std::to_string(W) + "> (hub rows per tile in LDS, a group's "
             "rows per group, wave = root, lane = node)";
  u.fn = [=](hipStream_t strm) {
    const hipError_t e = ospf::launch_wnh_hub(c->g, hp, strm);
    return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_wnh_hub");
  };
  return OSPF_OK;
}

// opt-in (OSPF_WNH_RUNS, W > 4): u runs wnh_runs_kernel (runs of roots with
// one neighbour list) when its plan applies
int wcover_runs_unit(CoverPlan& d, const std::vector<uint32_t>& roots, uint32_t W, uint32_t* nh,
                     ospf_digest* dg, Unit& u) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const uint32_t V = d.V;
  WRunsHost wh;
  const std::string err1 = c->err;
  if (wruns_build(c, d.f, roots, W, d.pos, wh) != OSPF_OK) {
    c->err = err1;
    return OSPF_OK;
  }
  uint4* d_run;
  uint32_t *d_sl, *d_wt, *d_own, *d_rid;
  int rc;
  if ((rc = upload(s, &d_run, wh.run)) || (rc = upload(s, &d_sl, wh.slots)) ||
      (rc = upload(s, &d_wt, wh.wt)) || (rc = upload(s, &d_own, wh.own)) ||
      (rc = upload(s, &d_rid, wh.rootid)))
    return rc;
  ospf::WRunsPlan wp{};
  wp.nruns = (uint32_t)wh.run.size();
  wp.nroots = (uint32_t)roots.size();
  wp.W = W;
  wp.tiles = (V + ospf::kWrTile - 1) / ospf::kWrTile;
  wp.run = d_run;
  wp.slots = d_sl;
  wp.wt = d_wt;
  wp.own = d_own;
  wp.rootid = d_rid;
  wp.src = d.slab;
  wp.pitch = V;
  wp.nh = nh;
  wp.digest = dg;
  u.kernel = "wnh_runs_kernel (runs of roots with one neighbour list, lane = node, a wave "
             "per next-hop word)";
  u.fn = [=](hipStream_t strm) {
    const hipError_t e = ospf::launch_wnh_runs(c->g, wp, strm);
    return e == hipSuccess ? OSPF_OK : ospf_int::hip_fail(c, e, "launch_wnh_runs");
  };
  return OSPF_OK;
}

// (C) classes of cover roots by word count: next hops from their own and
// their neighbours' rows. Classes that read leaf rows queue behind the
// leaves (`narrow`), the others run beside them.
int wcover_class_units(CoverPlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const Facts& f = d.f;
  const uint32_t V = d.V;
  uint32_t *slab = d.slab, *d_pos = d.d_pos;
  int rc;
  for (uint32_t W : classes_by(d.c_der, [&](uint32_t r) { return f.words(r); })) {
    std::vector<uint32_t> roots;
    for (uint32_t r : d.c_der)
      if (f.words(r) == W) roots.push_back(r);
    locality_order(roots, [&](uint32_t v) { return f.last(v); });
    const uint32_t n = (uint32_t)roots.size();
    uint32_t *d_roots, *nh;
    if ((rc = upload(s, &d_roots, roots)) || (rc = dalloc(s, &nh, (size_t)n * V * W))) return rc;
    ospf_digest* dg = s->dig_all + d.slot;
    own_rows(s, roots, d.slot, slab, V, nh, (size_t)V * W, W, &d.pos);
    d.slot += n;
    Unit u;
    u.name = "wderive_wide_w" + std::to_string(W);
    u.kernel = std::string("ospf_wderive_wide_dev (") +
               (W <= 4 ? "wderive_wide_kernel<" + std::to_string(W) + ">"
                       : std::string("wderive_lanes_kernel")) + ")";
    u.n_roots = n;
    u.W = W;
    u.comp = (uint64_t)n * 4ull * V * W;
    // W > 4 (beside the leaves): 32-tile chunks, fewer blocks -- F100k-w step
    // 136 -> 126 ms though the launch alone takes 71 instead of 56 ms
    const uint32_t ct = W > 4 ? 32u : 0u;
    u.fn = [=](hipStream_t strm) {
      return ospf_int::wderive_wide(c, d_roots, n, 0, W, slab, V, d_pos, nh, dg, strm, ct);
    };
    if (W <= 4 && knob_flag(Knob::OSPF_WNH_HUB) && (rc = wcover_hub_unit(d, roots, W, nh, dg, u))) return rc;
    if (W > 4 && knob_flag(Knob::OSPF_WNH_RUNS) && (rc = wcover_runs_unit(d, roots, W, nh, dg, u))) return rc;
    bool reads_leaf = false;  // a neighbour's row comes from (B)
    for (uint32_t r : roots)
      for (uint32_t k = (*f.dn_off)[r]; k < (*f.dn_off)[r + 1] && !reads_leaf; ++k)
        reads_leaf = d.leaf[(*f.dn)[k]] != 0;
    if (W > 4 && !reads_leaf) {  // needs only the cover rows: beside the leaves
      const int st = new_stream(s);
      if (st < 0) return st;
      u.stream = st;
      u.wait = {d.ev_a};
      if (d.seed_rows_ev >= 0) u.wait.push_back(d.seed_rows_ev);  // may read a seed's row
      add_unit(s, std::move(u));
    } else {
      u.stream = 0;
      if (d.seed_rows_ev >= 0) u.wait.push_back(d.seed_rows_ev);
      d.narrow.push_back(std::move(u));
    }
  }
  return OSPF_OK;
}

// (B) with staged closure rows: leaf chunks beside the closure rows' chunks,
// then the narrow cover classes
int wcover_leaf_chunks(CoverPlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const Facts& f = d.f;
  const uint32_t V = d.V, nA = d.nA, nL = d.nL, kmax = d.kmax;
  uint32_t *slab = d.slab, *d_pos = d.d_pos;
  ospf_digest* dg = s->dig_all + d.slot;
  own_rows(s, d.own_l, d.slot, slab + (size_t)nA * V, V, d.lnh, V, 1);
  d.slot += nL;
  std::vector<uint8_t> is_sn(V, 0);
  for (uint32_t r : d.sd_nh) is_sn[r] = 1;
  const int lst = new_stream(s);
  if (lst < 0) return lst;
  const uint32_t KL = 4;
  int last = -1;
  for (uint32_t k = 0; k < KL; ++k) {
    const uint32_t lo = (uint32_t)((uint64_t)nL * k / KL), hi = (uint32_t)((uint64_t)nL * (k + 1) / KL);
    uint32_t dep = 0;
    bool seedn = false;
    for (uint32_t j = lo; j < hi; ++j)
      for (uint32_t e = (*f.dn_off)[d.need_l[j]]; e < (*f.dn_off)[d.need_l[j] + 1]; ++e) {
        const uint32_t x = (*f.dn)[e];
        if (d.row_chunk[x] != kNone) dep = std::max(dep, d.row_chunk[x]);
        else if (is_sn[x]) seedn = true;
      }
    Unit u;
    u.name = "wderive_s" + std::to_string(k);
    u.kernel = "ospf_wderive_dev (wderive_kernel: leaf rows from the cover rows, a chunk)";
    u.stream = lst;
    u.wait = {d.rows_ev[dep]};
    if (seedn && d.seed_rows_ev >= 0) u.wait.push_back(d.seed_rows_ev);
    u.record = new_event(s);
    if (u.record < 0) return u.record;
    last = u.record;
    u.n_roots = hi - lo;
    u.W = 1;
    u.comp = (uint64_t)(hi - lo) * 8ull * V;
    uint32_t* ldist = slab + (size_t)(nA + lo) * V;
    uint32_t* lnh_k = d.lnh + (size_t)lo * V;
    const uint32_t* d_lk = d.d_l + lo;
    ospf_digest* dgk = dg + lo;
    u.fn = [=](hipStream_t strm) {
      if (hi == lo) return OSPF_OK;
      return ospf_wderive_dev(c, d_lk, hi - lo, 0, kmax, slab, V, d_pos, ldist, lnh_k, dgk, strm);
    };
    add_unit(s, std::move(u));
  }
  for (auto& u : d.narrow) {
    u.wait.push_back(last);
    add_unit(s, std::move(u));
  }
  return OSPF_OK;
}

// (B) the leaves in one launch, then the narrow cover classes
void wcover_leaf_unit(CoverPlan& d) {
  ospf_sweep* s = d.s;
  ospf_ctx* c = d.c;
  const Facts& f = d.f;
  const uint32_t V = d.V, nA = d.nA, nL = d.nL, kmax = d.kmax;
  uint32_t *slab = d.slab, *d_pos = d.d_pos, *d_l = d.d_l, *lnh = d.lnh;
  ospf_digest* dg = s->dig_all + d.slot;
  own_rows(s, d.own_l, d.slot, slab + (size_t)nA * V, V, lnh, V, 1);
  d.slot += nL;
  Unit u;
  u.name = "wderive";
  u.kernel = "ospf_wderive_dev (wderive_kernel: leaf rows from the cover rows)";
  u.stream = 0;
  u.n_roots = nL;
  u.W = 1;
  u.comp = (uint64_t)nL * 8ull * V +
           (uint64_t)(d.cl.size() - std::min(d.cl.size(), (size_t)nL)) * 4ull * V;
  uint32_t* ldist = slab + (size_t)nA * V;
  if (d.seed_rows_ev >= 0) {  // a leaf next to a seed reads the seed's row
    std::vector<uint8_t> is_sn(V, 0);
    for (uint32_t r : d.sd_nh) is_sn[r] = 1;
    bool near = false;
    for (uint32_t r : d.need_l)
      for (uint32_t k = (*f.dn_off)[r]; k < (*f.dn_off)[r + 1] && !near; ++k) near = is_sn[(*f.dn)[k]] != 0;
    if (near) u.wait.push_back(d.seed_rows_ev);
  }
  u.fn = [=](hipStream_t strm) {
    if (!nL) return OSPF_OK;
    return ospf_wderive_dev(c, d_l, nL, 0, kmax, slab, V, d_pos, ldist, lnh, dg, strm);
  };
  add_unit(s, std::move(u));
  for (auto& x : d.narrow) add_unit(s, std::move(x));
}

}  // namespace

// WCOVER (spf_cover.hip + spf_wderive.hip): an independent set of leaves
// (<= 32 distinct neighbours; on a fabric the racks), the cover = the rest.
// (A) distance rows of the cover nodes the part needs by the contracted-graph
// SPF; (B) the leaves' dist + next-hop rows from their neighbours' rows;
// (C) next hops of cover roots (<= 2048 neighbours) from their own and their
// neighbours' rows, one launch per word count (> 4 words beside B). Cover
// roots beyond 2048 neighbours run their own batch from the start.
int ospf_int::sweep::plan_wcover(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                                 const std::vector<uint8_t>& leaf) {
  CoverPlan d(s, f, mine, leaf);
  ospf_ctx* c = s->c;
  int rc;
  if ((rc = wcover_rows(d))) return rc;
  wcover_choose_closure(d);
  if ((rc = wcover_digests(d)) || (rc = wcover_wide_batch(d))) return rc;
  // the Dial over the contracted cover graph: the seeds' rows (closure) or
  // every cover row
  s->trav_edges = (uint64_t)(d.closure ? d.seeds.size() : d.nA) * c->h_cedge.size();
  if (knob_flag(Knob::OSPF_SWEEP_DEBUG))
    fprintf(stderr, "plan_wcover: cover %u seeds %zu comps %zu closure roots %zu -> %s (%s)\n", d.nA,
            c->cl_seed.size(), c->cl_comp_off.size() - 1, d.clos.size(), d.closure ? "closure" : "dial",
            c->err.c_str());
  d.row_chunk.assign(d.V, kNone);
  if (d.closure) {
    if ((rc = wcover_closure_alloc(d)) || (rc = wcover_seed_units(d)) || (rc = wcover_rows_units(d)))
      return rc;
  } else {
    wcover_dial_unit(d);
  }
  if ((rc = wcover_class_units(d))) return rc;
  // (B) leaves, then the narrow cover classes (they read leaf rows)
  if (d.rows_ev.size() > 1 && d.nL) return wcover_leaf_chunks(d);
  wcover_leaf_unit(d);
  return OSPF_OK;
}

// WMULTI: the distance rows the part needs -- its non-leaf roots and every
// neighbour of its roots that is not one of its leaves -- from the multi-root
// traversal (spf_msdist.hip: groups of 32 roots adjacent in id order share a
// wavefront), then the leaves' rows derived from their neighbours' rows
// (ospf_wderive_dev), then the non-leaf roots' next hops from their own and
// their neighbours' rows (ospf_wderive_wide_dev). For large graphs where the
// cover does not fit the contracted-graph kernel (a mesh).
int ospf_int::sweep::plan_wmulti(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                                 const std::vector<uint8_t>& leaf) {
  ospf_ctx* c = s->c;
  const uint32_t V = s->V;
  const uint32_t hop = s->opts.flags & OSPF_HOP_COUNT;
  std::vector<uint8_t> own_m(V, 0), in_s(V, 0);
  std::vector<uint32_t> own_l, own_c;
  for (uint32_t r : mine) own_m[r] = 1;
  for (uint32_t r : mine) {
    (leaf[r] ? own_l : own_c).push_back(r);
    if (f.nbrs(r) > 2048) return fail(c, OSPF_E_RANGE, "wmulti: a root with > 2048 neighbours");
    if (!leaf[r]) in_s[r] = 1;
    for (uint32_t k = (*f.dn_off)[r]; k < (*f.dn_off)[r + 1]; ++k) {
      const uint32_t n = (*f.dn)[k];
      if (!(leaf[n] && own_m[n])) in_s[n] = 1;
    }
  }
  std::vector<uint32_t> srows;  // ascending ids: neighbours share a group
  for (uint32_t v = 0; v < V; ++v)
    if (in_s[v]) srows.push_back(v);
  const uint32_t nS = (uint32_t)srows.size(), nL = (uint32_t)own_l.size();
  std::vector<uint32_t> pos(V, kNone);
  for (uint32_t i = 0; i < nS; ++i) pos[srows[i]] = i;
  for (uint32_t j = 0; j < nL; ++j) pos[own_l[j]] = nS + j;
  // concurrent groups: two per CU, within a scratch budget (OSPF_MSD_MB, 64 GB)
  const uint32_t ngroups = (nS + 31u) / 32u;
  size_t budget = (size_t)knob_int(Knob::OSPF_MSD_MB) << 20;
  const size_t per = ospf::msdist_scratch_bytes(V, 1);
  uint32_t delta = hop ? 1u : std::max<uint32_t>(1, c->info.max_metric);
  delta = (uint32_t)knob_int(Knob::OSPF_MSD_DELTA, (int)delta);
  uint32_t *slab, *d_pos, *d_s, *d_l, *lnh, *scratch = nullptr;
  int rc;
  if ((rc = dalloc(s, &slab, (size_t)(nS + nL) * V)) || (rc = upload(s, &d_pos, pos)) ||
      (rc = upload(s, &d_s, srows.empty() ? std::vector<uint32_t>{0u} : srows)) ||
      (rc = upload(s, &d_l, own_l.empty() ? std::vector<uint32_t>{0u} : own_l)) ||
      (rc = dalloc(s, &lnh, (size_t)std::max(1u, nL) * V)))
    return rc;
  // the scratch also fits what the device has left (other parts' sweeps,
  // smaller devices), with a 1 GB margin; fewer blocks when an allocation
  // still fails
  // (destroyed sweeps' pooled blocks count as free: the allocation takes
  // from the pool or frees it)
  {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      fr += c->sweep_pool_bytes;
      budget = std::min<size_t>(budget, fr > (1ull << 30) ? fr - (1ull << 30) : per);
    }
  }
  uint32_t blocks = std::min<uint32_t>(std::max(1u, ngroups), 2u * (uint32_t)c->n_cu);
  blocks = std::max<uint32_t>(1, std::min<uint32_t>(blocks, (uint32_t)(budget / per)));
  blocks = std::min(blocks, (uint32_t)knob_int(Knob::OSPF_MSD_BLOCKS, (int)blocks));
  for (;;) {
    if (dalloc_try(s, &scratch, per * blocks / sizeof(uint32_t)) == OSPF_OK) break;
    if (blocks == 1) return sfail(s, OSPF_E_NOMEM, "wmulti: no room for one traversal's scratch");
    blocks = std::max(1u, blocks / 2);
  }
  const uint32_t ndig = (uint32_t)(own_c.size() + nL);
  if ((rc = dalloc(s, &s->dig_all, std::max(1u, ndig)))) return rc;
  s->n_dig = ndig;
  s->n_rows = nS + nL;
  s->trav_edges = (uint64_t)nS * c->info.n_edges;
  {
    ospf_sweep::Unit u;
    u.name = "msdist";
    u.kernel = "msdist_kernel (groups of 32 roots, [node][root] distances, label-correcting "
               "Delta-stepping)";
    u.stream = 0;
    u.n_roots = nS;
    u.comp = (uint64_t)nS * 4ull * V + (uint64_t)ngroups * scan_bytes(c, !hop);
    u.fn = [=](hipStream_t strm) {
      ospf::MsDistArgs a{};
      a.roots = d_s;
      a.n = nS;
      a.ngroups = ngroups;
      a.blocks = std::min(blocks, ngroups);
      a.delta = delta;
      a.hop = hop ? 1u : 0u;
      a.dist = slab;
      a.pitch = V;
      a.scratch = scratch;
      const bool dbg = knob_flag(Knob::OSPF_MSD_STATS);
      unsigned long long* st = nullptr;
      if (dbg && (hipMalloc(&st, 32) != hipSuccess || hipMemset(st, 0, 32) != hipSuccess))
        return ospf_int::fail(c, OSPF_E_DEVICE, "msdist stats");
      a.stats = st;
      const hipError_t e = ospf::launch_msdist(c->g, a, strm);
      if (e != hipSuccess) return ospf_int::hip_fail(c, e, "launch_msdist");
      if (dbg) {  // debug only (never inside a capture: OSPF_MSD_STATS runs eager sweeps)
        unsigned long long h[4];
        hipStreamSynchronize(strm);
        hipMemcpy(h, st, 32, hipMemcpyDeviceToHost);
        hipFree(st);
        fprintf(stderr, "msdist: %u rows, %u groups: phases %llu (%.1f per group), frontier "
                "nodes %llu (%.2f per node per group), candidates %llu (%.2f per node per group)\n",
                nS, ngroups, h[0], (double)h[0] / ngroups, h[1],
                (double)h[1] / ((double)ngroups * V), h[2], (double)h[2] / ((double)ngroups * V));
      }
      c->spf_runs += nS;
      return OSPF_OK;
    };
    add_unit(s, std::move(u));
  }
  uint32_t slot = 0;
  {  // leaves from their neighbours' rows
    ospf_digest* dg = s->dig_all + slot;
    own_rows(s, own_l, slot, slab + (size_t)nS * V, V, lnh, V, 1);
    slot += nL;
    uint32_t kmax = 1;
    for (uint32_t r : own_l) kmax = std::max(kmax, f.nbrs(r));
    ospf_sweep::Unit u;
    u.name = "wderive";
    u.kernel = "ospf_wderive_dev (wderive_kernel: leaf rows from neighbours' dist rows)";
    u.stream = 0;
    u.n_roots = nL;
    u.W = 1;
    u.comp = (uint64_t)nL * 8ull * V;
    uint32_t* ldist = slab + (size_t)nS * V;
    u.fn = [=](hipStream_t strm) {
      if (!nL) return OSPF_OK;
      return ospf_wderive_dev(c, d_l, nL, hop, kmax, slab, V, d_pos, ldist, lnh, dg, strm);
    };
    add_unit(s, std::move(u));
  }
  // next hops of the non-leaf roots
  for (uint32_t W : classes_by(own_c, [&](uint32_t r) { return f.words(r); })) {
    std::vector<uint32_t> roots;
    for (uint32_t r : own_c)
      if (f.words(r) == W) roots.push_back(r);
    const uint32_t n = (uint32_t)roots.size();
    uint32_t *d_roots, *nh;
    if ((rc = upload(s, &d_roots, roots)) || (rc = dalloc(s, &nh, (size_t)n * V * W))) return rc;
    ospf_digest* dg = s->dig_all + slot;
    own_rows(s, roots, slot, slab, V, nh, (size_t)V * W, W, &pos);
    slot += n;
    Unit u;
    u.name = "wderive_wide_w" + std::to_string(W);
    u.kernel = std::string("ospf_wderive_wide_dev (") +
               (W <= 4 ? "wderive_wide_kernel<" + std::to_string(W) + ">"
                       : std::string("wderive_lanes_kernel")) + ")";
    u.stream = 0;
    u.n_roots = n;
    u.W = W;
    u.comp = (uint64_t)n * 4ull * V * W;
    u.fn = [=](hipStream_t strm) {
      return ospf_int::wderive_wide(c, d_roots, n, hop, W, slab, V, d_pos, nh, dg, strm, 0);
    };
    add_unit(s, std::move(u));
  }
  return OSPF_OK;
}

// WDERIVE: cover roots (the part's non-leaves plus every neighbour of its
// leaves) on the per-root batch path, one launch per class on its own
// stream; then the leaves derived from those rows.
int ospf_int::sweep::plan_wderive(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                                  const std::vector<uint8_t>& leaf) {
  ospf_ctx* c = s->c;
  const uint32_t V = s->V;
  const uint32_t hop = s->opts.flags & OSPF_HOP_COUNT;
  std::vector<uint32_t> lr, cov;
  std::vector<uint8_t> own_m(V, 0);
  for (uint32_t r : mine) {
    own_m[r] = 1;
    if (leaf[r]) lr.push_back(r);
  }
  std::vector<uint8_t> in_c(V, 0);
  for (uint32_t r : mine)
    if (!leaf[r]) in_c[r] = 1;
  for (uint32_t v : closure(f, lr))
    if (!leaf[v]) in_c[v] = 1;
  for (uint32_t v = 0; v < V; ++v)
    if (in_c[v]) cov.push_back(v);
  locality_order(lr, [&](uint32_t v) { return f.first(v); });
  const uint32_t nC = (uint32_t)cov.size(), nl = (uint32_t)lr.size();
  uint32_t *cdist, *d_pos, *d_lr, *ldist, *lnh;
  int rc;
  if ((rc = dalloc(s, &cdist, (size_t)nC * V)) || (rc = upload(s, &d_lr, lr)) ||
      (rc = dalloc(s, &ldist, (size_t)nl * V)) || (rc = dalloc(s, &lnh, (size_t)nl * V)) ||
      (rc = dalloc(s, &s->dig_all, nC + nl)))
    return rc;
  s->n_dig = nC + nl;
  s->n_rows = nC + nl;
  s->trav_edges = (uint64_t)nC * c->info.n_edges;  // cover rows on the batch path
  std::vector<uint32_t> pos(V, kNone);
  uint32_t off = 0;
  const uint32_t flags = hop | OSPF_WANT_DIST | OSPF_WANT_NH | OSPF_WANT_DIGEST;
  std::vector<int> done;
  for (uint32_t cap : classes_by(cov, [&](uint32_t r) { return f.cap(r); })) {
    std::vector<uint32_t> roots;
    uint32_t mx = 1;
    for (uint32_t r : cov)
      if (f.cap(r) == cap) {
        roots.push_back(r);
        mx = std::max(mx, f.nbrs(r));
      }
    locality_order(roots, [&](uint32_t v) { return f.first(v); });
    const uint32_t n = (uint32_t)roots.size(), W = std::max(1u, (cap + 31) / 32);
    uint32_t *d_roots, *nh;
    if ((rc = upload(s, &d_roots, roots)) || (rc = dalloc(s, &nh, (size_t)n * V * W))) return rc;
    uint32_t* dist = cdist + (size_t)off * V;
    for (uint32_t j = 0; j < n; ++j) pos[roots[j]] = off + j;
    own_rows(s, roots, off, dist, V, nh, (size_t)V * W, W, nullptr, &own_m);
    Unit u;
    if ((rc = class_batch_unit(s, u, "cover_cap" + std::to_string(cap), d_roots, n, flags, W, mx, dist, nh,
                               s->dig_all + off, !hop)))
      return rc;
    off += n;
    u.record = new_event(s);
    if (u.record < 0) return u.record;
    done.push_back(u.record);
    add_unit(s, std::move(u));
  }
  if ((rc = upload(s, &d_pos, pos))) return rc;
  // owned leaves: digests after the cover rows
  own_rows(s, lr, nC, ldist, V, lnh, V, 1);
  uint32_t kmax = 1;
  for (uint32_t r : lr) kmax = std::max(kmax, f.nbrs(r));
  Unit u;
  u.name = "wderive";
  u.kernel = "ospf_wderive_dev (wderive_kernel: leaf rows from neighbours' dist rows)";
  u.stream = 0;
  u.wait = done;
  u.n_roots = nl;
  u.W = 1;
  u.comp = (uint64_t)nl * 8ull * V + (uint64_t)nC * 4ull * V;
  ospf_digest* dg = s->dig_all + nC;
  u.fn = [=](hipStream_t strm) {
    if (!nl) return OSPF_OK;
    return ospf_wderive_dev(c, d_lr, nl, hop, kmax, cdist, V, d_pos, ldist, lnh, dg, strm);
  };
  add_unit(s, std::move(u));
  return OSPF_OK;
}
