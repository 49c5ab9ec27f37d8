// sweep_units.hip — what the sweep planners share when they build launch
// units (sweep_impl.h, "units"), and the two planners that are little more:
// BATCH and LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sweep_impl.h"

using namespace ospf_int;
using namespace ospf_int::sweep;

void ospf_int::sweep::own_rows(ospf_sweep* s, const std::vector<uint32_t>& roots, uint32_t slot0,
                               const uint32_t* dist, size_t dist_pitch, const uint32_t* nh,
                               size_t nh_pitch, uint32_t W, const std::vector<uint32_t>* pos,
                               const std::vector<uint8_t>* only) {
  for (uint32_t j = 0; j < roots.size(); ++j) {
    const uint32_t r = roots[j];
    if (only && !(*only)[r]) continue;
    own(s, r, slot0 + j, dist + (size_t)(pos ? (*pos)[r] : j) * dist_pitch, nh + (size_t)j * nh_pitch, W);
  }
}

void ospf_int::sweep::add_unit(ospf_sweep* s, Unit&& u, uint64_t step_bytes) {
  s->step_comp += step_bytes;
  s->units.push_back(std::move(u));
}

Unit ospf_int::sweep::batch_unit(ospf_ctx* c, const std::string& name, const uint32_t* d_roots, uint32_t n,
                                 uint32_t flags, uint32_t W, uint32_t mx, uint32_t* dist, uint32_t* nh,
                                 ospf_digest* dg, uint64_t comp) {
  Unit u;
  u.name = name;
  u.wait = {0};
  u.n_roots = n;
  u.W = W;
  u.comp = comp;
  u.fn = [=](hipStream_t strm) {
    ospf_batch b{};
    b.d_roots = d_roots;
    b.n_roots = n;
    b.flags = flags;
    b.nh_words = W;
    b.max_root_neighbors = mx;
    b.d_dist = dist;
    b.d_nh = nh;
    b.d_digest = dg;
    return ospf_run_batch_dev(c, &b, strm);
  };
  return u;
}

int ospf_int::sweep::class_batch_unit(ospf_sweep* s, Unit& u, const std::string& name,
                                      const uint32_t* d_roots, uint32_t n, uint32_t flags, uint32_t W,
                                      uint32_t mx, uint32_t* dist, uint32_t* nh, ospf_digest* dg,
                                      bool weighted) {
  ospf_ctx* c = s->c;
  ospf_plan_info pi{};
  ospf_plan_n(c, flags, W, 0, n, mx, &pi);
  const uint64_t scans = pi.variant == 5 ? (uint64_t)((n + 63) / 64) * pi.slices : (uint64_t)n;
  u = batch_unit(c, name, d_roots, n, flags, W, mx, dist, nh, dg,
                 (uint64_t)n * 4ull * s->V * (1 + W) + scans * scan_bytes(c, weighted && pi.variant != 5));
  u.kernel = "ospf_run_batch_dev (variant " + std::to_string(pi.variant) + ", " + std::to_string(W) +
             " next-hop word" + (W > 1 ? "s)" : ")");
  const int st = new_stream(s);
  if (st < 0) return st;
  u.stream = st;
  return OSPF_OK;
}

namespace {

// the digests, rows and traversal count of a plan with one row per owned root
int one_row_per_root(ospf_sweep* s, const std::vector<uint32_t>& mine) {
  const int rc = dalloc(s, &s->dig_all, mine.size());
  if (rc) return rc;
  s->n_dig = (uint32_t)mine.size();
  s->n_rows = (uint32_t)mine.size();
  s->trav_edges = (uint64_t)mine.size() * s->c->info.n_edges;
  return OSPF_OK;
}

}  // namespace

int ospf_int::sweep::class_rows(ospf_sweep* s, const std::vector<uint32_t>& roots, uint32_t W,
                                uint32_t& slot, uint32_t** d_roots, uint32_t** dist, uint32_t** nh) {
  const size_t n = roots.size(), V = s->V;
  int rc;
  if ((rc = upload(s, d_roots, roots)) || (rc = dalloc(s, dist, n * V)) || (rc = dalloc(s, nh, n * V * W)))
    return rc;
  own_rows(s, roots, slot, *dist, V, *nh, V * W, W);
  slot += (uint32_t)n;
  return OSPF_OK;
}

// BATCH: one engine batch per width class of the part, each on its own
// stream from the run's start (ospf_run_batch_dev picks the kernel).
int ospf_int::sweep::plan_batch(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine,
                                bool weighted) {
  int rc;
  if ((rc = one_row_per_root(s, mine))) return rc;
  uint32_t slot = 0;
  const uint32_t flags = (s->opts.flags & OSPF_HOP_COUNT) | OSPF_WANT_DIST | OSPF_WANT_NH |
                         OSPF_WANT_DIGEST;
  for (uint32_t cap : classes_by(mine, [&](uint32_t r) { return f.cap(r); })) {
    std::vector<uint32_t> roots;
    uint32_t mx = 1;
    for (uint32_t r : mine)
      if (f.cap(r) == cap) {
        roots.push_back(r);
        mx = std::max(mx, f.nbrs(r));
      }
    locality_order(roots, [&](uint32_t v) { return f.first(v); });
    const uint32_t n = (uint32_t)roots.size(), W = std::max(1u, (cap + 31) / 32);
    ospf_digest* dg = s->dig_all + slot;
    uint32_t *d_roots, *dist, *nh;
    if ((rc = class_rows(s, roots, W, slot, &d_roots, &dist, &nh))) return rc;
    Unit u;
    if ((rc = class_batch_unit(s, u, "batch_cap" + std::to_string(cap), d_roots, n, flags, W, mx, dist, nh,
                               dg, weighted)))
      return rc;
    add_unit(s, std::move(u));
  }
  return OSPF_OK;
}

// LDS (spf_small.hip): small graphs, one launch per next-hop width (W <= 4)
// -- a wave per root with the graph in LDS; the widest class on the main
// stream, the others beside it.
int ospf_int::sweep::plan_lds(ospf_sweep* s, const Facts& f, const std::vector<uint32_t>& mine) {
  ospf_ctx* c = s->c;
  const uint32_t V = s->V;
  const uint32_t hop = s->opts.flags & OSPF_HOP_COUNT;
  const std::vector<uint32_t> ws = classes_by(mine, [&](uint32_t r) { return f.words(r); });
  int rc;
  if ((rc = one_row_per_root(s, mine))) return rc;
  uint32_t slot = 0;
  bool first = true;
  for (auto it = ws.rbegin(); it != ws.rend(); ++it) {
    const uint32_t W = *it;
    std::vector<uint32_t> roots;
    for (uint32_t r : mine)
      if (f.words(r) == W) roots.push_back(r);
    const uint32_t n = (uint32_t)roots.size();
    ospf_digest* dg = s->dig_all + slot;
    uint32_t *d_roots, *dist, *nh;
    if ((rc = class_rows(s, roots, W, slot, &d_roots, &dist, &nh))) return rc;
    Unit u;
    u.name = "lds_w" + std::to_string(W);
    u.kernel = "ospf_lds_sweep_dev (lds_sweep_kernel<" + std::to_string(W) +
               ">: a wave per root, graph + BFS state in LDS)";
    if (first) {
      u.stream = 0;
    } else {
      const int st = new_stream(s);
      if (st < 0) return st;
      u.stream = st;
      u.wait = {0};
    }
    first = false;
    u.n_roots = n;
    u.W = W;
    // rows written + the padded CSR each block copies in (read once from HBM)
    u.comp = (uint64_t)n * 4ull * V * (1 + W) + scan_bytes(c, false);
    u.fn = [=](hipStream_t strm) {
      return ospf_lds_sweep_dev(c, d_roots, n, hop, W, dist, nh, dg, strm);
    };
    add_unit(s, std::move(u));
  }
  return OSPF_OK;
}
