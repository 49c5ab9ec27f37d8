// spf_multi.hip — the multi-device context (include/openr_spf.h, "devices"):
// ospf_multi_* replicates the graph on several devices, ospf_msweep_* runs one
// part of the root partition per device slot (each an ospf_sweep, spf_sweep.hip)
// and gathers their digests on device 0, by RCCL or by peer copies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "sweep_impl.h"

using namespace ospf_int;
using namespace ospf_int::sweep;

namespace {

// a gathered digest to its root's slot of the by-node table (kNone: padding)
__global__ void scatter_digest_kernel(const ospf_digest* __restrict__ src,
                                      const uint32_t* __restrict__ roots, uint32_t n,
                                      ospf_digest* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && roots[i] != kNone) out[roots[i]] = src[i];
}

}  // namespace

// ---------------------------------------------------------------- devices
struct ospf_multi {
  std::vector<ospf_ctx*> ctx;
  std::string err;
  // RCCL communicators, one per device slot (ncclCommInitAll in this
  // process): the digest gather of a sweep is one ncclAllGather over xGMI.
  // 0 = not tried, 1 = live, -1 = unavailable (duplicate devices -- RCCL
  // takes one rank per GPU -- or init failed: peer copies instead)
  int rccl = 0;
  std::vector<ncclComm_t> comms;
};

struct ospf_msweep {
  ospf_multi* m = nullptr;
  std::vector<ospf_sweep*> parts;
  std::vector<uint32_t> owner;          // slot owning each node (kNone: none)
  uint32_t V = 0;
  ospf_digest* d_all = nullptr;         // device 0: [total owned] part digests, part order
  uint32_t* d_roots = nullptr;          // device 0: their root ids
  ospf_digest* d_by_node = nullptr;     // device 0: [V]
  std::vector<ospf_digest*> d_part;     // per slot (on its device): [slot] (padded)
  uint32_t total = 0;
  // RCCL gather: every part's digests padded to `slot` entries, all-gathered
  // into d_recv on every device; d_roots_pad (device 0) = the root of each
  // gathered entry (kNone: padding)
  uint32_t slot = 0;
  std::vector<ospf_digest*> d_recv;     // per slot (on its device): [n_parts * slot]
  uint32_t* d_roots_pad = nullptr;
};

namespace {
// RCCL communicators for the multi context, once: distinct devices only
// (OSPF_RCCL=1 also takes a single device -- a one-rank communicator, which
// exercises the path on a one-GPU box; OSPF_RCCL=0 keeps peer copies)
bool multi_rccl(ospf_multi* m) {
  if (m->rccl) return m->rccl > 0;
  m->rccl = -1;
  const char* e = knob_str(Knob::OSPF_RCCL);
  if (e && e[0] == '0') return false;
  const size_t n = m->ctx.size();
  std::vector<int> devs;
  for (ospf_ctx* c : m->ctx) devs.push_back(c->device);
  std::vector<int> u = devs;
  std::sort(u.begin(), u.end());
  if (std::unique(u.begin(), u.end()) != u.end()) return false;  // a device twice
  if (n < 2 && !(e && e[0] == '1')) return false;
  m->comms.assign(n, nullptr);
  if (ncclCommInitAll(m->comms.data(), (int)n, devs.data()) != ncclSuccess) {
    m->comms.clear();
    return false;
  }
  m->rccl = 1;
  return true;
}
}  // namespace

extern "C" {

int ospf_multi_open(const int* devices, uint32_t n, ospf_multi** out) {
  if (!devices || !n || !out) return OSPF_E_INVAL;
  *out = nullptr;
  ospf_multi* m = new (std::nothrow) ospf_multi();
  if (!m) return OSPF_E_NOMEM;
  for (uint32_t i = 0; i < n; ++i) {
    ospf_ctx* c = nullptr;
    const int rc = ospf_open(devices[i], &c);
    if (rc) {
      for (ospf_ctx* x : m->ctx) ospf_close(x);
      delete m;
      return rc;
    }
    m->ctx.push_back(c);
  }
  // peer access between distinct devices (xGMI); same-device slots need none
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j) {
      if (devices[i] == devices[j]) continue;
      int can = 0;
      hipDeviceCanAccessPeer(&can, devices[i], devices[j]);
      if (can) {
        hipSetDevice(devices[i]);
        hipDeviceEnablePeerAccess(devices[j], 0);
        (void)hipGetLastError();  // already enabled
      }
    }
  *out = m;
  return OSPF_OK;
}

int ospf_multi_close(ospf_multi* m) {
  if (!m) return OSPF_E_INVAL;
  for (ncclComm_t cm : m->comms)
    if (cm) ncclCommDestroy(cm);
  for (ospf_ctx* c : m->ctx) ospf_close(c);
  delete m;
  return OSPF_OK;
}

const char* ospf_multi_last_error(const ospf_multi* m) { return m ? m->err.c_str() : "null"; }

uint32_t ospf_multi_size(const ospf_multi* m) { return m ? (uint32_t)m->ctx.size() : 0u; }

ospf_ctx* ospf_multi_ctx(ospf_multi* m, uint32_t i) {
  return (m && i < m->ctx.size()) ? m->ctx[i] : nullptr;
}

int ospf_multi_load_graph(ospf_multi* m, const ospf_csr* csr, uint64_t version) {
  if (!m) return OSPF_E_INVAL;
  for (ospf_ctx* c : m->ctx) {
    const int rc = ospf_load_graph(c, csr, version);
    if (rc) {
      m->err = ospf_last_error(c);
      return rc;
    }
  }
  return OSPF_OK;
}

int ospf_msweep_destroy(ospf_msweep* ms) {
  if (!ms) return OSPF_E_INVAL;
  for (size_t i = 0; i < ms->parts.size(); ++i) {
    hipSetDevice(ms->m->ctx[i]->device);
    if (i < ms->d_part.size() && ms->d_part[i]) hipFree(ms->d_part[i]);
    if (i < ms->d_recv.size() && ms->d_recv[i]) hipFree(ms->d_recv[i]);
    ospf_sweep_destroy(ms->parts[i]);
  }
  if (!ms->m->ctx.empty()) hipSetDevice(ms->m->ctx[0]->device);
  if (ms->d_roots_pad) hipFree(ms->d_roots_pad);
  if (!ms->m->ctx.empty()) hipSetDevice(ms->m->ctx[0]->device);
  if (ms->d_all) hipFree(ms->d_all);
  if (ms->d_roots) hipFree(ms->d_roots);
  if (ms->d_by_node) hipFree(ms->d_by_node);
  delete ms;
  return OSPF_OK;
}

int ospf_msweep_create(ospf_multi* m, const ospf_sweep_opts* o, ospf_msweep** out) {
  if (!m || !o || !out || m->ctx.empty()) return OSPF_E_INVAL;
  *out = nullptr;
  ospf_msweep* ms = new (std::nothrow) ospf_msweep();
  if (!ms) return OSPF_E_NOMEM;
  ms->m = m;
  const uint32_t n = (uint32_t)m->ctx.size();
  auto bail = [&](int rc, const std::string& msg) {
    m->err = msg;
    ospf_msweep_destroy(ms);
    return rc;
  };
  ms->V = m->ctx[0]->info.n_nodes;
  ms->owner.assign(ms->V, kNone);
  std::vector<uint32_t> all_roots;
  for (uint32_t i = 0; i < n; ++i) {
    ospf_sweep_opts oi = *o;
    oi.part = i;
    oi.n_parts = n;
    // without HIP graphs no part runs at create: ospf_msweep_run starts every
    // device's first run together (a capture needs its part's eager run)
    if (!o->hip_graph) oi.flags |= OSPF_SWEEP_DEFER;
    ospf_sweep* s = nullptr;
    const int rc = ospf_sweep_create(m->ctx[i], &oi, &s);
    if (rc) return bail(rc, ospf_last_error(m->ctx[i]));
    ms->parts.push_back(s);
    for (uint32_t r : s->roots) ms->owner[r] = i;
    all_roots.insert(all_roots.end(), s->roots.begin(), s->roots.end());
    ms->slot = std::max<uint32_t>(ms->slot, (uint32_t)s->roots.size());
  }
  ms->slot = std::max(ms->slot, 1u);
  for (uint32_t i = 0; i < n; ++i) {  // digests padded to the widest part
    ospf_digest* dp = nullptr;
    hipSetDevice(m->ctx[i]->device);
    if (hipMalloc(&dp, (size_t)ms->slot * sizeof(ospf_digest)) != hipSuccess)
      return bail(OSPF_E_NOMEM, "msweep: hipMalloc");
    ms->d_part.push_back(dp);
    if (hipMemset(dp, 0, (size_t)ms->slot * sizeof(ospf_digest)) != hipSuccess)
      return bail(OSPF_E_DEVICE, "msweep: hipMemset");
  }
  if (multi_rccl(m)) {
    for (uint32_t i = 0; i < n; ++i) {
      ospf_digest* dr = nullptr;
      hipSetDevice(m->ctx[i]->device);
      if (hipMalloc(&dr, (size_t)n * ms->slot * sizeof(ospf_digest)) != hipSuccess)
        return bail(OSPF_E_NOMEM, "msweep: hipMalloc");
      ms->d_recv.push_back(dr);
    }
    std::vector<uint32_t> pad((size_t)n * ms->slot, kNone);
    for (uint32_t i = 0; i < n; ++i)
      std::copy(ms->parts[i]->roots.begin(), ms->parts[i]->roots.end(), pad.begin() + (size_t)i * ms->slot);
    hipSetDevice(m->ctx[0]->device);
    if (hipMalloc(&ms->d_roots_pad, pad.size() * 4) != hipSuccess ||
        hipMemcpy(ms->d_roots_pad, pad.data(), pad.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return bail(OSPF_E_NOMEM, "msweep: root table");
  }
  ms->total = (uint32_t)all_roots.size();
  hipSetDevice(m->ctx[0]->device);
  if (hipMalloc(&ms->d_all, std::max<size_t>(1, ms->total) * sizeof(ospf_digest)) != hipSuccess ||
      hipMalloc(&ms->d_roots, std::max<size_t>(1, ms->total) * 4) != hipSuccess ||
      hipMalloc(&ms->d_by_node, (size_t)ms->V * sizeof(ospf_digest)) != hipSuccess)
    return bail(OSPF_E_NOMEM, "msweep: hipMalloc");
  if (hipMemcpy(ms->d_roots, all_roots.data(), all_roots.size() * 4, hipMemcpyHostToDevice) !=
      hipSuccess)
    return bail(OSPF_E_DEVICE, "msweep: hipMemcpy");
  *out = ms;
  return OSPF_OK;
}

int ospf_msweep_run(ospf_msweep* ms) {
  if (!ms) return OSPF_E_INVAL;
  // queue every device's run first, then wait: the devices run concurrently
  for (size_t i = 0; i < ms->parts.size(); ++i) {
    const int rc = ospf_sweep_run(ms->parts[i], nullptr);
    if (rc) {
      ms->m->err = ospf_sweep_last_error(ms->parts[i]);
      return rc;
    }
  }
  for (size_t i = 0; i < ms->parts.size(); ++i) {
    const int rc = ospf_sync(ms->m->ctx[i], nullptr);
    if (rc) {
      ms->m->err = ospf_last_error(ms->m->ctx[i]);
      return rc;
    }
  }
  return OSPF_OK;
}

int ospf_msweep_digests(ospf_msweep* ms, ospf_digest* out) {
  if (!ms || !out) return OSPF_E_INVAL;
  ospf_ctx* c0 = ms->m->ctx[0];
  if (!ms->d_recv.empty()) {
    // every part's digests (queued on its device's stream), then ONE
    // ncclAllGather of the padded records; device 0 scatters them by root
    const size_t n = ms->parts.size();
    for (size_t i = 0; i < n; ++i) {
      const int rc = ospf_sweep_digests(ms->parts[i], ms->d_part[i], nullptr);
      if (rc) {
        ms->m->err = ms->parts[i]->err;
        return rc;
      }
    }
    ncclResult_t nr = ncclGroupStart();
    for (size_t i = 0; i < n && nr == ncclSuccess; ++i) {
      hipSetDevice(ms->m->ctx[i]->device);
      nr = ncclAllGather(ms->d_part[i], ms->d_recv[i], (size_t)ms->slot * 3, ncclUint64,
                         ms->m->comms[i], (hipStream_t)0);
    }
    const ncclResult_t ne = ncclGroupEnd();
    if (nr != ncclSuccess || ne != ncclSuccess) {
      ms->m->err = std::string("msweep: ncclAllGather: ") + ncclGetErrorString(nr != ncclSuccess ? nr : ne);
      return OSPF_E_DEVICE;
    }
    hipSetDevice(c0->device);
    hipMemset(ms->d_by_node, 0, (size_t)ms->V * sizeof(ospf_digest));
    const uint32_t tot = (uint32_t)(n * ms->slot);
    hipLaunchKernelGGL(scatter_digest_kernel, dim3((tot + 255) / 256), dim3(256), 0, 0,
                       ms->d_recv[0], ms->d_roots_pad, tot, ms->d_by_node);
    if (hipMemcpy(out, ms->d_by_node, (size_t)ms->V * sizeof(ospf_digest), hipMemcpyDeviceToHost) !=
        hipSuccess) {
      ms->m->err = "msweep: hipMemcpy";
      return OSPF_E_DEVICE;
    }
    return OSPF_OK;
  }
  size_t off = 0;
  for (size_t i = 0; i < ms->parts.size(); ++i) {
    ospf_sweep* s = ms->parts[i];
    const size_t n = s->roots.size();
    int rc = ospf_sweep_digests(s, ms->d_part[i], nullptr);
    if (rc) {
      ms->m->err = s->err;
      return rc;
    }
    hipSetDevice(ms->m->ctx[i]->device);
    if (hipDeviceSynchronize() != hipSuccess) return OSPF_E_DEVICE;
    if (n && hipMemcpyPeer(ms->d_all + off, c0->device, ms->d_part[i], ms->m->ctx[i]->device,
                           n * sizeof(ospf_digest)) != hipSuccess) {
      ms->m->err = "msweep: hipMemcpyPeer";
      return OSPF_E_DEVICE;
    }
    off += n;
  }
  hipSetDevice(c0->device);
  hipMemset(ms->d_by_node, 0, (size_t)ms->V * sizeof(ospf_digest));
  if (ms->total)
    hipLaunchKernelGGL(scatter_digest_kernel, dim3((ms->total + 255) / 256), dim3(256), 0, 0,
                       ms->d_all, ms->d_roots, ms->total, ms->d_by_node);
  if (hipMemcpy(out, ms->d_by_node, (size_t)ms->V * sizeof(ospf_digest), hipMemcpyDeviceToHost) !=
      hipSuccess) {
    ms->m->err = "msweep: hipMemcpy";
    return OSPF_E_DEVICE;
  }
  return OSPF_OK;
}

int ospf_msweep_select(ospf_msweep* ms, const ospf_select_table* t, uint32_t nh_words,
                       uint32_t* metric, uint32_t* count, uint32_t* nh) {
  if (!ms || !t) return OSPF_E_INVAL;
  const size_t n = ms->parts.size(), P = t->n_prefixes;
  auto part_fail = [&](size_t i, int rc) {
    ms->m->err = ms->parts[i]->err;
    return rc;
  };
  auto dev_fail = [&](const char* what) {
    (void)hipGetLastError();
    ms->m->err = std::string("msweep select: ") + what;
    return OSPF_E_DEVICE;
  };
  // every part queues its own roots' select on its device, then the copies
  std::vector<SelectOut> d(n);
  for (size_t i = 0; i < n; ++i) {
    ospf_sweep* s = ms->parts[i];
    if (ospf_int::injected(s->c)) return part_fail(i, sfail(s, OSPF_E_DEVICE, s->c->err));
    const size_t cells = s->roots.size() * P;
    if (cells && s->ran) {
      if (hipSetDevice(s->c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return dev_fail("hipDeviceSynchronize");
      if (!d[i].alloc(cells, std::max(1u, nh_words), metric, count, nh)) {
        (void)hipGetLastError();
        ms->m->err = "msweep select: hipMalloc of the outputs";
        return OSPF_E_NOMEM;
      }
    }
    const int rc = select_queue(s, t, nh_words, d[i].m, d[i].k, d[i].nh, nullptr);
    if (rc) return part_fail(i, rc);
  }
  std::vector<uint32_t> tmp;
  for (size_t i = 0; i < n; ++i) {
    ospf_sweep* s = ms->parts[i];
    const size_t cells = s->roots.size() * P;
    if (!cells) continue;
    if (hipSetDevice(s->c->device) != hipSuccess) return dev_fail("hipSetDevice");
    // owned-roots order -> node id order, `per` words per (root, prefix)
    auto by_node = [&](const uint32_t* dsrc, uint32_t* out, size_t per) {
      if (!dsrc) return true;
      tmp.resize(cells * per);
      if (hipMemcpy(tmp.data(), dsrc, tmp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
      for (size_t k = 0; k < s->roots.size(); ++k)
        std::copy(tmp.begin() + k * P * per, tmp.begin() + (k + 1) * P * per,
                  out + (size_t)s->roots[k] * P * per);
      return true;
    };
    if (!by_node(d[i].m, metric, 1) || !by_node(d[i].k, count, 1) ||
        !by_node(d[i].nh, nh, nh_words))
      return dev_fail("hipMemcpy");
  }
  return OSPF_OK;
}

int ospf_msweep_select_policy(ospf_msweep* ms, const ospf_select_ptable* t, uint32_t nh_words,
                              const ospf_select_pout* out) {
  if (!ms || !t || !out) return OSPF_E_INVAL;
  const size_t n = ms->parts.size(), P = t->n_prefixes;
  auto part_fail = [&](size_t i, int rc) {
    ms->m->err = ms->parts[i]->err;
    return rc;
  };
  auto dev_fail = [&](const char* what) {
    (void)hipGetLastError();
    ms->m->err = std::string("msweep select policy: ") + what;
    return OSPF_E_DEVICE;
  };
  // every part queues its own roots' select on its device, then the copies
  std::vector<PolicyOut> d(n);
  for (size_t i = 0; i < n; ++i) {
    ospf_sweep* s = ms->parts[i];
    if (ospf_int::injected(s->c)) return part_fail(i, sfail(s, OSPF_E_DEVICE, s->c->err));
    const size_t cells = s->roots.size() * P;
    if (cells && s->ran) {
      if (hipSetDevice(s->c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return dev_fail("hipDeviceSynchronize");
      if (!d[i].alloc(cells, std::max(1u, nh_words), out)) {
        (void)hipGetLastError();
        ms->m->err = "msweep select policy: hipMalloc of the outputs";
        return OSPF_E_NOMEM;
      }
    }
    const int rc = policy_queue(s, t, nh_words, &d[i].o, nullptr);
    if (rc) return part_fail(i, rc);
  }
  // the parts' outputs (owned-roots order) into host buffers of this call
  // first: a failed copy leaves the caller's as they were
  std::vector<std::vector<uint32_t>> tmp(n * 6);
  for (size_t i = 0; i < n; ++i) {
    ospf_sweep* s = ms->parts[i];
    const size_t cells = s->roots.size() * P;
    if (!cells) continue;
    if (hipSetDevice(s->c->device) != hipSuccess) return dev_fail("hipSetDevice");
    uint32_t* const src[6] = {d[i].o.metric, d[i].o.count, d[i].o.nh,
                              d[i].o.links,  d[i].o.need,  d[i].o.best};
    for (int k = 0; k < 6; ++k) {
      if (!src[k]) continue;
      auto& h = tmp[i * 6 + k];
      h.resize(cells * (k == 2 ? nh_words : 1u));
      if (hipMemcpy(h.data(), src[k], h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return dev_fail("hipMemcpy");
    }
  }
  uint32_t* const dst[6] = {out->metric, out->count, out->nh, out->links, out->need, out->best};
  for (size_t i = 0; i < n; ++i) {
    ospf_sweep* s = ms->parts[i];
    for (int k = 0; k < 6; ++k) {
      const auto& h = tmp[i * 6 + k];
      if (h.empty()) continue;
      const size_t per = P * (k == 2 ? nh_words : 1u);
      for (size_t j = 0; j < s->roots.size(); ++j)  // owned-roots order -> node id
        std::copy(h.begin() + j * per, h.begin() + (j + 1) * per, dst[k] + (size_t)s->roots[j] * per);
    }
  }
  return OSPF_OK;
}

ospf_sweep* ospf_msweep_part(ospf_msweep* ms, uint32_t slot) {
  return (ms && slot < ms->parts.size()) ? ms->parts[slot] : nullptr;
}

uint32_t ospf_msweep_gather_backend(const ospf_msweep* ms) {
  return (ms && !ms->d_recv.empty()) ? 1u : 0u;
}

int ospf_msweep_owner(const ospf_msweep* ms, uint32_t root, uint32_t* slot) {
  if (!ms || !slot || root >= ms->V) return OSPF_E_INVAL;
  if (ms->owner[root] == kNone) return OSPF_E_RANGE;
  *slot = ms->owner[root];
  return OSPF_OK;
}

}  // extern "C"
