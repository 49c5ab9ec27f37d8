// spf_selstate.h — the select state and what its translation units share:
// spf_seldelta.hip (the resident selection, prime / update / copy) and
// spf_ucmp.hip (the UCMP weights resolved over it). Not a public header.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "spf_internal.h"

// ---------------------------------------------------------------- the state
struct ospf_selstate {
  ospf_ctx* c = nullptr;
  std::string err;
  uint32_t V = 0, P = 0;
  std::vector<uint32_t> t_off, t_nodes;  // the table's copy
  uint32_t* d_tab = nullptr;             // offsets, then nodes
  bool primed = false;
  int cur = 0;  // the committed buffer
  struct Buf {
    uint32_t* data = nullptr;  // the root blocks
    size_t data_words = 0;     // allocated
    uint64_t* off = nullptr;   // [V] block offset (words) by node id
    uint32_t* w = nullptr;     // [V] next-hop words by node id
    uint32_t* dn_off = nullptr;  // [V + 1]
    uint32_t* dn = nullptr;
    size_t dn_words = 0;  // allocated
    std::vector<uint64_t> h_off;
    std::vector<uint32_t> h_w;
  } b[2];
  uint32_t* d_roots = nullptr;  // [V]
  uint32_t* d_cnt = nullptr;    // [2]
  uint4* d_chg = nullptr;
  uint32_t* d_chg_nh = nullptr;
  uint32_t* d_reb = nullptr;
  size_t chg_cap = 0, chg_nh_words = 0, reb_cap = 0;
  uint64_t device_bytes = 0;
  // the committed selection: the context's graph version it was swept on,
  // whether under OSPF_HOP_COUNT, and the commits so far (prime / update)
  uint64_t gen = 0, serial = 0;
  bool hop = false;
  // the UCMP result resolved over it (spf_ucmp.hip; released with the state)
  struct ospf_ucmp* ucmp = nullptr;
  void (*release_ucmp)(ospf_selstate*) = nullptr;
};

namespace ospf_int {
namespace selst {

inline int stfail(ospf_selstate* st, int code, const std::string& m) {
  st->err = m;
  if (st->c) st->c->err = m;
  return code;
}

#define STCHK(st, call)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return ospf_int::selst::stfail(st, OSPF_E_DEVICE,                                    \
                                     std::string(#call) + ": " + hipGetErrorString(e_));   \
  } while (0)

inline void dfree(ospf_selstate* st, void* p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  st->device_bytes -= std::min<uint64_t>(st->device_bytes, bytes);
}

// *p grown to `count` elements (contents dropped); `have` = its capacity
template <class T>
int grow(ospf_selstate* st, T** p, size_t* have, size_t count) {
  count = std::max<size_t>(count, 1);
  if (*p && *have >= count) return OSPF_OK;
  dfree(st, *p, *have * sizeof(T));
  *p = nullptr;
  *have = 0;
  void* q = nullptr;
  if (dev_malloc(st->c, &q, count * sizeof(T)) != hipSuccess)
    return stfail(st, OSPF_E_NOMEM, "selstate: hipMalloc of " + std::to_string(count * sizeof(T)) + " B");
  *p = (T*)q;
  *have = count;
  st->device_bytes += count * sizeof(T);
  return OSPF_OK;
}

}  // namespace selst
}  // namespace ospf_int
