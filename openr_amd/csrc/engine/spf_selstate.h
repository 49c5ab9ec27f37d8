// spf_selstate.h — the select state and what its translation units share:
// spf_seldelta.hip (the resident selection, prime / update / copy),
// spf_seldelta_policy.hip (the same under the best-route policy) and
// spf_ucmp.hip (the UCMP weights resolved over either), and what
// spf_selareas.hip shares with the multi-area state of spf_seldelta_areas.hip.
// Not a public header.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "spf_internal.h"

struct ospf_sweep;

// ---------------------------------------------------------------- the state
struct ospf_selstate {
  ospf_ctx* c = nullptr;
  std::string err;
  uint32_t V = 0, P = 0;
  std::vector<uint32_t> t_off, t_nodes;  // the table's copy
  uint32_t* d_tab = nullptr;             // offsets, then nodes
  // a policy state (ospf_selstate_create_policy): an entry's header is metric,
  // count, links, need, best (hdr = 5) instead of metric, count (hdr = 2); the
  // table's policy columns, parallel to t_nodes (t_mnh empty: all unset)
  bool policy = false;
  uint32_t hdr = 2;
  std::vector<uint32_t> t_pref, t_mnh;
  uint32_t* d_pol = nullptr;  // pref, then min_nexthop
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
  uint4* d_chg = nullptr;  // change records: one uint4 each, two in a policy state
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

// `St`: ospf_selstate or ospf_areastate (c, err, device_bytes)
template <class St>
inline int stfail(St* st, int code, const std::string& m) {
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

template <class St>
inline void dfree(St* st, void* p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  st->device_bytes -= std::min<uint64_t>(st->device_bytes, bytes);
}

// *p grown to `count` elements (contents dropped); `have` = its capacity
template <class St, class T>
int grow(St* st, T** p, size_t* have, size_t count) {
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

// ---- spf_seldelta.hip
// a state over `t`; with `pol` (its offsets / nodes are t's) a policy state
int create(ospf_ctx* c, const ospf_select_table* t, const ospf_select_ptable* pol,
           ospf_selstate** out);
// sw's selection into the shadow buffer; with `compare` the entries that
// differ from the committed buffer's and the rebased roots are listed (up to
// the caps) and counted. Nothing is committed.
int write_shadow(ospf_selstate* st, ospf_sweep* sw, bool compare, uint32_t nh_words, bool want_nh,
                 uint32_t cap, uint32_t cap_reb, uint32_t counts[2]);
// what makes `sw` unusable for the state (null: usable)
const char* sweep_error(const ospf_selstate* st, const ospf_sweep* sw);
// the committed selection is sw's: what a consumer of the state checks it by
void committed(ospf_selstate* st, const ospf_sweep* sw);
// the widest owned root's next-hop words
uint32_t max_words(const ospf_sweep* sw);

// ---- spf_seldelta_policy.hip
// write_shadow's launch for a policy state (the buffers, lists and counters
// are in place): queued on the null stream, not waited for
int policy_delta_launch(ospf_selstate* st, ospf_sweep* sw, bool compare, uint32_t nh_words,
                        bool want_nh, uint32_t cap, uint32_t cap_reb);

// ---- spf_selareas.hip
// ospf_areas_select_policy's per-sweep rules for `s` beside area 0's sweep s0
// (null: they hold)
const char* areas_sweep_error(const ospf_sweep* s, const ospf_sweep* s0);
// the gid lists and the table of `t` against areas of Va[a] nodes (t->sweeps is
// not read): null when they hold, else what is wrong. Fills lid [A][G] (global
// -> node id) on the way.
const char* areas_table_error(const ospf_areas_table* t, const uint32_t* Va,
                              std::vector<uint32_t>& lid);
// every node's rows of a sweep that owns every root, by node id (s->d_area_rows)
int area_rows(ospf_sweep* s);

}  // namespace selst
}  // namespace ospf_int
