/*
 * openr_decision.h — C ABI of libopenr_decision, the host-side mirror of
 * OpenR's LinkState (openr/decision/LinkState.{h,cpp}) whose SPF runs on the
 * MI355X engine (include/openr_spf.h).
 *
 * The C++ class (openr_amd/csrc/decision/link_state.h, namespace odl) keeps
 * the reference's public surface and semantics:
 *   updateAdjacencyDatabase  LinkState.cpp:584-726 -> odl_apply (odl_apply_hold: TTLs)
 *   decrementHolds, hasHolds LinkState.cpp:520-548 -> odl_decrement_holds, odl_has_holds
 *   deleteAdjacencyDatabase  LinkState.cpp:728-746 -> odl_apply (db_delete=1)
 *   linksFromNode            LinkState.cpp:477-485 -> odl_links_text
 *   isNodeOverloaded         LinkState.cpp:515-518 -> odl_is_overloaded
 *   getSpfResult             LinkState.cpp:821-831 -> odl_spf_text
 *   getKthPaths              LinkState.cpp:790-819 -> odl_kth_paths_text
 *   getMetricFromAToB        LinkState.cpp:777-788 -> odl_metric_a_to_b
 *   decision.spf_runs        LinkState.cpp:843     -> odl_spf_runs
 *   resolveUcmpWeights       LinkState.cpp:913-1033 -> odl_ucmp_text
 * plus batched entry points the reference lacks (all-sources digests, KSP2
 * masked reruns for many destinations, per-neighbour reruns).
 *
 * This ABI exists for tests, benches and non-C++ callers; a C++ Decision
 * module links the class directly. Text results use the format documented
 * in DESIGN.md §Result text (same as the oracle's). Returned strings are
 * malloc'd; free them with odl_free(). NULL / negative return = error, see
 * odl_last_error().
 */
#ifndef OPENR_DECISION_H
#define OPENR_DECISION_H

#include <stdint.h>

#include "openr_adjdb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct odl_ls odl_ls;

/* New LinkState for `area` whose SPF engine runs on HIP device `device`. */
int odl_create(const char* area, int device, odl_ls** out);
/* Same over several devices of the node (device ids, may repeat): the graph
 * is replicated, all-sources sweeps run one root partition part per device. */
int odl_create_multi(const char* area, const int* devices, uint32_t n, odl_ls** out);
void odl_destroy(odl_ls* ls);
const char* odl_last_error(const odl_ls* ls);
void odl_free(char* p);

/* Apply stream records [first, first+count) in order; changes[count] out. */
int odl_apply(odl_ls* ls, const oadj_stream* s, uint32_t first, uint32_t count,
              oadj_change* changes);
/* Same with updateAdjacencyDatabase's hold TTLs (LinkState.cpp:585-700,
 * HoldableValue LinkState.cpp:48-117): a new link stays down for hold_up_ttl
 * odl_decrement_holds calls; a metric / overload change is held back
 * hold_up_ttl calls when it brings the link up (metric decrease, overload
 * cleared), hold_down_ttl otherwise. Decision itself passes 0
 * (Decision.cpp:756), which is odl_apply. */
int odl_apply_hold(odl_ls* ls, const oadj_stream* s, uint32_t first, uint32_t count,
                   oadj_change* changes, uint64_t hold_up_ttl, uint64_t hold_down_ttl);
/* LinkState::decrementHolds (LinkState.cpp:520-535): 1 when a hold expired
 * (topology changed, memoised results dropped), 0 when none did, < 0 error.
 * odl_has_holds (:537-548): 1 while any hold is on. */
int odl_decrement_holds(odl_ls* ls);
int odl_has_holds(const odl_ls* ls);

char* odl_spf_text(odl_ls* ls, const char* root, int use_link_metric);
char* odl_kth_paths_text(odl_ls* ls, const char* src, const char* dst, int k);
char* odl_links_text(odl_ls* ls, const char* node);
/* Keys of the snapshot's links in link id order (the ids of odl_csr_export
 * and of the engine's KSP2 records), one per line. */
char* odl_link_keys_text(odl_ls* ls);
int64_t odl_metric_a_to_b(odl_ls* ls, const char* a, const char* b, int use_link_metric);
int odl_is_overloaded(odl_ls* ls, const char* node);
uint64_t odl_spf_runs(const odl_ls* ls);
/* The path's fb303 counters: decision.spf_runs COUNT
 * (LinkState.cpp:843); decision.spf_ms (:909), ucmp_ms (:1029) and
 * route_build_ms (SpfSolver.cpp:640-644) are AVG stats, kept here as a sum
 * and a sample count; ucmp_runs COUNT (:926). Plus the device errors the
 * LinkState survived (it then runs on its host path; degraded = 1). */
typedef struct odl_counters {
  uint64_t spf_runs;
  uint64_t spf_ms_samples;
  double spf_ms_sum;
  uint64_t ucmp_runs;
  double ucmp_ms_sum;
  uint64_t route_build_runs;
  double route_build_ms_sum;
  uint64_t engine_errors;
  uint32_t engine_degraded;
} odl_counters;
void odl_get_counters(const odl_ls* ls, odl_counters* out);
/* The last engine error the LinkState degraded on ("" when none). */
const char* odl_last_engine_error(const odl_ls* ls);
/* Test hook: the after-th engine call from now fails with OSPF_E_DEVICE
 * (ospf_inject_error); the LinkState must degrade to its host path. */
int odl_inject_engine_error(odl_ls* ls, uint32_t after);
/* Degrade to the host path on device errors (default 1; 0: the call fails
 * with the engine's error instead). A LinkState whose engine never opened
 * (no device) always fails: there is no silent CPU path. ODL_STRICT_ENGINE
 * in the environment sets 0 at creation. */
void odl_set_degrade(odl_ls* ls, int on);
/* Incremental mode (off by default; odl::LinkState::setIncremental): keep the
 * memoised SPF of roots a metric / up / overload-only update cannot affect.
 * Stats: {patches applied, results kept, results dropped}. */
/* KvStore publications (the step before LinkState in Decision): compact-
 * thrift values decoded on host threads (adjdb_thrift.cpp).
 *
 * odl_apply_kvs -- Decision::processPublication's LinkState part
 * (Decision.cpp:846-870): keys[i] / values[i] (value_lens[i] bytes,
 * values[i] == NULL: a TTL-only update) in the caller's keyVals iteration
 * order; an "adj:" key's value (a CompactSerializer thrift::AdjacencyDatabase,
 * Types.thrift:175-207) goes to updateAdjacencyDatabase (updateKeyInLsdb
 * :743-765), other keys are skipped; then each expired "adj:" key deletes
 * the node getNodeNameFromKey names (deleteKeyFromLsdb :812-826). my_node !=
 * NULL applies filterUnuseableAdjacency (:568-600). changes: n + n_expired
 * records (zero for skipped keys) or NULL. */
int odl_apply_kvs(odl_ls* ls, uint32_t n, const char* const* keys, const uint8_t* const* values,
                  const uint64_t* value_lens, uint32_t n_expired, const char* const* expired,
                  const char* my_node, oadj_change* changes);
/* Same from a whole compact-thrift thrift::Publication (KvStore.thrift:270-
 * 320) in `buf`: keyVals in wire order, then expiredKeys. n_changes_out (may
 * be NULL) = number of records. When `changes` is not NULL and the records
 * do not fit max_changes, nothing is applied and ODL_E_SMALL is returned with
 * *n_changes_out set (call again with room for them). A publication whose
 * area field is set and differs from this LinkState's area is rejected
 * (Decision::processPublication picks the LinkState by the area,
 * Decision.cpp:847-854; the caller routes it). */
#define ODL_E_SMALL (-2)
int odl_apply_publication(odl_ls* ls, const uint8_t* buf, uint64_t len, const char* my_node,
                          oadj_change* changes, uint32_t max_changes, uint32_t* n_changes_out);
/* The last value odl_apply_kvs / odl_apply_publication could not decode
 * ("" when none; owned by ls) and the number of such values so far. */
const char* odl_last_decode_error(const odl_ls* ls, uint64_t* n_errors);
/* Decode n compact-thrift AdjacencyDatabase values into a columnar stream
 * (include/openr_adjdb.h; adj_only_used_by_other filled, db_delete all 0),
 * owned by *out until odl_adjdbs_free. NULL on malformed input, with the
 * reason in odl_adjdbs_error. */
typedef struct odl_adjdbs odl_adjdbs;
odl_adjdbs* odl_adjdbs_decode(const uint8_t* const* values, const uint64_t* lens, uint32_t n);
const oadj_stream* odl_adjdbs_stream(const odl_adjdbs* d);
const char* odl_adjdbs_error(void);
void odl_adjdbs_free(odl_adjdbs* d);
void odl_set_incremental(odl_ls* ls, int on);
/* Every SPF / KSP2 / digest of this LinkState on the host with the
 * reference's algorithm (LinkState.cpp:836-911), the engine never opened: a
 * GPU-free run of the ingest / in-place patch / memo logic (sanitizer builds;
 * also the environment variable ODL_HOST_SPF at creation). Not a fallback:
 * off by default, and nothing switches it on by itself. */
void odl_set_host_spf(odl_ls* ls, int on);
void odl_incremental_stats(const odl_ls* ls, uint64_t* out3);
/* {whole CSR snapshots, whole device graph loads, updates whose added /
 * removed links were patched in place (ospf_update_rows), rows rebuilt by
 * them}: a [LINK UP] / [LINK DOWN] between known nodes (LinkState.cpp:632-657)
 * takes no snapshot and no load. */
void odl_topology_stats(const odl_ls* ls, uint64_t* out4);
/* nodes added or removed in place (their rows inserted / erased and the ids
 * above them renumbered, no whole snapshot; the device graph reloads) */
uint64_t odl_node_patches(const odl_ls* ls);
/* multi-device LinkState (odl_create_multi): out4 = {root batches split
 * across the device slots, their per-slot launches, KSP2 prefetches split
 * across the slots (destinations of one source), their per-slot runs} */
void odl_shard_stats(const odl_ls* ls, uint64_t* out4);
uint32_t odl_num_nodes(const odl_ls* ls);
uint32_t odl_num_links(const odl_ls* ls);

/* Batched runs. roots / dsts are '\n'-separated node names.
 * odl_spf_digests: one engine batch, out[3*i] = {reached, sum_dist, hash}. */
int odl_spf_digests(odl_ls* ls, const char* roots_nl, uint32_t n, int use_link_metric,
                    uint64_t* out);
/* All-sources: runSpf for every node in one engine sweep (ospf_sweep_*, one
 * partition part per device), rows resident on the devices; getSpfResult of
 * any node then copies its rows (Decision::getDecisionRouteDb for every
 * node, Decision.cpp:309). odl_all_sources_digests: out[3 * id] for every
 * node id (odl_node_name order). A prefetch / route build asking for at
 * least 256 roots and half of the nodes takes the sweep by itself.
 * odl_sweep_stats: {sweeps, rows copied, mode (OSPF_SWEEP_*), devices,
 * hip graph}. */
int odl_all_sources_prefetch(odl_ls* ls, int use_link_metric);
int odl_all_sources_digests(odl_ls* ls, int use_link_metric, uint64_t* out);
void odl_sweep_stats(const odl_ls* ls, uint64_t* out5);
/* SpfSolver::getNextHopsWithMetric (SpfSolver.cpp:1043-1089) for every node
 * and every prefix of a table, selected on the device from the all-sources
 * sweep's resident rows (ospf_sweep_select / ospf_msweep_select; the host
 * path computes the same from getSpfResult of every node). prefixes_nl: one
 * prefix per line, its announcer node names tab-separated (an empty line: no
 * announcer); names unknown to the LinkState and duplicates are dropped.
 * Outputs by node id (odl_node_name order), any may be NULL:
 *   metric [V][n_prefixes]  smallest metric over the announcers the node
 *                           reaches, OSPF_DIST_INF when none;
 *   count  [V][n_prefixes]  announcers at that metric (0 when none);
 *   nh     [V][n_prefixes][nh_words]  union of their next hops, bit k = the
 *                           node's k-th distinct neighbour in ascending id order.
 * *nh_words_needed (optional) = the next-hop words of the widest node.
 * nh_words = 0 asks for that width only: nothing else is read or written.
 * nh_words below it fails (-1, odl_last_error). */
int odl_all_sources_select(odl_ls* ls, const char* prefixes_nl, uint32_t n_prefixes,
                           int use_link_metric, uint32_t nh_words, uint32_t* nh_words_needed,
                           uint32_t* metric, uint32_t* count, uint32_t* nh);
/* The same under the reference's route selection (createRouteForPrefix,
 * SpfSolver.cpp:197-458: unreached announcers dropped, the best
 * (path preference, source preference, distance) class kept, drained
 * announcers filtered unless all are, the route withheld below minNexthop;
 * LinkState::allSourcesSelect with attributes -> ospf_sweep_select_policy /
 * ospf_msweep_select_policy, or the same rule on the host path). prefixes_nl
 * as above; attrs holds four int64 per announcer name AS WRITTEN (n_attrs of
 * them in all, line after line, empty fields not counted): path preference,
 * source preference (the higher wins), distance (the lower wins) and
 * minNexthop (INT64_MIN = unset; clamped to [0, 2^32 - 1]). For a name given
 * twice the first occurrence counts; unknown names are dropped together with
 * their attributes. Outputs by node id, any may be NULL: metric / count / nh
 * as above over the selected announcers, and
 *   links     [V][n_prefixes]  next-hop links of the node's IP route;
 *   need      [V][n_prefixes]  the largest minNexthop of the filtered class;
 *   best      [V][n_prefixes]  bestNodeArea's node id, 0xFFFFFFFF when no
 *                              announcer is reached;
 *   installed [V][n_prefixes]  (bytes) 1 iff links > 0 and need <= links.
 * nh_words / *nh_words_needed as above. SR_MPLS per-destination next hops:
 * odl_all_sources_select_srmpls below. Not covered: KSP2 and per-area distance
 * selection, BGP metric vectors.
 * Several areas: odl_areas_select_policy. */
int odl_all_sources_select_policy(odl_ls* ls, const char* prefixes_nl, uint32_t n_prefixes,
                                  const int64_t* attrs, uint32_t n_attrs, int use_link_metric,
                                  uint32_t nh_words, uint32_t* nh_words_needed, uint32_t* metric,
                                  uint32_t* count, uint32_t* nh, uint32_t* links, uint32_t* need,
                                  uint32_t* best, uint8_t* installed);
/* The same for prefixes forwarded as SR_MPLS (LinkState::allSourcesSelectSrMpls
 * -> ospf_sweep_select_srmpls on one device, the same rule on the host path:
 * host mode, several devices, after a device error): the next hops are kept
 * per destination instead of ORed. Arguments as odl_all_sources_select_policy
 * with FIVE int64 per announcer name: the fifth is 1 when the entry has a
 * prepend label, else 0 (a node whose own entry has one routes to the other
 * announcers, SpfSolver.cpp:794-802). The kept entries of a prefix (unknown
 * names dropped, the first occurrence of a name, ascending by node id) are
 * indexed by entry_offsets [n_prefixes + 1]; A = entry_offsets[n_prefixes] is
 * at most the number of names given, so buffers sized for every name suffice.
 * Outputs by node id, any may be NULL: metric / count / links / need / best
 * [V][P], installed [V][P], dst_links [V][A] and dst_nh [V][A][nh_words] in
 * the kept-entry order. links counts (link, destination) pairs: the route's
 * nextHops.size() when the node labels are valid and distinct and a prepend
 * label is valid; the caller builds the PUSH stacks. nh_words 0 returns the
 * width only. Not covered: the resident selection and its delta, several
 * areas, KSP2, static MPLS next hops. */
int odl_all_sources_select_srmpls(odl_ls* ls, const char* prefixes_nl, uint32_t n_prefixes,
                                  const int64_t* attrs, uint32_t n_attrs, int use_link_metric,
                                  uint32_t nh_words, uint32_t* nh_words_needed,
                                  uint32_t* entry_offsets, uint32_t* metric, uint32_t* count,
                                  uint32_t* links, uint32_t* need, uint32_t* best,
                                  uint32_t* dst_links, uint32_t* dst_nh, uint8_t* installed);
/* The same selection across several areas, one LinkState each
 * (LinkState::allAreasSelect -> ospf_areas_select_policy over the areas'
 * resident sweeps, or the same steps on the host over each area's
 * getSpfResult when an area is in host mode, multi-device, on another device
 * or degraded, or when the engine call fails; a device error degrades every
 * area, any other refusal sends only this call to the host). A line of
 * prefixes_nl holds
 * tab-separated fields in pairs, node name then area name; attrs as above,
 * four int64 per pair. An unknown area is an error; a node unknown to its
 * area is dropped with its attributes. The areas are ordered by area name:
 * order[i] is the index into `areas` of the i-th by name, and nh_words[i],
 * nh[i] and bit i of `areas_mask` belong to it. The union of the node names,
 * by name bytes, gives the global ids. Need query, then fill: with
 * names_nl NULL the call only writes *n_global, order [n_areas] and nh_words
 * [n_areas]; otherwise *names_nl receives the global names, newline-separated
 * (odl_free), and the outputs that are not NULL are filled: metric / count /
 * links / need / best / areas_mask [G][n_prefixes] u32 by global id (best: the
 * entry's position among the kept entries of its prefix in (node, area)
 * order), installed [G][n_prefixes] bytes, nh[i] [V_i][n_prefixes]
 * [nh_words[i]] by that area's node id. *on_device: 1 when the device
 * answered. Errors (-1) are reported on areas[0]. The same selection kept
 * resident and its delta: odl_areas_track below. Not covered: UCMP across
 * areas, SR_MPLS per-destination next hops across areas (one area:
 * odl_all_sources_select_srmpls) and KSP2, BGP metric vectors, several
 * devices. */
int odl_areas_select_policy(odl_ls* const* areas, uint32_t n_areas, const char* prefixes_nl,
                            uint32_t n_prefixes, const int64_t* attrs, uint32_t n_attrs,
                            int use_link_metric, uint32_t* n_global, uint32_t* order,
                            uint32_t* nh_words, char** names_nl, uint32_t* metric, uint32_t* count,
                            uint32_t* links, uint32_t* need, uint32_t* best, uint32_t* areas_mask,
                            uint32_t* const* nh, uint8_t* installed, int* on_device);
/* odl_areas_select_policy's route DB kept resident, and only the cells an
 * event in some area or a change of the entries' attributes altered
 * (LinkState::AreasTracker over ospf_areastate_*; calculateUpdate across
 * areas). The tracker is bound to the given areas, which must outlive it, and
 * to one table (the lines and attributes of odl_areas_select_policy).
 *   odl_areas_delta     sweeps again every area whose version moved and returns
 *                       malloc'ed lists (odl_free_buf): 32-B records {root,
 *                       prefix, metric, count, links, need, best, areas} with
 *                       the NEW values by global id, nh [n_changes][sum of
 *                       nh_words] (area i's words one after the other, areas in
 *                       name order), the rebased global roots. nh_words
 *                       [n_areas]. *full: the node-name set of an area changed;
 *                       a new baseline was made and no lists are returned.
 *                       *on_device: 0 when the host path answered (an area in
 *                       host mode, multi-device or degraded, or an engine
 *                       error: the previous result is first copied off the
 *                       device, so the delta is still answered).
 *   odl_areas_tracked   the committed cells of some global nodes, in `nodes`
 *                       order: columns [n][prefixes], nh[i] [n][prefixes]
 *                       [nh_words[i]], zero where area i does not hold the
 *                       node. With every output but order / nh_words NULL it
 *                       only reports those two (what sizes nh).
 *   odl_areas_set_attrs new attributes for the same entries, four per entry in
 *                       table order; applied by the next odl_areas_delta.
 * Errors (-1) are reported on the first area given to odl_areas_track. */
typedef struct odl_areas_tracker odl_areas_tracker;
int odl_areas_track(odl_ls* const* areas, uint32_t n_areas, const char* prefixes_nl,
                    uint32_t n_prefixes, const int64_t* attrs, uint32_t n_attrs,
                    int use_link_metric, odl_areas_tracker** out);
int odl_areas_untrack(odl_areas_tracker* t);
int odl_areas_set_attrs(odl_areas_tracker* t, const int64_t* attrs, uint32_t n_attrs);
int odl_areas_delta(odl_areas_tracker* t, uint32_t* n_changes, uint32_t* n_rebased,
                    uint32_t* nh_words, int* full, int* on_device, void** changes, void** nh,
                    void** rebased);
int odl_areas_tracked(odl_areas_tracker* t, const char* nodes_nl, uint32_t n, uint32_t* order,
                      uint32_t* nh_words, uint32_t* metric, uint32_t* count, uint32_t* links,
                      uint32_t* need, uint32_t* best, uint32_t* areas_mask, uint32_t* const* nh,
                      uint8_t* installed);
/* Only the selections a topology change altered (LinkState::trackSelect /
 * selectDelta / selectTracked): DecisionRouteDb::calculateUpdate
 * (SpfSolver.cpp:24-59) for odl_all_sources_select's route DB.
 * odl_track_select binds the LinkState to a prefix table (prefixes_nl as
 * above) and stores the current snapshot's selection as the baseline, on the
 * device (ospf_selstate_*). odl_select_delta re-sweeps when the graph version
 * moved and returns the entries that differ from the baseline, then makes the
 * new selection the baseline:
 *   *changes  odl_select_change[*n_changes], the NEW values, order unspecified;
 *   *nh       uint32 [*n_changes][*nh_words], record i's next-hop words (bit k
 *             = the node's k-th distinct neighbour), zero-padded;
 *   *rebased  uint32 [*n_rebased] node ids whose distinct-neighbour list
 *             changed: none of their entries is listed (their bits mean other
 *             neighbours now) -- read them with odl_select_tracked;
 *   *full     1 when the node-name set changed since the last call (ids were
 *             renumbered): the baseline was taken again and no list is
 *             returned; read everything anew.
 * The three buffers are malloc'd (free each with odl_free_buf). A prefix that
 * lost its last reached announcer comes back with metric OSPF_DIST_INF and
 * count 0. odl_select_tracked copies the baseline of n nodes (names, one per
 * line) as odl_all_sources_select lays it out: metric / count [n][P], nh
 * [n][P][nh_words] (0 = the baseline's width; any output may be NULL). On the
 * host path (odl_set_host_spf, metrics outside the engine contract, after a
 * device error) and on a multi-device LinkState the previous selection is
 * kept on the host and diffed there: the same answers. */
typedef struct odl_select_change {
  uint32_t node, prefix, metric, count;
} odl_select_change;
int odl_track_select(odl_ls* ls, const char* prefixes_nl, uint32_t n_prefixes, int use_link_metric);
int odl_select_delta(odl_ls* ls, uint32_t* n_changes, uint32_t* n_rebased, uint32_t* nh_words,
                     int* full, void** changes, void** nh, void** rebased);
int odl_select_tracked(odl_ls* ls, const char* nodes_nl, uint32_t n, uint32_t nh_words,
                       uint32_t* metric, uint32_t* count, uint32_t* nh);
/* The same over the policy selection of odl_all_sources_select_policy
 * (LinkState::trackSelect with attributes / policyDelta / policyTracked /
 * setTrackedAttrs): what calculateUpdate diffs when best-route selection, a
 * drained node or minNexthop are in play. odl_track_select_policy takes the
 * prefix lines and attributes as odl_all_sources_select_policy does and stores
 * the policy selection as the baseline (on the device:
 * ospf_selstate_create_policy). odl_policy_delta is odl_select_delta with
 * odl_policy_change records: an entry changed when any of metric, count,
 * links, need, best or a next-hop word differs; installed = links > 0 && need
 * <= links. odl_policy_tracked copies the baseline of n nodes in
 * odl_all_sources_select_policy's layout (any output may be NULL).
 * odl_set_tracked_attrs replaces the attributes (n_attrs sets, parallel to the
 * tracked lines' names): nothing stored changes; the next odl_policy_delta
 * reports what the new attributes changed, with or without a topology event.
 * A table tracked with attributes refuses odl_select_delta /
 * odl_select_tracked, one tracked without refuses these calls (-1).
 * odl_all_sources_ucmp / odl_ucmp_tracked / odl_ucmp_host_loop on such a table
 * run over the policy selection. Host path and degraded behaviour as above. */
typedef struct odl_policy_change {
  uint32_t node, prefix, metric, count, links, need, best, installed;
} odl_policy_change;
int odl_track_select_policy(odl_ls* ls, const char* prefixes_nl, uint32_t n_prefixes,
                            const int64_t* attrs, uint32_t n_attrs, int use_link_metric);
int odl_policy_delta(odl_ls* ls, uint32_t* n_changes, uint32_t* n_rebased, uint32_t* nh_words,
                     int* full, void** changes, void** nh, void** rebased);
int odl_policy_tracked(odl_ls* ls, const char* nodes_nl, uint32_t n, uint32_t nh_words,
                       uint32_t* metric, uint32_t* count, uint32_t* nh, uint32_t* links,
                       uint32_t* need, uint32_t* best, uint8_t* installed);
int odl_set_tracked_attrs(odl_ls* ls, const int64_t* attrs, uint32_t n_attrs);
/* UCMP weights of every node for every prefix of the tracked table
 * (LinkState::allSourcesUcmp): SpfSolver::getNodeUcmpResult ->
 * resolveUcmpWeights (SpfSolver.cpp:1091-1161, LinkState.cpp:913-1033) for all
 * nodes at once, resolved on the device over the selection odl_track_select /
 * odl_select_delta keep resident (ospf_selstate_ucmp). algo 2 =
 * SP_UCMP_ADJ_WEIGHT_PROPAGATION, 3 = SP_UCMP_PREFIX_WEIGHT_PROPAGATION.
 * leaf_weights: one int64 >= 0 per announcer NAME of odl_track_select's lines,
 * in their order (n_weights of them; for a name given twice the first counts).
 * Outputs by node id: weight [V][P] (advertised; 0 unless OK) and status [V][P]
 * (0 OK, 1 no announcer reached, 2 a zero-weight announcer among the min-cost
 * ones: the reference returns nullopt, 3 a sum above 2^63 - 1 -- device only);
 * *rounds = the device's gather rounds, *on_device = 1 when the device
 * answered, *engine_ms = the engine call alone; any may be NULL. The tracked
 * selection must be the current topology's (odl_track_select or
 * odl_select_delta since the last change): -1 otherwise. On the host path
 * (odl_set_host_spf, metrics outside the engine contract, several devices,
 * after a device error with degrading on) the answer is the loop
 * resolveUcmpWeights(getSpfResult(node), min-cost announcers) per node and
 * prefix. odl_ucmp_tracked: the per-link view of n nodes (names, one per line)
 * from that result: weight / status [n][P], off [n * P + 1] and *wt (malloc'd,
 * *n_wt int64; odl_free_buf) -- entry (i, p)'s next-hop weights, one per
 * selected next hop in the node's distinct-neighbour order, divided by their
 * gcd; every tight link to that neighbour carries it. odl_ucmp_host_loop: the
 * host loop alone for n nodes, same outputs, nothing kept (cross-checks and
 * measurement). */
int odl_all_sources_ucmp(odl_ls* ls, int algo, const int64_t* leaf_weights, uint32_t n_weights,
                         int64_t* weight, uint8_t* status, uint32_t* rounds, int* on_device,
                         double* engine_ms);
int odl_ucmp_tracked(odl_ls* ls, const char* nodes_nl, uint32_t n, int64_t* weight, uint8_t* status,
                     uint64_t* off, void** wt, uint64_t* n_wt);
int odl_ucmp_host_loop(odl_ls* ls, int algo, const int64_t* leaf_weights, uint32_t n_weights,
                       const char* nodes_nl, uint32_t n, int64_t* weight, uint8_t* status,
                       uint64_t* off, void** wt, uint64_t* n_wt);
/* Fill the getSpfResult memo for many roots with one engine batch. */
int odl_spf_prefetch(odl_ls* ls, const char* roots_nl, uint32_t n, int use_link_metric);
/* getKthPaths(src, d, 2) for every d, masked reruns batched on the engine;
 * text = paths of each d, then a line "=". */
char* odl_ksp2_text(odl_ls* ls, const char* src, const char* dsts_nl, uint32_t n);

/* Route building over the GPU SPF results (SpfSolver consumers, SURVEY.md §8
 * a8-a10) for a prefix announced by `announcers` ('\n'-separated):
 *   algo 0 = SP_ECMP unicast (getNextHopsWithMetric + getNextHopsThrift,
 *            SpfSolver.cpp:1043-1285), 1 = KSP2_ED_ECMP (selectBestPathsKsp2,
 *            SpfSolver.cpp:847-973), 2 = MPLS node-label route of the single
 *            announcer (PHP / SWAP, SpfSolver.cpp:501-598).
 * Text: one next-hop per line, sorted: ifName \t neighbor \t metric \t
 * mpls-op (0 none, 1 PHP, 2 SWAP, 3 PUSH) \t labels (',' separated). */
char* odl_route_text(odl_ls* ls, const char* me, const char* announcers_nl, uint32_t n,
                     int algo);

/* LinkState::pathAInPathB (LinkState.h:477-492): 1 if path a (n links, keys
 * "n1%if1|n2%if2" one per line) occurs contiguously in path b, else 0; -1 on
 * a malformed key. */
int odl_path_a_in_b(const char* a_nl, uint32_t na, const char* b_nl, uint32_t nb);

/* SpfSolver::buildRouteDb (SpfSolver.cpp:460-646), one area, for each of the
 * n_mes nodes in mes_nl (their SPF results come from one batched engine
 * launch). prefixes_nl = n lines "prefix \t entry,entry,..." with
 * entry = "node:fwd:algo:weight[:prepend]" (a thrift::PrefixEntry: fwd 0 IP /
 * 1 SR_MPLS; algo 0 SP_ECMP, 1 KSP2_ED_ECMP, 2 SP_UCMP_ADJ_WEIGHT_PROPAGATION,
 * 3 SP_UCMP_PREFIX_WEIGHT_PROPAGATION; weight 0 = unset; optional prepend
 * label; then optionally "%pp/sp/d" = PrefixMetrics path_preference /
 * source_preference / distance, and "!bgp" or "!bgpmv" = PrefixType::BGP
 * without / with a metric vector). flags: 1 node-segment labels, 2 adjacency
 * labels, 4 UCMP, 8 enableBestRouteSelection (the SpfSolver constructor
 * switches, SpfSolver.h:108-118). Text, one line each, next hops sorted:
 *   me \t NONE                       (`me` unknown: the reference's nullopt)
 *   me \t R \t prefix \t igpCost(u32) \t ucmpWeight | -
 *        [flag 8: \t best node@area \t selected node@area,...]
 *   me \t U \t prefix \t ifName \t neighbor \t metric(i32) \t op \t labels \t weight
 *   me \t M \t label  \t ifName \t neighbor \t metric(i32) \t op \t labels \t weight
 * op: 0 none, 1 PHP, 2 SWAP, 3 PUSH, 4 POP_AND_LOOKUP; labels comma-separated
 * (SWAP: the swap label; PUSH: bottom of stack first). */
char* odl_route_db_text(odl_ls* ls, const char* mes_nl, uint32_t n_mes, const char* prefixes_nl,
                        uint32_t n, int flags);
/* Prefix entries may end in "@area" (the entry's area; default: the first
 * area by name) and then "#n" (PrefixEntry.minNexthop = n: addBestPaths
 * drops a route with fewer next hops, SpfSolver.cpp:976-1000,
 * getMinNextHopThreshold :694-710).
 * odl_route_db_multi_text: the same over several areas, one LinkState each
 * (their area names, odl_create's `area`, distinct): createRouteForPrefix's
 * per-area loop (SpfSolver.cpp:229-250, 360-442: entries reachable in their
 * own area; per area the forwarding type / algorithm of its best entries;
 * the next hops of the areas at the shortest IGP metric, UCMP weights
 * summed, KSP2 next hops added), node labels of every area's databases
 * (:490-598) and adjacency labels of every area (:603-631). Next-hop lines
 * carry a last field: the next hop's area. Errors: odl_last_error(areas[0]). */
char* odl_route_db_multi_text(odl_ls* const* areas, uint32_t n_areas, const char* mes_nl,
                              uint32_t n_mes, const char* prefixes_nl, uint32_t n, int flags);

/* odl_route_db_text's databases as one binary buffer (no text formatting or
 * parsing on either side; every string stored once). *out is malloc'd (free
 * with odl_free_buf), *bytes its size. Layout (little-endian, sections 8-B
 * aligned, offsets from the buffer start; string fields are offsets into the
 * NUL-terminated string section):
 *   odl_rdb_header; odl_rdb_node[n_nodes] (one per requested node, in order);
 *   odl_rdb_route[n_routes] (per node: unicast by prefix, then MPLS by label);
 *   odl_rdb_nh[n_nhs] (per route, sorted as in the text); int32 labels[];
 *   strings.
 * Replaces the text hop of Decision's route publication
 * (Decision::getDecisionRouteDb -> DecisionRouteDb, SpfSolver.h:80-98). */
#define ODL_RDB_MAGIC 0x4244524Fu /* "ORDB" */
typedef struct {
  uint32_t magic, version;
  uint64_t bytes;
  uint32_t n_nodes, n_routes, n_nhs, n_labels;
  uint64_t off_nodes, off_routes, off_nhs, off_labels, off_strings, str_bytes;
} odl_rdb_header;
typedef struct {
  uint32_t name;    /* string */
  uint32_t found;   /* 0: unknown node (the reference's nullopt) */
  uint32_t first_route, n_unicast, n_mpls, pad;
} odl_rdb_node;
typedef struct {
  uint32_t kind;        /* 0 unicast, 1 MPLS */
  uint32_t key;         /* unicast: prefix string; MPLS: the label */
  uint32_t igp_cost;    /* unicast */
  uint32_t has_weight;  /* unicast: ucmp_weight set */
  int64_t ucmp_weight;
  uint32_t first_nh, n_nh;
} odl_rdb_route;
typedef struct {
  uint32_t if_name, neighbor; /* strings */
  int32_t metric, weight;
  uint32_t op;                /* 0 none, 1 PHP, 2 SWAP, 3 PUSH, 4 POP_AND_LOOKUP */
  uint32_t first_label, n_labels, pad;
} odl_rdb_nh;
int odl_route_db_bin(odl_ls* ls, const char* mes_nl, uint32_t n_mes, const char* prefixes_nl,
                     uint32_t n, int flags, void** out, uint64_t* bytes);
void odl_free_buf(void* p);

/* LinkState::resolveUcmpWeights (LinkState.cpp:913-1033) over
 * getSpfResult(root): leaves_nl = n lines "name\tweight"; algo 2 =
 * SP_UCMP_ADJ_WEIGHT_PROPAGATION, 3 = SP_UCMP_PREFIX_WEIGHT_PROPAGATION.
 * Text: one line per node of the result, sorted by name:
 *   node \t advertised weight \t iface=nextHopNode:weight,... (sorted by iface) */
char* odl_ucmp_text(odl_ls* ls, const char* root, const char* leaves_nl, uint32_t n, int algo,
                    int use_link_metric);

/* CSR snapshot the engine sees (node ids = rank of name, byte order).
 * Copies into caller arrays sized by odl_csr_size(); any pointer may be NULL. */
int odl_csr_size(odl_ls* ls, uint32_t* n_nodes, uint32_t* n_edges);
int odl_csr_export(odl_ls* ls, uint32_t* row_ptr, uint32_t* col, uint32_t* metric,
                   uint32_t* link_id, uint32_t* twin, uint8_t* edge_up, uint8_t* no_transit,
                   uint32_t* link_rank);
/* Node name of id (pointer valid until the next apply). */
const char* odl_node_name(odl_ls* ls, uint32_t id);
int64_t odl_node_id(odl_ls* ls, const char* name);

#ifdef __cplusplus
}
#endif

#endif /* OPENR_DECISION_H */
