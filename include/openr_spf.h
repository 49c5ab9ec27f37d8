/*
 * openr_spf.h — C ABI of libopenr_spf_hip, the MI355X batched SPF engine.
 *
 * Drop-in boundary for OpenR's Decision SPF hot path. The reference has no
 * FFI or plugin hook for SPF (openr/plugin/Plugin.h:19-42 is queue-level), so
 * the surface this ABI replaces is the body of one private C++ method:
 *
 *   LinkState::runSpf(src, useLinkMetric, linksToIgnore)
 *                                  openr/decision/LinkState.cpp:836-911
 *                                  (declared openr/decision/LinkState.h:518-525)
 *
 * batched over many roots, plus the graph those calls read
 * (linkMap_/allLinks_/nodeOverloads_, LinkState.h:538-549). The C++ caller (our
 * LinkState mirror, include/openr_decision.h, or the reference's own LinkState
 * after the patch in INTEGRATION.md) keeps the memo, SpfResult reconstruction
 * and route building; this library only computes, per root:
 *   dist[v]   u32, LinkState metric (UINT32_MAX = not reached)
 *   nh[v][w]  next-hop set of v as a bitset over the root's distinct
 *             neighbours in ascending node-id order (bit i = i-th neighbour)
 *   digest    {reached, sum dist, 64-bit hash} (definition: DESIGN.md §Digest)
 *
 * Semantics = the reference's runSpf: edges usable iff
 * Link::isUp (LinkState.cpp:242-245) and not ignored; weight = metric
 * advertised by the relaxing node (Link::getMetricFromNode, LinkState.cpp:193)
 * or 1 in hop-count mode; overloaded nodes other than the root never relax
 * (LinkState.cpp:859-866); nextHops(v) = union over tight transit predecessors
 * u of (u == root ? {v} : nextHops(u)) (LinkState.cpp:885-901).
 *
 * Conventions: every function returns OSPF_OK (0) or a negative OSPF_E_*
 * code; nothing throws or aborts across the ABI; ospf_last_error() explains
 * the last failure. One context per LinkState (area); a context is not
 * thread-safe (the reference calls SPF from the single Decision thread,
 * openr/Main.cpp:515-527). Out-of-contract inputs (metric 0, possible u32
 * distance overflow, > OSPF_MAX_ROOT_NEIGHBORS distinct root neighbours,
 * > OSPF_MAX_PARALLEL_LINKS entries from one node to one neighbour)
 * return OSPF_E_RANGE; there is no CPU fallback.
 */
#ifndef OPENR_SPF_H
#define OPENR_SPF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSPF_OK 0
#define OSPF_E_INVAL (-1)   /* bad argument */
#define OSPF_E_NOGRAPH (-2) /* no graph loaded */
#define OSPF_E_DEVICE (-3)  /* HIP runtime / device error */
#define OSPF_E_RANGE (-4)   /* input outside the engine's contract */
#define OSPF_E_NOMEM (-5)   /* device allocation failed */

#define OSPF_DIST_INF 0xFFFFFFFFu
#define OSPF_MAX_ROOT_NEIGHBORS 8192u /* nh words <= 256 */
/* The largest parallel group: CSR entries u -> v of one row towards one
 * neighbour, up or down (a down link may come up in place). ospf_load_graph
 * and ospf_update_rows refuse a larger one with OSPF_E_RANGE, so c(r, k) --
 * the links of a next hop k of root r, see `links` of ospf_sweep_select_policy
 * -- always fits the 16 bits the selection kernels keep per slot. */
#define OSPF_MAX_PARALLEL_LINKS 65535u
#define OSPF_MAX_IGNORED_PER_RUN 2048u

/* flags for ospf_sssp_batch* */
#define OSPF_HOP_COUNT 0x1u   /* useLinkMetric = false (LinkState.cpp:878) */
#define OSPF_WANT_DIST 0x2u
#define OSPF_WANT_NH 0x4u
#define OSPF_WANT_DIGEST 0x8u

typedef struct ospf_ctx ospf_ctx;

/* Link-state graph snapshot in CSR form (caller-owned, copied on load).
 * Node ids are 0..n_nodes-1; each row lists the directed edges u->col[e] of
 * node u sorted by col ascending (parallel links adjacent). Every undirected
 * link appears twice (once per endpoint); twin[e] is the other entry. */
typedef struct ospf_csr {
  uint32_t n_nodes;
  uint32_t n_edges;            /* directed entries = 2 x links */
  const uint32_t* row_ptr;     /* [n_nodes + 1] */
  const uint32_t* col;         /* [n_edges] neighbour id */
  const uint32_t* metric;      /* [n_edges] metric advertised by the row node, >= 1 */
  const uint32_t* link_id;     /* [n_edges] undirected link id (same for twins) */
  const uint32_t* twin;        /* [n_edges] index of the reverse entry */
  const uint8_t* edge_up;      /* [n_edges] Link::isUp() */
  const uint8_t* no_transit;   /* [n_nodes] LinkState::isNodeOverloaded() */
  /* optional (NULL = keep the given order of parallel entries): position of
   * the entry's link in linksFromNode(row node) iteration
   * (LinkState.cpp:477-485). The engine orders each parallel group of a row
   * by the rank of the twin entry, i.e. by the link's position in the
   * neighbour's linksFromNode, which is the pathLinks order
   * (LinkState.cpp:885-901) the KSP2 trace walks. */
  const uint32_t* link_rank;   /* [n_edges] */
} ospf_csr;

/* Per-run ignored links (LinkState::runSpf linksToIgnore). Run i ignores
 * link_ids[offsets[i] .. offsets[i+1]) (sorted ascending). */
typedef struct ospf_ignore {
  const uint32_t* offsets;  /* [n_roots + 1] */
  const uint32_t* link_ids;
} ospf_ignore;

typedef struct ospf_digest {
  uint64_t reached;
  uint64_t sum_dist;
  uint64_t hash;
} ospf_digest;

typedef struct ospf_graph_info {
  uint32_t n_nodes;
  uint32_t n_edges;
  uint32_t n_links;
  uint32_t max_degree;
  uint32_t max_metric;
  uint32_t unit_metric;        /* every usable edge has metric 1 */
  uint64_t version;
  uint64_t device_bytes;       /* resident graph bytes on the device */
} ospf_graph_info;

/* Open a context on HIP device `device` (ordinal). */
int ospf_open(int device, ospf_ctx** out);
int ospf_close(ospf_ctx* ctx);
const char* ospf_last_error(const ospf_ctx* ctx);

/* Upload (replace) the graph. `version` is the caller's topology version;
 * it is echoed by ospf_graph_info. */
int ospf_load_graph(ospf_ctx* ctx, const ospf_csr* csr, uint64_t version);
int ospf_graph_info_get(const ospf_ctx* ctx, ospf_graph_info* info);

/* Distinct neighbours of `root` in ascending id order = the nh bit order.
 * Writes min(n, cap) ids; *n = total. nh words for root = ceil(n / 32). */
int ospf_root_neighbors(const ospf_ctx* ctx, uint32_t root, uint32_t* ids,
                        uint32_t cap, uint32_t* n);

/* Batched SPF, host buffers, synchronous.
 *   roots[n_roots]; ignore may be NULL (no run ignores anything);
 *   dist_out: [n_roots][n_nodes] when OSPF_WANT_DIST;
 *   nh_out:   [n_roots][n_nodes][nh_words] when OSPF_WANT_NH; nh_words must be
 *             >= ceil(distinct neighbours / 32) of every root in the batch;
 *   digest_out: [n_roots] when OSPF_WANT_DIGEST. */
int ospf_sssp_batch(ospf_ctx* ctx, const uint32_t* roots, uint32_t n_roots,
                    const ospf_ignore* ignore, uint32_t flags, uint32_t nh_words,
                    uint32_t* dist_out, uint32_t* nh_out, ospf_digest* digest_out);

/* Same, device-resident: every pointer is device memory, the work is queued
 * on `stream` (hipStream_t, NULL = default stream) and NOT synchronised.
 * d_dist / d_nh may be NULL when not wanted (the engine then uses its own
 * scratch). d_ign_offsets / d_ign_ids may be NULL; otherwise max_ignored
 * bounds every run's ignore-list length. A run whose root has more than
 * 32 * nh_words distinct neighbours, or whose ignore list exceeds
 * max_ignored, raises the context's device error word: check it with
 * ospf_sync(). */
int ospf_sssp_batch_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n_roots,
                        const uint32_t* d_ign_offsets, const uint32_t* d_ign_ids,
                        uint32_t max_ignored, uint32_t flags, uint32_t nh_words,
                        uint32_t* d_dist, uint32_t* d_nh, ospf_digest* d_digest,
                        void* stream);

/* Device-resident batch with every option in one descriptor. Same contract
 * as ospf_sssp_batch_dev, plus a hint: max_root_neighbors >= the distinct
 * neighbour count of every root in the batch (0 = unknown, 32 * nh_words).
 * It sizes the multi-source BFS (next-hop passes and planes); a root above
 * it raises the device error word like a too-small nh_words. */
typedef struct ospf_batch {
  const uint32_t* d_roots;
  uint32_t n_roots;
  const uint32_t* d_ign_offsets; /* NULL = no run ignores links */
  const uint32_t* d_ign_ids;
  uint32_t max_ignored;
  uint32_t flags;
  uint32_t nh_words;
  uint32_t max_root_neighbors;
  uint32_t* d_dist;
  uint32_t* d_nh;
  ospf_digest* d_digest;
} ospf_batch;
int ospf_run_batch_dev(ospf_ctx* ctx, const ospf_batch* batch, void* stream);

/* Wait for `stream`, then report (and clear) the device error word:
 * OSPF_OK or OSPF_E_RANGE. */
int ospf_sync(ospf_ctx* ctx, void* stream);

/* All-sources next hops in two phases ("derive", unit metric or hop count).
 * ospf_levels_dev: distances of the n device roots by the distance-only
 * multi-source BFS, written as d_dist [n][V] u32 rows (optional), byte level
 * rows d_lev [n][lev_pitch] (dist + 1; 0x7F = unreached and padding;
 * lev_pitch a multiple of 16 >= V; needs a depth bound <= 123, else
 * OSPF_E_RANGE) and, optional, the distance
 * part {reached, sum dist, sum dist_key * (dist + 1)} of each run's digest.
 * ospf_nh_derive_dev: next-hop words [n][V][nh_words] (+ complete digests) of
 * the n device roots from level rows: d_lev_pos[v] = row of node v in d_lev
 * (0xFFFFFFFF: none), d_lev_digest = the level rows' digest parts (needed for
 * d_digest). Every distinct transit neighbour of every root with an up link
 * must have a row (else error bit 16 at ospf_sync); max_root_neighbors (0 =
 * 32 nh_words, at most 2048) bounds the roots' distinct neighbours. Bit k of a
 * root's word k / 32 = its k-th distinct neighbour n is a next hop towards v:
 * an up link, n transit or n == v, and dist(n, v) + 1 == dist(root, v) (the
 * reference's nextHops, LinkState.cpp:885-901). Both queue on `stream`. */
int ospf_levels_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t flags,
                    uint32_t* d_dist, uint8_t* d_lev, uint32_t lev_pitch,
                    ospf_digest* d_lev_digest, void* stream);
int ospf_nh_derive_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t nh_words,
                       uint32_t max_root_neighbors, const uint8_t* d_lev, uint32_t lev_pitch,
                       const uint32_t* d_lev_pos, const ospf_digest* d_lev_digest,
                       uint32_t* d_nh, ospf_digest* d_digest, void* stream);

/* Next hops (nh_words 1..4) from twin classes (spf_twin.hip), otherwise as
 * ospf_nh_derive_dev. Twins = nodes with the same usable distinct
 * neighbours and the same transit bit: their level rows agree except at the
 * members' own positions (dist(a, v) == dist(b, v) for v outside {a, b},
 * dist(a, b) == dist(b, a); LinkState.cpp:836-911 with unit weights), so a
 * root reads one row per class of its neighbours (a fabric switch: its
 * pod's racks, its plane's spines) instead of one per neighbour.
 * d_twin_class [V] = class of each node, d_twin_rep / d_twin_second
 * [classes] = its smallest member (whose level row is read) and another
 * member (0xFFFFFFFF for a class of one). A root whose usable transit
 * neighbours span more than 16 classes raises error bit 256. */
int ospf_nh_derive_twin_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t nh_words,
                            uint32_t max_root_neighbors, const uint8_t* d_lev,
                            uint32_t lev_pitch, const uint32_t* d_lev_pos,
                            const ospf_digest* d_lev_digest, const uint32_t* d_twin_class,
                            const uint32_t* d_twin_rep, const uint32_t* d_twin_second,
                            uint32_t* d_nh, ospf_digest* d_digest, void* stream);

/* Level + dist rows from twin classes, no traversal (spf_twin.hip; unit
 * metric or hop count, depth bound <= 123). For a root r whose usable transit
 * neighbours fall into <= 16 twin classes (d_twin_class / d_twin_rep as for
 * ospf_nh_derive_twin_dev), every class's representative having a level row
 * in d_lev at d_pos: dist(r, v) = 1 + min over the classes of the
 * representative's dist(rep, v), except 0 at r and 1 at every usable
 * neighbour -- Bellman's equation over r's out-links (LinkState.cpp:836-911,
 * overloaded neighbours reach only themselves, :859-866): twins' rows agree
 * outside their members, and every member of a neighbour class is a usable
 * neighbour of r. Writes r's level row (d_lev at d_pos[r]), its dist row
 * (d_dist + d_pos[r] * V; NULL = not wanted) and the distance part of its
 * digest (d_lev_digest[d_pos[r]], stored; NULL = not wanted). Error bits at
 * ospf_sync: 1 (> 128 distinct neighbours), 16 (a class row missing), 256
 * (> 16 classes, or > 16 distinct class rows in a group). d_groups
 * [n_groups + 1]: offsets into the roots, <= 8 roots per group, the roots of
 * a group reading <= 16 class rows together (each chunk's rows loaded once
 * for the group); NULL = one root per group. On a fabric the fabric
 * switches' rows come from one rack row of their pod and one spine row of
 * their plane (group = a pod's fabric switches). */
int ospf_twin_levels_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n,
                         const uint32_t* d_groups, uint32_t n_groups, uint8_t* d_lev,
                         uint32_t lev_pitch, const uint32_t* d_pos, const uint32_t* d_twin_class,
                         const uint32_t* d_twin_rep, uint32_t* d_dist, ospf_digest* d_lev_digest,
                         void* stream);

/* All-sources rows of leaf roots from level rows (unit metric or hop count;
 * spf_leaf.hip). A leaf r (no two leaves adjacent, <= 32 distinct
 * neighbours n_k) has dist(r, v) = 1 + min_k dist(n_k, v) over n_k with an
 * up link r-n_k (a non-transit n_k reaches only itself) and next hops = the
 * tight n_k -- LinkState::runSpf's Bellman equation over the root's
 * out-links (LinkState.cpp:836-911, :859-866, :885-901). Reads the level rows
 * of every usable transit neighbour (d_lev at d_pos[n], e.g. from
 * ospf_levels_dev) and writes the roots' own level rows and dist rows at
 * d_pos[root] (d_dist [rows][V], NULL = not wanted), one-word next-hop rows
 * d_nh [n][V] in root order and complete digests d_digest [n] (NULL = not
 * wanted). Groups: d_groups [n_groups + 1] offsets into the roots, <= 64
 * roots each, every root of a group with the same distinct neighbours and
 * usable links (the racks of a pod: a tile's neighbour rows are read once
 * per group; a group that is not uniform raises error bit 128); NULL = one
 * root per group. max_root_neighbors (0 = 32) bounds every root's distinct
 * neighbours. Needs a depth bound <= 123. Queued on `stream`. */
int ospf_leaf_derive_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n,
                         const uint32_t* d_groups, uint32_t n_groups, uint32_t max_root_neighbors,
                         uint8_t* d_lev, uint32_t lev_pitch, const uint32_t* d_pos,
                         uint32_t* d_dist, uint32_t* d_nh, ospf_digest* d_digest, void* stream);

/* Same, with d_lev_out [n] (device): the level row each root's level bytes
 * are written to, 0xFFFFFFFF = not kept (their dist and next-hop rows are
 * still written); NULL = d_pos[root] (ospf_leaf_derive_dev). A sweep keeps
 * only the rows its next-hop launches read: one per twin class. */
int ospf_leaf_derive2_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n,
                          const uint32_t* d_groups, uint32_t n_groups,
                          uint32_t max_root_neighbors, uint8_t* d_lev, uint32_t lev_pitch,
                          const uint32_t* d_pos, const uint32_t* d_lev_out, uint32_t* d_dist,
                          uint32_t* d_nh, ospf_digest* d_digest, void* stream);

/* All-sources rows of small graphs in one launch (spf_small.hip), unit
 * metric or OSPF_HOP_COUNT: a wave per root, the padded CSR and the root's
 * BFS state (visited bits, u16 levels, queue, next-hop words) in LDS --
 * LinkState::runSpf (LinkState.cpp:836-911) with unit weights, next hops as
 * :885-901 (the first hops of the shortest paths; overloaded nodes never
 * relay, :859-866). Writes d_dist [n][V], d_nh [n][V][nh_words] and
 * d_digest [n] (each NULL = not wanted); nh_words 1..4 must cover every
 * root's distinct neighbours (else error bit 1 at ospf_sync). flags may
 * carry OSPF_HOP_COUNT (the WANT bits are ignored: the buffers decide).
 * OSPF_E_RANGE when the graph is outside the kernel's contract (V > 65535,
 * or the CSR + one root's state does not fit in LDS): ospf_lds_sweep_fits
 * says beforehand. Queued on `stream`. Replaces the per-node
 * Decision::getDecisionRouteDb loop (Decision.cpp:309) for small areas. */
int ospf_lds_sweep_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t flags,
                       uint32_t nh_words, uint32_t* d_dist, uint32_t* d_nh,
                       ospf_digest* d_digest, void* stream);
int ospf_lds_sweep_fits(const ospf_ctx* ctx, uint32_t flags, uint32_t nh_words);

/* Weighted all-sources rows of leaf roots (any metric, or OSPF_HOP_COUNT; no
 * ignored links). For a root r with distinct neighbours n_k, w_k = the
 * smallest metric r advertises on an up link to n_k and D_k = the distance row
 * of n_k (d_src + d_pos[n_k] * src_pitch, computed by any engine path with the
 * same flags): dist(r, v) = min_k w_k + D_k(v) over transit n_k (an overloaded
 * n_k only reaches itself, at w_k), and bit k of next-hop word 0 of v is set
 * iff n_k's term is tight -- the reference's runSpf (LinkState.cpp:836-911:
 * Bellman's equation over the root's out-links; nextHops = the first hops of
 * the shortest paths, :885-901). Writes d_dist [n][V], d_nh [n][V] (one word
 * per node; NULL = not wanted) and d_digest [n] (NULL = not wanted). Every
 * root must have <= max_root_neighbors (1..32, 0 = 32) distinct neighbours,
 * each transit one with an up link needing a row (else error bits 1 / 16 at
 * ospf_sync). The caller derives an independent set of roots (no two
 * adjacent: the racks of a fabric) from the rows of the others. */
int ospf_wderive_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t flags,
                     uint32_t max_root_neighbors, const uint32_t* d_src, uint64_t src_pitch,
                     const uint32_t* d_pos, uint32_t* d_dist, uint32_t* d_nh,
                     ospf_digest* d_digest, void* stream);

/* Distance rows of cover roots on weighted graphs (the cover = the nodes
 * outside an independent set of leaves, e.g. the fabric and spine switches
 * when the racks are the leaves). ospf_cover_prepare builds the contracted
 * graph from the loaded graph: leaf_mask[V] (host) = 1 for leaves, no two of
 * them adjacent; cover nodes <= 32768, leaf in-link metrics <= 65535 (else
 * OSPF_E_RANGE). Shortest paths between cover nodes cross leaves only as
 * single-node detours through transit leaves, so the cover's distances are
 * those of the cover plus one shortcut edge per transit leaf detour, and a
 * leaf's distance is the minimum over its up in-links (LinkState.cpp:836-911
 * with metrics >= 1). ospf_cover_dist_dev writes d_dist [n][V] (link metrics;
 * no ignored links) for n cover roots (node ids; a leaf root raises error bit
 * 64). The prepared graph is tied to the graph version: prepare again after
 * ospf_load_graph / ospf_update_*. Next hops then come from ospf_wderive_dev
 * (leaves) and ospf_wderive_wide_dev (cover roots). */
int ospf_cover_prepare(ospf_ctx* ctx, const uint8_t* leaf_mask);
int ospf_cover_dist_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t* d_dist,
                        void* stream);

/* Next hops of roots with up to 128 distinct neighbours (nh_words 1..4), any
 * metric: every row -- the roots' own and their transit neighbours' -- is in
 * d_src at d_pos[] (computed with the same flags: ospf_cover_dist_dev for the
 * cover, ospf_wderive_dev for the leaves); bit k of v is set iff w_k + D_k(v)
 * == D_root(v) with n_k transit, or v == n_k and w_k == D_root(v) (the first
 * hops of the shortest paths, LinkState.cpp:885-901). Writes d_nh
 * [n][V][nh_words] and the complete digests (dist part from the own row). */
int ospf_wderive_wide_dev(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t flags,
                          uint32_t nh_words, const uint32_t* d_src, uint64_t src_pitch,
                          const uint32_t* d_pos, uint32_t* d_nh, ospf_digest* d_digest,
                          void* stream);

/* Kernel variant the engine would use for a large batch (for reporting):
 * 0 = Dial, LDS-resident (dist+nh in LDS), 1 = Dial, LDS dist + HBM
 * next-hops, 2 = Dial, HBM state, 3 = per-root BFS with LDS bitmaps and LDS
 * byte next-hops, 4 = per-root BFS with HBM next-hops, 5 = multi-source
 * bit-parallel BFS (64 roots per traversal; unit metric, no ignored links). */
int ospf_plan_variant(const ospf_ctx* ctx, uint32_t flags, uint32_t nh_words,
                      int* variant);

/* Full launch plan the engine would use for a batch (reporting / profiling). */
typedef struct ospf_plan_info {
  int32_t variant;       /* as ospf_plan_variant */
  uint32_t block;        /* threads per workgroup */
  uint32_t lds_bytes;    /* dynamic LDS per workgroup */
  uint32_t slices;       /* workgroups per SPF run (next-hop slices); variant 5:
                            passes per 64-root batch */
} ospf_plan_info;
int ospf_plan(const ospf_ctx* ctx, uint32_t flags, uint32_t nh_words, uint32_t max_ignored,
              ospf_plan_info* out);
/* Same for a batch of n_roots roots with the given neighbour hint (variant 5:
 * slices = next-hop passes per 64-root batch). */
int ospf_plan_n(const ospf_ctx* ctx, uint32_t flags, uint32_t nh_words, uint32_t max_ignored,
                uint32_t n_roots, uint32_t max_root_neighbors, ospf_plan_info* out);

/* KSP2 edge-disjoint paths (LinkState::getKthPaths k = 1 and k = 2,
 * LinkState.cpp:790-819, with traceOnePath :418-439) from one source to many
 * destinations, computed on the device: the link-metric SPF of src; per
 * destination the greedy edge-disjoint trace over its pathLinks (k = 1);
 * the masked SPF rerun that ignores every link of the k = 1 paths and the
 * trace over it (k = 2). Records (u32, per destination and k, path_cap words):
 *   n_paths, then per path: len, link ids (ospf_csr link_id) from src to dst.
 * status[i] bits: OSPF_KSP_RERUN = destination i's k = 2 needed a masked SPF
 * (its k = 1 paths are not empty, LinkState.cpp:802-806); OSPF_KSP_OVF1 /
 * OSPF_KSP_OVF2 = the k = 1 / k = 2 record was not computed (record or trace
 * budget exceeded: path_cap, 256 links deep, 1536 links visited); the caller
 * computes those destinations itself. src == dst and unreached destinations
 * give empty records (no paths). The graph must be loaded with link_rank for
 * the reference's parallel-link order. */
#define OSPF_KSP_RERUN 0x1u
#define OSPF_KSP_OVF1 0x2u
#define OSPF_KSP_OVF2 0x4u
typedef struct ospf_ksp2 {
  uint32_t src;
  const uint32_t* dsts;  /* [n] node ids */
  uint32_t n;
  uint32_t path_cap;     /* words per record, 2 .. OSPF_MAX_IGNORED_PER_RUN */
  uint32_t* k1;          /* [n][path_cap] */
  uint32_t* k2;          /* [n][path_cap] */
  uint32_t* status;      /* [n] */
} ospf_ksp2;
/* host buffers, synchronous */
int ospf_ksp2_run(ospf_ctx* ctx, const ospf_ksp2* args);
/* device buffers, queued on `stream` (hipStream_t); the engine waits on the
 * stream itself between rounds only when a masked run is deeper than the
 * graph's static depth bound. */
int ospf_ksp2_dev(ospf_ctx* ctx, const ospf_ksp2* args, void* stream);
/* The k = 2 masked reruns run as decremental SSSP from the source's row (the
 * nodes whose every tight in-link the ignored links cut, directly or through
 * other such nodes, get new distances; the rest keep the source's) with the
 * trace fused in one launch; a run past that kernel's LDS budgets takes the
 * full masked rerun. Cumulative counts of this context since open: out3 =
 * {runs by the decremental kernel, runs sent to the full reruns, affected
 * nodes summed over the decremental runs}. OSPF_KSP_NODECR in the environment
 * sends every run to the full reruns. */
int ospf_ksp2_stats(const ospf_ctx* ctx, uint64_t* out3);

/* Incremental updates (Decision.cpp:918-996 re-runs SPF after
 * every debounced adjacency batch; LinkState clears every memoised result on
 * a topology change, LinkState.cpp:751-754). When a batch changes only link
 * metrics, link up/down state or node overload bits -- no link or node added
 * or removed -- the resident device CSR is patched in place instead of
 * reloaded, and ospf_affected_roots tells which of a set of finished runs can
 * differ under the new state; the others are bit-identical and need no rerun.
 *
 * Link update: the two CSR entries of link_id get Link::isUp() = up and the
 * metrics advertised by each endpoint (metric_lo: the endpoint with the lower
 * node id). Node update: LinkState::isNodeOverloaded. `version` is the
 * caller's new topology version. */
typedef struct ospf_link_update {
  uint32_t link_id;
  uint32_t up;
  uint32_t metric_lo;
  uint32_t metric_hi;
} ospf_link_update;
int ospf_update_links(ospf_ctx* ctx, const ospf_link_update* updates, uint32_t n,
                      uint64_t version);
int ospf_update_nodes(ospf_ctx* ctx, const uint32_t* nodes, const uint8_t* no_transit,
                      uint32_t n, uint64_t version);

/* Structural update in place: links added or removed between existing nodes
 * -- LinkState's [LINK UP] / [LINK DOWN] (LinkState.cpp:632-657; Decision
 * applies them per adjacency database, Decision.cpp:743-765). `csr` is the
 * caller's whole CSR after the change (same nodes and node ids, any link ids:
 * a removed link's id simply no longer appears, an added link may take a new
 * or a retired id), `rows` the nodes whose rows changed (both ends of every
 * added / removed link). The engine rebuilds those rows (and, when a row's
 * parallel links to a neighbour may have been reordered, that neighbour's
 * row) in their padded slots, moving the rows after a row that outgrows its
 * slots, and refreshes the distinct-neighbour lists, link positions and
 * planner bounds. O(changed rows) host work plus device copies; sweeps made
 * before the call return OSPF_E_NOGRAPH. OSPF_E_RANGE when the layout's
 * reserve (~3 % of entries, distinct neighbours, link ids) is exhausted, a
 * metric leaves the contract, or the node count differs: reload with
 * ospf_load_graph. On any error the context is unchanged except after a
 * device error (then reload). */
int ospf_update_rows(ospf_ctx* ctx, const ospf_csr* csr, const uint32_t* rows, uint32_t n,
                     uint64_t version);

/* One change of a batch, for ospf_affected_roots. LINK: endpoints a, b;
 * before / after: up, metric advertised by a (w_ab) and by b (w_ba). NODE:
 * node a changed its overload bit (either way). */
#define OSPF_CHANGE_LINK 0u
#define OSPF_CHANGE_NODE 1u
typedef struct ospf_change {
  uint32_t kind;
  uint32_t a, b;
  uint32_t up0, w_ab0, w_ba0;
  uint32_t up1, w_ab1, w_ba1;
} ospf_change;
/* Which finished runs can change: d_dist = their distance rows ([n_roots][V],
 * device, computed before the batch), flags as the runs were made (only
 * OSPF_HOP_COUNT is read); d_affected[i] = 1 if run i must be re-run, 0 if
 * its dist / next hops / pathLinks are unchanged. Run i is unaffected when no
 * changed link was tight for it before (dist(a) + w_ab0 == dist(b), or the
 * reverse) nor reaches or ties a distance after (dist(a) + w_ab1 <= dist(b),
 * or the reverse), and every re-flagged node either is unreached, is the root,
 * or has no up link (x, y) with dist(x) + w(x -> y) <= dist(y) (transit
 * conditions are ignored: the answer errs towards re-running). Graph state
 * read for node changes: the current (patched) one. Queued on `stream`. */
int ospf_affected_roots(ospf_ctx* ctx, const uint32_t* d_dist, uint32_t n_roots, uint32_t flags,
                        const ospf_change* changes, uint32_t n_changes, uint8_t* d_affected,
                        void* stream);

/* Repair finished runs in place after a patch (ospf_update_links /
 * ospf_update_nodes): d_dist / d_nh hold rows computed before the batch
 * ([n][V], [n][V][nh_words], device) for roots d_roots, made with `flags`
 * (OSPF_HOP_COUNT read). A run none of whose shortest distances the batch
 * changes -- only next-hop sets and ties move, the usual effect of a link
 * event in an ECMP fabric -- gets its next-hop words re-derived where they
 * change (d_status[i] = 0: the rows now equal a fresh run's). Link changes
 * and overload toggles (node changes: the current transit bit is read) are
 * both repaired, in one call and in either order: whether a changed link was
 * tight before the batch is judged from its old up flag and metric alone, not
 * from its tail's transit bit (which is the patched one), so a node that sets
 * overload and loses or re-metrics a link in the same batch is repaired like
 * the two events apart. A run whose distances would change, or beyond the repair
 * budget (8192 re-derivations, 1024 queued nodes), gets d_status[i] = 1 and
 * must be re-run. Digests are not maintained. Queued on `stream`. */
int ospf_repair_runs(ospf_ctx* ctx, const uint32_t* d_roots, uint32_t n, uint32_t flags,
                     uint32_t nh_words, uint32_t* d_dist, uint32_t* d_nh,
                     const ospf_change* changes, uint32_t n_changes, uint32_t* d_status,
                     void* stream);

/* Take links down for a while and put back exactly what was there. The
 * reference reruns runSpf(src, true, linksToIgnore) with every link of the
 * k = 1 paths ignored (LinkState.cpp:802-806); an ignore set beyond one
 * run's list (OSPF_MAX_IGNORED_PER_RUN) is applied to the device graph
 * instead. ospf_links_mask marks the links down (like ospf_update_links);
 * ospf_links_unmask restores their entries and the planner state (level and
 * distance bounds, metric facts, the prepared cover graph), so the pair
 * leaves no trace in later runs. One mask at a time. */
int ospf_links_mask(ospf_ctx* ctx, const uint32_t* link_ids, uint32_t n, uint64_t version);
int ospf_links_unmask(ospf_ctx* ctx);

/* ---------------------------------------------------------------- sweeps
 * All-sources sweeps: runSpf (LinkState.cpp:836-911) for every node of the
 * graph -- or for one part of a root partition (multi-GPU) -- with every
 * root's dist row and next-hop row written to device memory the sweep owns,
 * plus a digest per root. The reference's all-sources use is
 * Decision::getDecisionRouteDb(node) for every node (openr/decision/
 * Decision.cpp:309) and `breeze decision routes --nodes all` (openr/py/openr/
 * cli/commands/decision.py:26-48): one getSpfResult per node. A sweep owns
 * the whole orchestration -- the path, the root order, the width classes,
 * their streams and the HIP graph one run replays:
 *   OSPF_SWEEP_DERIVE  unit metric or hop count, depth bound <= 123, <= 2048
 *                      distinct neighbours per node: distance-only 128-root
 *                      BFS over the closure of the roots, then each root's
 *                      next hops from its neighbours' level rows
 *                      (ospf_levels_dev + ospf_nh_derive_dev);
 *   OSPF_SWEEP_WCOVER  link metrics: distance rows of a vertex cover by the
 *                      contracted-graph SPF, leaf rows and cover next hops
 *                      derived from them (ospf_cover_*, ospf_wderive*_dev);
 *   OSPF_SWEEP_WDERIVE cover rows on the per-root batch path, leaf rows
 *                      derived (any metric, or hop count);
 *   OSPF_SWEEP_BATCH   per width class batches (ospf_run_batch_dev);
 *   OSPF_SWEEP_LDS     small graphs, unit metric or hop count, <= 4 next-hop
 *                      words: one launch per width class, a wave per root
 *                      with the graph in LDS (ospf_lds_sweep_dev);
 *   OSPF_SWEEP_WMULTI  any metric (or hop count), large graphs without a
 *                      small cover (meshes): the rows the part needs by a
 *                      multi-root traversal (groups of 32 roots adjacent in
 *                      id order, [node][root] distances, Delta-stepping),
 *                      leaf rows and next hops derived from them.
 * OSPF_SWEEP_AUTO takes LDS when it applies, then the others in the order
 * above. Row layout:
 * dist u32[V] per root; next hops u32[V][W] with W = max(1, ceil(distinct
 * neighbours / 32)) words in the bit order of ospf_root_neighbors. A sweep
 * belongs to the graph it was created on: after ospf_load_graph,
 * ospf_update_* or ospf_links_mask, ospf_sweep_run returns OSPF_E_NOGRAPH
 * (rows already computed stay readable). Partition (n_parts > 1): each width
 * class, ordered by each node's largest neighbour id, is cut into n_parts
 * contiguous slices -- a fabric's racks and fabric switches by pod, its
 * spines by plane -- so a part's closure stays small. */
#define OSPF_SWEEP_AUTO 0u
#define OSPF_SWEEP_DERIVE 1u
#define OSPF_SWEEP_WCOVER 2u
#define OSPF_SWEEP_WDERIVE 3u
#define OSPF_SWEEP_BATCH 4u
#define OSPF_SWEEP_LDS 5u
#define OSPF_SWEEP_WMULTI 6u
/* opts.flags: create without the eager first run (hip_graph must be 0); the
 * first ospf_sweep_run is then the first run. A caller that runs the sweep
 * once per graph version (odl::LinkState; ospf_msweep_create, which starts
 * every device's first run together) pays one run instead of two. */
#define OSPF_SWEEP_DEFER 0x100u
/* opts.flags, with OSPF_SWEEP_DEFER: the first run starts inside
 * ospf_sweep_create -- each launch unit of the plan's serial prefix (derive
 * mode: the seed BFS and the twin levels) is queued as soon as it is planned,
 * ordered after the null stream's prior work, so the device works on it while
 * the host plans the rest; the first ospf_sweep_run queues the remaining
 * units and joins the caller's stream. For a caller that runs the sweep right
 * after creating it on an unchanged graph (odl::LinkState's re-sweep after a
 * topology change). */
#define OSPF_SWEEP_EARLY_START 0x200u

typedef struct ospf_sweep ospf_sweep;
typedef struct ospf_sweep_opts {
  uint32_t flags;      /* 0 (link metrics) or OSPF_HOP_COUNT, | OSPF_SWEEP_DEFER
                          (| OSPF_SWEEP_EARLY_START) */
  uint32_t mode;       /* OSPF_SWEEP_* */
  uint32_t part;       /* this part of the root partition ... */
  uint32_t n_parts;    /* ... over n_parts (0 or 1: every node) */
  uint32_t hip_graph;  /* 1: capture one run as a HIP graph, runs replay it
                          (eager launches if capture fails: see info).
                          Open: with 32 contexts alive in one process, each
                          with a graph sweep, the replay of a graph with
                          several width classes has ended the process with a
                          segmentation fault once; the cause is not found
                          (DESIGN.md section 2). A process that keeps tens of
                          contexts alive should pass 0. */
} ospf_sweep_opts;

typedef struct ospf_sweep_info {
  uint32_t mode;             /* the path taken (OSPF_SWEEP_*) */
  uint32_t n_roots;          /* roots this part owns */
  uint32_t n_rows;           /* distance rows computed per run (closure / cover rows) */
  uint32_t n_launches;       /* launch units (ospf_sweep_profile) */
  uint32_t hip_graph;        /* 1: runs replay a captured graph */
  uint32_t max_nh_words;     /* widest next-hop row of an owned root */
  uint64_t device_bytes;     /* rows, level rows, digests, tables */
  uint64_t step_compulsory_bytes;  /* rows written + CSR scans, per run */
  /* edges the run's traversal kernels relax: traversed rows x edges of the
   * graph they traverse (derive: seed BFS rows x E; weighted cover: seeds'
   * Dial rows x contracted-graph edges; batch / LDS: roots x E). Rows
   * derived from other rows relax no edge. TEPS = this / run time. */
  uint64_t step_traversed_edges;
} ospf_sweep_info;

/* One launch unit of a run, timed alone on its stream (HIP events). */
typedef struct ospf_sweep_launch {
  char name[32];
  char kernel[112];
  uint32_t n_roots;          /* runs the launch computes */
  uint32_t nh_words;         /* 0 = distance rows only */
  uint64_t compulsory_bytes; /* rows written + CSR / source rows read at least once */
  double ms_median;          /* isolated launch time, median of the reps */
  double ms_min;
} ospf_sweep_launch;

int ospf_sweep_create(ospf_ctx* ctx, const ospf_sweep_opts* opts, ospf_sweep** out);
int ospf_sweep_destroy(ospf_sweep* sw);
const char* ospf_sweep_last_error(const ospf_sweep* sw);
int ospf_sweep_get_info(const ospf_sweep* sw, ospf_sweep_info* info);
/* The owned roots, in digest order ([n_roots] host). */
int ospf_sweep_roots(const ospf_sweep* sw, uint32_t* roots);
/* One all-sources run queued on `stream` (hipStream_t; not synchronised;
 * ospf_sync(ctx, stream) reports device errors). */
int ospf_sweep_run(ospf_sweep* sw, void* stream);
/* Digests of the owned roots in ospf_sweep_roots order into device memory
 * d_out[n_roots], queued on `stream`. */
int ospf_sweep_digests(ospf_sweep* sw, ospf_digest* d_out, void* stream);
/* Same into host memory out[n_roots], synchronous. */
int ospf_sweep_digests_host(ospf_sweep* sw, ospf_digest* out);
/* Fill every digest the sweep keeps with 0xFF (a run rewrites them all; a
 * run that did nothing is then visible). */
int ospf_sweep_poison(ospf_sweep* sw, void* stream);
/* Device rows of an owned root (valid until ospf_sweep_destroy). */
int ospf_sweep_row(const ospf_sweep* sw, uint32_t root, const uint32_t** d_dist,
                   const uint32_t** d_nh, uint32_t* nh_words);
/* Host copies of owned roots' rows, synchronous (after the work queued on
 * every stream is done): dist_out [n][V] and nh_out [n][V][nh_words] (each
 * root's W words, zero padded; nh_words >= every root's W), either may be
 * NULL. */
int ospf_sweep_copy_rows(ospf_sweep* sw, const uint32_t* roots, uint32_t n, uint32_t nh_words,
                         uint32_t* dist_out, uint32_t* nh_out);
/* Anycast route selection over the sweep's resident rows:
 * SpfSolver::getNextHopsWithMetric (openr/decision/SpfSolver.cpp:1043-1089)
 * for every owned root and every prefix of a table, in one launch, instead
 * of ospf_sweep_copy_rows + a host loop per root. The table is CSR in host
 * memory: prefix p is announced by nodes[offsets[p] .. offsets[p + 1]), node
 * ids strictly ascending within a prefix (a prefix may be empty). Outputs, in
 * ospf_sweep_roots order:
 *   metric [n_roots][P]  the smallest dist[root][a] over the announcers a the
 *                        root reaches (an announcer absent from the SPF result
 *                        is skipped, :1065-1068); OSPF_DIST_INF when none is;
 *   count  [n_roots][P]  announcers at that metric (minCostNodes, :1070-1076;
 *                        0 when none is reached);
 *   nh     [n_roots][P][nh_words]  the OR of those announcers' next-hop words
 *                        (:1080-1086), bit order of ospf_root_neighbors; a
 *                        root's words W .. nh_words are zero.
 * A root that announces the prefix itself gets metric 0, count 1 and no next
 * hop (its own SPF entry). Any output may be NULL (not wanted); every word of
 * a wanted output is written, once. nh_words >= the sweep's max_nh_words.
 * Preconditions as ospf_sweep_copy_rows: the sweep has run and its rows are
 * complete (the _dev call does not wait for streams other than `stream`).
 * OSPF_E_INVAL (reason in ospf_sweep_last_error, nothing written): an id >= V,
 * a list not strictly ascending, offsets not monotone, nh_words too small,
 * no run yet. n_prefixes == 0 or a part without roots: OSPF_OK, nothing
 * written. The row table is uploaded once per sweep, the prefix table on
 * every call (synchronously, before the kernel is queued on `stream`). */
typedef struct ospf_select_table { /* host memory */
  uint32_t n_prefixes;
  const uint32_t* offsets; /* [n_prefixes + 1] */
  const uint32_t* nodes;   /* announcer ids, strictly ascending per prefix */
} ospf_select_table;
/* device outputs, queued on `stream` after the table's upload */
int ospf_sweep_select_dev(ospf_sweep* sw, const ospf_select_table* table, uint32_t nh_words,
                          uint32_t* d_metric, uint32_t* d_count, uint32_t* d_nh, void* stream);
/* host outputs, synchronous (after the work queued on every stream) */
int ospf_sweep_select(ospf_sweep* sw, const ospf_select_table* table, uint32_t nh_words,
                      uint32_t* metric, uint32_t* count, uint32_t* nh);
/* Route selection under the reference's best-route policy: what
 * createRouteForPrefix (openr/decision/SpfSolver.cpp:197-458) decides around
 * the minimum ospf_sweep_select takes, for every owned root and every prefix
 * of a table, in one launch. Each announcer entry i of a prefix carries
 *   pref[i]         the rank of its (path preference, source preference,
 *                   distance) class within the prefix: a u32 below 2^31, the
 *                   smaller wins (selectBestRoutes -> selectRoutes(
 *                   SHORTEST_DISTANCE), SpfSolver.cpp:649-676, LsdbUtil.cpp:
 *                   841-883);
 *   min_nexthop[i]  its minNexthop threshold, 0 = unset;
 * and its node's drained bit, which is the no-transit (overload) bit of the
 * LOADED graph (in-place node patches are followed). Per (root r, prefix p):
 *   R  = the entries with dist[r][a_i] != OSPF_DIST_INF (:229-244; r itself
 *        is at distance 0 when it announces);
 *   S  = the entries of R at the smallest pref;
 *   S' = the undrained entries of S, or S when all of S are drained
 *        (maybeFilterDrainedNodes, :709-731);
 *   L  = the entries of S' at the smallest distance m.
 * That is one unsigned minimum of key_i = pref_i << 33 | drained_i << 32 |
 * dist_i over R (DESIGN.md §3 p'''). Outputs, in ospf_sweep_roots order:
 *   metric [n][P]  m; OSPF_DIST_INF when R is empty;
 *   count  [n][P]  |L|; 0 when R is empty;
 *   nh     [n][P][nh_words]  the OR of the next-hop words of L, zero padded;
 *   links  [n][P]  the next-hop links getNextHopsThrift emits for an IP
 *                  route: the sum of c(r, k) over the set bits k of nh, c as
 *                  ospf_selstate_ucmp defines it (up links r - k at the
 *                  smallest metric r advertises on an up link to k; every up
 *                  link under OSPF_HOP_COUNT), from the loaded graph. The sum
 *                  is plain and exact: no c(r, k) is capped, because a graph
 *                  with more than OSPF_MAX_PARALLEL_LINKS (65,535) entries
 *                  r -> k is refused at load (OSPF_E_RANGE), never answered
 *                  with a smaller count;
 *   need   [n][P]  the largest min_nexthop over S' (not over L: the reference
 *                  takes it over allNodeAreas, :693-707); 0 when R is empty.
 *                  The route is withheld iff need > links and links > 0
 *                  (:990-1000);
 *   best   [n][P]  bestNodeArea: r when r is in S, else the smallest node id
 *                  of S (S, not S': picked before the drain filter, which
 *                  never moves it, :724-728); 0xFFFFFFFF when R is empty.
 * A root in L gets metric 0, count 1 and no next hop; a drained root that
 * announces p beside an undrained announcer of its class is NOT selected and
 * gets a route to the other. Any output may be NULL; every word of a wanted
 * output is written exactly once (plain stores, no memset, no atomics).
 * Preconditions, errors and the nothing-written-on-error rule are those of
 * ospf_sweep_select; in addition OSPF_E_INVAL for a pref >= 2^31, a NULL pref
 * (with announcers) and a sweep that does not describe the context's current
 * graph (the kernel reads the live CSR and no-transit bits).
 * SR_MPLS per-destination next hops: ospf_sweep_select_srmpls below (one area,
 * one sweep). Not covered: K_SHORTEST_DISTANCE_2 and
 * PER_AREA_SHORTEST_DISTANCE, BGP metric vectors. (Several areas:
 * ospf_areas_select_policy below. The same
 * selection kept resident, its delta and UCMP over it: the policy state of
 * ospf_selstate_create_policy below.) */
typedef struct ospf_select_ptable { /* host memory */
  uint32_t n_prefixes;
  const uint32_t* offsets;     /* [n_prefixes + 1] */
  const uint32_t* nodes;       /* strictly ascending per prefix */
  const uint32_t* pref;        /* [offsets[P]], < 2^31, smaller wins */
  const uint32_t* min_nexthop; /* [offsets[P]] or NULL (all unset) */
} ospf_select_ptable;
typedef struct ospf_select_pout {
  uint32_t *metric, *count, *nh, *links, *need, *best;
} ospf_select_pout;
/* device outputs, queued on `stream` after the table's upload */
int ospf_sweep_select_policy_dev(ospf_sweep* sw, const ospf_select_ptable* table,
                                 uint32_t nh_words, const ospf_select_pout* d_out, void* stream);
/* host outputs, synchronous (after the work queued on every stream) */
int ospf_sweep_select_policy(ospf_sweep* sw, const ospf_select_ptable* table, uint32_t nh_words,
                             const ospf_select_pout* out);
/* The same selection for a prefix forwarded as SR_MPLS: selectBestPathsSpf
 * calls getNextHopsWithMetric(..., perDestination = true) (openr/decision/
 * SpfSolver.cpp:784-806), so the route is a set of (next hop, destination)
 * pairs (:1189-1261) and the next hops of the selected announcers are NOT
 * ORed. Each entry i carries, beside pref and min_nexthop,
 *   flags[i]        OSPF_SEL_SELF_PREPEND (bit 0): the entry has a prepend
 *                   label; it matters only on the root's own entry. Any other
 *                   bit set is OSPF_E_INVAL.
 * Per (root r, prefix p), with R, S, S', need and best exactly as
 * ospf_sweep_select_policy defines them (need includes the root's own entry):
 *   D  = S' without r's own entry when that entry is in S' and has
 *        OSPF_SEL_SELF_PREPEND (filteredBestNodeAreas, :794-802: an announcing
 *        root routes to the OTHER announcers); S' otherwise;
 *   m  = the smallest dist[r][a_i] over D, L = the entries of D at m.
 * Outputs, rows in ospf_sweep_roots order, A = offsets[n_prefixes]:
 *   metric [n][P]   m; OSPF_DIST_INF when R or D is empty;
 *   count  [n][P]   |L|; a root in L (flag unset) gets metric 0, count 1 and
 *                   nothing else, as in the policy call;
 *   need, best [n][P]  as ospf_sweep_select_policy;
 *   dst_nh [n][A][nh_words]  per ENTRY: the next-hop words of a_i's row when
 *                   i is in L and a_i != r, else zero; a root's words
 *                   W .. nh_words are zero;
 *   dst_links [n][A]  the sum of c(r, k) over the set bits k of dst_nh[i]
 *                   (c as `links` of ospf_sweep_select_policy);
 *   links  [n][P]   the sum of dst_links over the prefix's entries: the number
 *                   of (link, destination) pairs. It equals nextHops.size()
 *                   of the reference route when every destination's node
 *                   label is valid, the labels are pairwise distinct and any
 *                   prepend label is valid -- the engine never sees labels;
 *                   the consumer builds the PUSH stacks (:1231-1261) and
 *                   pushes nothing when the next hop IS the destination.
 *                   The route is installed iff links > 0 and need <= links.
 * "Do not reach one destination through another" (:1205-1211) cannot fire
 * here: a next hop k of a destination at distance m has dist[r][k] < m
 * (metrics >= 1), m is the minimum over D and S' \ D is r itself, so k is not
 * in S'; it is not evaluated.
 * Contract, preconditions and errors are ospf_sweep_select_policy's: any
 * output may be NULL, every word of a wanted output is written exactly once by
 * plain stores, nothing is written on error.
 * Not covered: this selection kept resident (ospf_selstate_*) and its delta,
 * several areas, ospf_msweep, K_SHORTEST_DISTANCE_2, label validity and static
 * MPLS next hops (:1019-1029). */
#define OSPF_SEL_SELF_PREPEND 0x1u
typedef struct ospf_select_stable { /* host memory; ospf_select_ptable + flags */
  uint32_t n_prefixes;
  const uint32_t* offsets;     /* [n_prefixes + 1] */
  const uint32_t* nodes;       /* strictly ascending per prefix */
  const uint32_t* pref;        /* [offsets[P]], < 2^31, smaller wins */
  const uint32_t* min_nexthop; /* [offsets[P]] or NULL (all unset) */
  const uint32_t* flags;       /* [offsets[P]] or NULL (all 0) */
} ospf_select_stable;
typedef struct ospf_select_sout {
  uint32_t *metric, *count, *links, *need, *best; /* [n][P] */
  uint32_t* dst_links;                            /* [n][A], A = offsets[P] */
  uint32_t* dst_nh;                               /* [n][A][nh_words] */
} ospf_select_sout;
/* device outputs, queued on `stream` after the table's upload */
int ospf_sweep_select_srmpls_dev(ospf_sweep* sw, const ospf_select_stable* table,
                                 uint32_t nh_words, const ospf_select_sout* d_out, void* stream);
/* host outputs, synchronous (after the work queued on every stream) */
int ospf_sweep_select_srmpls(ospf_sweep* sw, const ospf_select_stable* table, uint32_t nh_words,
                             const ospf_select_sout* out);
/* The same selection across several areas (createRouteForPrefix is multi-area
 * at its core, SpfSolver.cpp:229-244, :365-443), for every node of the union
 * of the areas and every prefix, in one launch. Areas 0 .. n_areas - 1 are
 * given in area-name byte order; each is one sweep that has run, owns every
 * root (one part) and describes its context's current graph, all on one
 * device and in one metric mode. The union of the node names, sorted by name
 * bytes, gives global ids 0 .. n_global - 1; gid[a][i] is the global id of
 * area a's node i (strictly ascending in i: both orders are name rank). An
 * entry of a prefix is a (global node n, area a) pair with pref (< 2^31,
 * smaller wins) and min_nexthop (0 = unset); entries are strictly ascending
 * per prefix in (n, a) -- the order of the reference's std::set<NodeAndArea>,
 * which decides bestNodeArea -- and n exists in a. Per global root g (its
 * areas: those that contain it) and prefix p:
 *   R  = the entries (n, a) with g in a and dist_a[g][n] finite (reachability
 *        is judged in the entry's own area only; g itself is at distance 0);
 *   S  = the entries of R at the smallest pref;
 *   S' = the entries of S whose node is not drained in its own area's loaded
 *        graph, or S when all are (:709-731);
 *   per area a of g with at least one entry OF ITS OWN in S' (the default
 *   computation rules): the destinations are the nodes of ALL of S', whatever
 *   their area, that exist in a and that g reaches there (the reference looks
 *   other areas' announcers up in this area's SPF, :805-806, :1064-1068);
 *   m_a = the smallest dist_a[g][.] over them, L_a = those at m_a (each node
 *   once), nh_a = the OR of their next-hop words in a;
 *   metric = the smallest m_a; the winning areas are those at it (:399-407).
 * Outputs, by global id:
 *   metric [G][P]  OSPF_DIST_INF when R is empty;
 *   count  [G][P]  the sum of |L_a| over the winning areas;
 *   links  [G][P]  the sum over the winning areas of the links of nh_a, c(r, k)
 *                  from that area's loaded graph as ospf_sweep_select_policy
 *                  has it (next hops of different areas never merge: the area
 *                  is part of the next hop);
 *   need   [G][P]  the largest min_nexthop over S', all areas; the route is
 *                  withheld iff need > links and links > 0;
 *   best   [G][P]  the position within the prefix of the first entry of S
 *                  whose node is g, else of the first entry of S (S, not S');
 *                  0xFFFFFFFF when R is empty;
 *   areas  [G][P]  the bit mask of the winning areas (0 when R is empty);
 *   nh[a]  [V_a][P][nh_words[a]]  by area a's node id: nh_a of a winning area,
 *                  zero for any other; nh_words[a] >= that sweep's max_nh_words.
 * With one area this is ospf_sweep_select_policy word for word, rows by node
 * id and best as an entry position. Any output may be NULL (`nh` as a whole or
 * one area's); every word of a wanted output is written exactly once by plain
 * stores; nothing is written on error. The _dev call uploads the table, the
 * global -> local id maps and the per-area pointers, then queues the kernel on
 * `stream` (a stream of area 0's device); it does not wait for other streams.
 * The upload is one synchronous copy from host memory, into a block kept on
 * area 0's sweep: the call first waits on the host for the kernel of the
 * previous areas call made through that sweep, so two such calls do not
 * overlap.
 * OSPF_E_INVAL with the reason in area 0's sweep's last error: n_areas 0 or
 * > 32, a NULL sweep, sweeps on different devices, a sweep that has not run,
 * is stale against its context's graph or does not own every root, mixed
 * metric modes, gid not strictly ascending or >= n_global, a global id no area
 * holds, an entry whose node is absent from its area, entries not strictly
 * ascending in (node, area), area >= n_areas, pref >= 2^31 or NULL with
 * entries, an nh_words[a] too small. n_prefixes == 0: OSPF_OK, nothing written.
 * The same selection kept resident and its delta: ospf_areastate_* below.
 * Not covered: UCMP across areas, SR_MPLS per-destination next hops across
 * areas (one area: ospf_sweep_select_srmpls) and KSP2, BGP metric vectors,
 * ospf_msweep and several devices. */
typedef struct ospf_areas_table { /* host memory */
  uint32_t n_areas;               /* 1 .. 32 */
  ospf_sweep* const* sweeps;      /* [n_areas] */
  const uint32_t* const* gid;     /* [n_areas][V_a] */
  uint32_t n_global;
  uint32_t n_prefixes;
  const uint32_t* offsets;        /* [n_prefixes + 1] */
  const uint32_t* node;           /* [offsets[P]] global ids */
  const uint32_t* area;           /* [offsets[P]] */
  const uint32_t* pref;           /* [offsets[P]], < 2^31, smaller wins */
  const uint32_t* min_nexthop;    /* [offsets[P]] or NULL (all unset) */
} ospf_areas_table;
typedef struct ospf_areas_pout {
  uint32_t *metric, *count, *links, *need, *best, *areas; /* [G][P] */
  uint32_t* const* nh;            /* [n_areas] (an entry may be NULL), or NULL */
  const uint32_t* nh_words;       /* [n_areas]; may be NULL when nh is */
} ospf_areas_pout;
/* device outputs, queued on `stream` after the uploads */
int ospf_areas_select_policy_dev(const ospf_areas_table* table, const ospf_areas_pout* d_out,
                                 void* stream);
/* host outputs, synchronous (after the work queued on every stream) */
int ospf_areas_select_policy(const ospf_areas_table* table, const ospf_areas_pout* out);
/* Only the route selections a re-sweep changed: the counterpart of
 * DecisionRouteDb::calculateUpdate (openr/decision/SpfSolver.cpp:24-59, called
 * from Decision.cpp:963) for the route DB ospf_sweep_select answers. An
 * ospf_selstate belongs to a context, not to a sweep (a sweep lives for one
 * graph version), and to one prefix table, copied at create (contract and
 * errors of ospf_select_table as above, against the loaded graph's V). It
 * keeps the selection of every root resident on the device in the root's own
 * width: per root metric [P], count [P], nh [P][W_root], indexed by NODE ID
 * (ospf_sweep_roots order changes between plans), twice (double-buffered).
 *   prime   stores sw's selection as the baseline; reports nothing.
 *   update  computes sw's selection into the shadow buffer (its own per-root
 *           offsets: W_root may have changed), compares it on the device with
 *           the stored one and returns the entries that changed, then commits
 *           by swapping the buffers. Host outputs, synchronous.
 *   copy    the stored selection of `roots`, expanded as ospf_sweep_select
 *           does: metric / count [n][P], nh [n][P][nh_words] (a root's words
 *           W_root .. nh_words zero); any output may be NULL.
 * A root's entry for a prefix is {metric, count, its W_root next-hop words},
 * exactly as ospf_sweep_select defines them; an entry changed when any of them
 * differs. A prefix that lost its last reached announcer comes back as metric
 * = OSPF_DIST_INF, count = 0: the caller's route to delete. A change record
 * carries the NEW values; nh[i] holds record i's words zero-padded to
 * nh_words (nh may be NULL; nh_words >= the sweep's max_nh_words either way).
 * The order of the records is unspecified.
 * Next-hop bits are positions in the root's distinct-neighbour list
 * (ospf_root_neighbors). When that list differs between the stored version
 * and sw's graph the old and new words are not comparable (equal words can
 * mean different neighbours), so the state keeps every root's list (dn_off /
 * dn, about E words) and compares it on the device: a root whose list changed
 * is "rebased" -- reported once in rebased_roots, none of its entries listed;
 * the caller reads them with ospf_selstate_copy.
 * sw must belong to the state's context, have run, describe the context's
 * current graph, and own every node of a graph with the state's V: anything
 * else (another V, a part of the roots) is OSPF_E_INVAL with the state
 * untouched. Several parts / ospf_msweep are not supported here.
 * n_changes > cap or n_rebased > cap_rebased: OSPF_E_RANGE with both counts
 * filled; the state is UNCHANGED and whatever the lists hold is to be
 * ignored -- the caller retries with larger capacities and gets the complete
 * set. update / copy before prime: OSPF_E_INVAL. n_prefixes == 0: OSPF_OK with
 * zero counts. Any failure (an injected one included) leaves the state as it
 * was. Errors through ospf_selstate_last_error (and ospf_last_error). */
typedef struct ospf_selstate ospf_selstate;
typedef struct ospf_select_change {
  uint32_t root, prefix, metric, count;
} ospf_select_change;
int ospf_selstate_create(ospf_ctx* ctx, const ospf_select_table* table, ospf_selstate** out);
int ospf_selstate_destroy(ospf_selstate* st);
const char* ospf_selstate_last_error(const ospf_selstate* st);
/* device memory the state holds now (both buffers, lists, the table) */
uint64_t ospf_selstate_device_bytes(const ospf_selstate* st);
int ospf_selstate_prime(ospf_selstate* st, ospf_sweep* sw);
int ospf_selstate_update(ospf_selstate* st, ospf_sweep* sw, uint32_t nh_words,
                         ospf_select_change* changes, uint32_t* nh /*[cap][nh_words]*/,
                         uint32_t cap, uint32_t* n_changes, uint32_t* rebased_roots,
                         uint32_t cap_rebased, uint32_t* n_rebased);
int ospf_selstate_copy(ospf_selstate* st, const uint32_t* roots, uint32_t n, uint32_t nh_words,
                       uint32_t* metric, uint32_t* count, uint32_t* nh);
/* UCMP weights of every root and prefix, resolved on the device over the
 * selection a primed state holds: SpfSolver::getNodeUcmpResult ->
 * LinkState::resolveUcmpWeights (openr/decision/SpfSolver.cpp:1091-1161,
 * LinkState.cpp:913-1033) for all roots at once, instead of a priority-queue
 * walk per root and prefix. The weight a node advertises in any root's walk is
 * that of its own selection (DESIGN.md §3 o'''):
 *   W(u) = leaf weight                       u announces the prefix (metric 0)
 *   W(u) = sum over u's selected next hops k of
 *            c(u, k) * W(k)                  OSPF_UCMP_PREFIX
 *            S(u, k)                         OSPF_UCMP_ADJ
 * c(u, k) = the tight links u - k: up, at the smallest metric u advertises on
 * an up link to k (every up link when the selection was swept under
 * OSPF_HOP_COUNT); derived on the device from the loaded graph, in-place
 * patches included. S(u, k) = the sum of u's link weights (getWeightFromNode)
 * over those links: the engine holds no link weights, so the caller passes
 * link_weight_sum, one per distinct-neighbour slot in the order of
 * ospf_root_neighbors, node after node (n_slots of them: the count
 * ospf_selstate_ucmp_info reports); NULL is allowed for OSPF_UCMP_PREFIX.
 * leaf_weight is parallel to the table's `nodes` (one per announcer entry).
 *   ospf_selstate_ucmp       resolves W and a status for every (node, prefix)
 *                            and keeps them resident; *rounds = gather rounds
 *                            taken = the hop depth of the deepest selected path.
 *   ospf_selstate_ucmp_copy  the per-link view of some roots: advertised
 *                            [n][P], status [n][P], and a CSR off [n * P + 1] /
 *                            wt of the root's next-hop weights -- one per set
 *                            next-hop bit of the entry, in bit order, W(k)
 *                            divided by the gcd of the entry's weights when it
 *                            is > 1 (normalizeNextHopWeights, LinkState.h:
 *                            317-328); every tight link to k carries wt. An
 *                            entry that is not OSPF_UCMP_OK has advertised 0
 *                            and no weights.
 *                            off NULL: advertised and status only (wt, cap
 *                            ignored, *n_wt = 0).
 * Status: OK; NONE no announcer reached; VOID a zero-weight announcer among
 * the min-cost ones (getNodeUcmpResult returns nullopt, :1139-1142; it
 * propagates to every node that selects through it); OVERFLOW a sum above
 * 2^63 - 1 (propagates likewise; VOID wins over OVERFLOW). An entry is OK only when
 * its advertised weight AND its next hops' weights are representable, so under
 * OSPF_UCMP_ADJ too an OVERFLOW next hop marks the entry (deliberate).
 * OSPF_E_INVAL, nothing changed: a state not primed; a graph version other
 * than the one the state's selection was stored on (reload or patch without
 * ospf_selstate_update); a negative weight; OSPF_UCMP_ADJ without
 * link_weight_sum; n_slots that does not match; copy before a run, or after
 * the selection changed (update) without a new run. copy with more weights
 * than `cap`: OSPF_E_RANGE, *n_wt = the count needed, no output written. Any
 * failure (an injected one included) leaves the previous result as it was.
 * Several parts / ospf_msweep are not supported (as the state). */
#define OSPF_UCMP_ADJ 2u    /* SP_UCMP_ADJ_WEIGHT_PROPAGATION */
#define OSPF_UCMP_PREFIX 3u /* SP_UCMP_PREFIX_WEIGHT_PROPAGATION */
#define OSPF_UCMP_OK 0u
#define OSPF_UCMP_NONE 1u
#define OSPF_UCMP_VOID 2u
#define OSPF_UCMP_OVERFLOW 3u
int ospf_selstate_ucmp(ospf_selstate* st, uint32_t algo, const int64_t* leaf_weight,
                       const int64_t* link_weight_sum, uint32_t n_slots, uint32_t* rounds);
int ospf_selstate_ucmp_copy(ospf_selstate* st, const uint32_t* roots, uint32_t n,
                            int64_t* advertised, uint8_t* status, uint64_t* off, int64_t* wt,
                            uint64_t cap, uint64_t* n_wt);
/* rounds of the last run (0: none yet) and the graph's distinct-neighbour
 * slots (the length of link_weight_sum); either may be NULL */
int ospf_selstate_ucmp_info(const ospf_selstate* st, uint32_t* rounds, uint32_t* n_slots);
/* A select state that holds ospf_sweep_select_policy's selection: what
 * calculateUpdate diffs and getNodeUcmpResult walks from when best-route
 * selection, drained nodes or minNexthop are in play (the reference applies
 * the policy before both).
 *   create_policy  the table and its pref / min_nexthop columns are copied;
 *                  the table's contract and errors are ospf_sweep_select_policy's
 *                  (a pref >= 2^31, a NULL pref with announcers: OSPF_E_INVAL).
 *                  A policy state keeps, per root and by node id, metric [P],
 *                  count [P], links [P], need [P], best [P], nh [P][W_root]
 *                  (SoA, no padding), twice: two buffers of the sum over the
 *                  roots of P * (5 + W_root) * 4 bytes.
 *   prime          ospf_selstate_prime, unchanged.
 *   update_policy  ospf_selstate_update for this state: an entry changed when
 *                  any of metric, count, links, need, best or a next-hop word
 *                  differs; a record carries the NEW values and installed =
 *                  links > 0 && need <= links. OSPF_E_RANGE / state unchanged /
 *                  retry, rebased roots, commit by swap, the preconditions on
 *                  sw and "any failure leaves the state as it was" hold as
 *                  there. The drained bits and the links are read from the
 *                  LOADED graph, so an in-place node overload
 *                  (ospf_update_nodes) + re-sweep is reported like any event.
 *   copy_policy    the committed entries of `roots` in
 *                  ospf_sweep_select_policy's layout ([n][P], nh
 *                  [n][P][nh_words]); any output may be NULL.
 *                  ospf_selstate_copy on a policy state answers metric /
 *                  count / nh as well.
 *   set_policy     replaces the two columns (offsets / nodes stay; the same
 *                  checks; min_nexthop NULL: all unset). Nothing committed
 *                  changes: the next update_policy, even with the same sweep,
 *                  reports what the new attributes changed -- the delta of a
 *                  prefix-attribute change without a topology event. A
 *                  resolved UCMP result becomes stale, as after an update.
 * ospf_selstate_ucmp / ospf_selstate_ucmp_copy run over a policy state too.
 * There an announcer need not select itself (a better class behind it, or it
 * is drained beside an undrained class-mate), so a selected next hop whose
 * no-transit bit is set contributes its LEAF weight for the prefix, VOID when
 * that is 0, and is never waited for ("UCMP over the policy
 * selection").
 * The wrong kind of state -- ospf_selstate_update on a policy state,
 * update_policy / copy_policy / set_policy on a plain one -- is OSPF_E_INVAL,
 * nothing changed. A root with more distinct neighbours than the LDS holds
 * link counts for (8 bytes each): OSPF_E_RANGE from prime / update_policy. */
typedef struct ospf_select_pchange {
  uint32_t root, prefix, metric, count, links, need, best, installed;
} ospf_select_pchange;
int ospf_selstate_create_policy(ospf_ctx* ctx, const ospf_select_ptable* table,
                                ospf_selstate** out);
int ospf_selstate_update_policy(ospf_selstate* st, ospf_sweep* sw, uint32_t nh_words,
                                ospf_select_pchange* changes, uint32_t* nh /*[cap][nh_words]*/,
                                uint32_t cap, uint32_t* n_changes, uint32_t* rebased_roots,
                                uint32_t cap_rebased, uint32_t* n_rebased);
int ospf_selstate_copy_policy(ospf_selstate* st, const uint32_t* roots, uint32_t n,
                              uint32_t nh_words, const ospf_select_pout* out);
int ospf_selstate_set_policy(ospf_selstate* st, const uint32_t* pref, const uint32_t* min_nexthop);
/* ospf_areas_select_policy's selection kept resident, and only the cells a
 * re-sweep of some areas (or a change of the entries' attributes) changed:
 * calculateUpdate for the multi-area route DB. An ospf_areastate holds one
 * ospf_areas_table, copied at create (n_areas, n_global, every gid[a], offsets
 * / node / area / pref / min_nexthop; the table's contract and errors as
 * above), and is bound to the contexts behind table->sweeps[a], which are read
 * at create for their context and node count V_a only (a sweep lives for one
 * graph version, the state does not). Per global root g it keeps, by global
 * id, SoA, no padding and twice (double-buffered): metric [P], count [P],
 * links [P], need [P], best [P], areas [P], then for every area a that holds
 * g nh_a [P][W_a(g)] in the root's own width in that area -- two buffers of
 * the sum over g of P * (6 + the sum over g's areas of W_a(g)) * 4 bytes --
 * and every area's distinct-neighbour lists for the rebase test. The calls are
 * ospf_selstate_update_policy's restated over areas:
 *   prime       stores the sweeps' selection as the baseline; reports nothing.
 *   update      computes the sweeps' selection into the shadow buffer (its own
 *               offsets: a W_a(g) may have changed), compares it on the device
 *               and returns the cells that changed, then commits by swapping.
 *               A cell is exactly what ospf_areas_select_policy defines; it
 *               changed when any of its six header words or any next-hop word
 *               of any area of the root differs. A record carries the NEW
 *               values; installed = links > 0 && need <= links is the
 *               caller's to derive. nh[i] is record i's areas one after the
 *               other: area a's words start at word sum of nh_words[b], b < a,
 *               zero-padded to nh_words[a] (>= that sweep's max_nh_words), and
 *               zero for an area that did not win or does not hold the root.
 *               A cell whose R became empty comes back as metric =
 *               OSPF_DIST_INF, count = links = areas = 0, best = 0xFFFFFFFF.
 *               The order of the records is unspecified. A global root whose
 *               distinct-neighbour list differs in any one of its areas
 *               between the stored version and the sweeps' graphs is rebased:
 *               reported once in rebased_roots (global ids), its cells written
 *               and not compared; the caller reads them with copy.
 *   copy        the committed cells of `roots` (global ids) in `roots` order:
 *               the six columns [n][P], nh[a] [n][P][nh_words[a]] (zero for an
 *               area that does not hold the root); any output may be NULL.
 *   set_policy  replaces pref / min_nexthop (the same checks; min_nexthop
 *               NULL: all unset). Nothing committed changes: the next update,
 *               even with the same sweeps, reports what the attributes changed.
 * sweeps[a] must satisfy ospf_areas_select_policy's rules (has run, current
 * against its context, owns every root, one device, one metric mode) and
 * belong to the state's context a with the V_a the state was created with:
 * anything else is OSPF_E_INVAL with the state untouched (a node added to or
 * removed from an area is the caller's cue to create a new state). update /
 * copy before prime: OSPF_E_INVAL. n_prefixes == 0: OSPF_OK with zero counts.
 * n_changes > cap or n_rebased > cap_rebased: OSPF_E_RANGE with both counts
 * complete; the state is UNCHANGED and the lists are to be ignored -- a retry
 * with larger capacities returns the whole set. A root whose link counts do
 * not fit the LDS: OSPF_E_RANGE, as from the select call. Any failure (an
 * injected one on any area's context included) leaves the state as it was.
 * When one of its contexts is closed the state releases its device memory and
 * every later call on it but destroy is OSPF_E_INVAL. Errors through
 * ospf_areastate_last_error. */
typedef struct ospf_areastate ospf_areastate;
typedef struct ospf_areas_change {
  uint32_t root, prefix, metric, count, links, need, best, areas;
} ospf_areas_change;
int ospf_areastate_create(const ospf_areas_table* table, ospf_areastate** out);
int ospf_areastate_destroy(ospf_areastate* st);
const char* ospf_areastate_last_error(const ospf_areastate* st);
/* device memory the state holds now (both buffers, lists, the table) */
uint64_t ospf_areastate_device_bytes(const ospf_areastate* st);
int ospf_areastate_prime(ospf_areastate* st, ospf_sweep* const* sweeps /*[n_areas]*/);
int ospf_areastate_update(ospf_areastate* st, ospf_sweep* const* sweeps,
                          const uint32_t* nh_words /*[n_areas]*/, ospf_areas_change* changes,
                          uint32_t* nh /*[cap][sum of nh_words]*/, uint32_t cap,
                          uint32_t* n_changes, uint32_t* rebased_roots, uint32_t cap_rebased,
                          uint32_t* n_rebased);
/* out->nh_words is read when out->nh is given */
int ospf_areastate_copy(ospf_areastate* st, const uint32_t* roots, uint32_t n,
                        const ospf_areas_pout* out);
int ospf_areastate_set_policy(ospf_areastate* st, const uint32_t* pref,
                              const uint32_t* min_nexthop);
/* Time every launch unit alone on its stream: reps (>= 1) timed launches
 * after one untimed one; fills min(cap, n_launches) records. The sweep must
 * have run once. */
int ospf_sweep_profile(ospf_sweep* sw, uint32_t reps, ospf_sweep_launch* out, uint32_t cap);
/* Diagnostic: the memset nodes of the sweep's captured HIP graph (none
 * unless OSPF_ZERO_MEMSET=1 routes the engine's zeroing through
 * hipMemsetAsync): how many (n_memset), how many whose destination range is
 * not inside a live device allocation (n_dead), how many inside the
 * sweep's own blocks (n_own). */
int ospf_sweep_graph_memsets(const ospf_sweep* sw, uint32_t* n_memset, uint32_t* n_dead,
                             uint32_t* n_own);

/* ---------------------------------------------------------------- devices
 * Several devices of one node behind one handle (SURVEY.md §8(b) ospf_open
 * with n_gpus; Decision runs in one process on one thread,
 * openr/Main.cpp:515-527, so the drop-in reaches the node's GPUs from
 * there). The graph is replicated on every device; an all-sources sweep runs
 * part i of the root partition on device i (no data-path exchange: every
 * run is independent, rows stay device-local); the 24-B digests are gathered
 * onto the first device by peer copies. Devices may repeat (several
 * contexts on one device: a test of the partition on a one-GPU box). */
typedef struct ospf_multi ospf_multi;
typedef struct ospf_msweep ospf_msweep;
int ospf_multi_open(const int* devices, uint32_t n, ospf_multi** out);
int ospf_multi_close(ospf_multi* m);
const char* ospf_multi_last_error(const ospf_multi* m);
uint32_t ospf_multi_size(const ospf_multi* m);
/* the context of device slot i (owned by m) */
ospf_ctx* ospf_multi_ctx(ospf_multi* m, uint32_t i);
int ospf_multi_load_graph(ospf_multi* m, const ospf_csr* csr, uint64_t version);
/* One sweep per device slot (opts->part / n_parts are set per slot). */
int ospf_msweep_create(ospf_multi* m, const ospf_sweep_opts* opts, ospf_msweep** out);
int ospf_msweep_destroy(ospf_msweep* ms);
/* Queue one run on every device and wait for all of them. */
int ospf_msweep_run(ospf_msweep* ms);
/* Digests of every node by node id (host [V]). With distinct devices the
 * parts' 24-B records (padded to the largest part) are all-gathered by ONE
 * RCCL ncclAllGather over xGMI (communicators from ncclCommInitAll in this
 * process, made once per ospf_multi); with a device given twice (RCCL takes
 * one rank per GPU) or OSPF_RCCL=0, peer copies onto the first device. Then
 * one scatter by root id and one copy back. OSPF_RCCL=1 takes RCCL for a
 * single device too (a one-rank communicator). */
int ospf_msweep_digests(ospf_msweep* ms, ospf_digest* out_by_node);
/* ospf_sweep_select on every part for its own roots (the parts' kernels run
 * side by side, one per device); host outputs by node id: metric / count
 * [V][P], nh [V][P][nh_words] (nh_words >= every part's max_nh_words). Errors
 * through ospf_multi_last_error. */
int ospf_msweep_select(ospf_msweep* ms, const ospf_select_table* table, uint32_t nh_words,
                       uint32_t* metric_by_node, uint32_t* count_by_node, uint32_t* nh_by_node);
/* ospf_sweep_select_policy on every part for its own roots; host outputs by
 * node id ([V][P], nh [V][P][nh_words]; any may be NULL). Nothing is written
 * unless every part succeeded. */
int ospf_msweep_select_policy(ospf_msweep* ms, const ospf_select_ptable* table, uint32_t nh_words,
                              const ospf_select_pout* out_by_node);
/* 1: this sweep's digests are gathered by RCCL, 0: by peer copies. */
uint32_t ospf_msweep_gather_backend(const ospf_msweep* ms);
/* The slot's sweep (row access, info) and the slot owning `root`. */
ospf_sweep* ospf_msweep_part(ospf_msweep* ms, uint32_t slot);
int ospf_msweep_owner(const ospf_msweep* ms, uint32_t root, uint32_t* slot);

/* Runtime statistics. spf_runs counts logical runSpf executions (one per
 * root per batch), matching the reference's decision.spf_runs counter
 * (LinkState.cpp:843). */
uint64_t ospf_spf_runs(const ospf_ctx* ctx);

/* Test hook (fault injection): the after_calls-th call from now of
 * ospf_load_graph / ospf_sssp_batch / ospf_ksp2_run / ospf_sweep_create /
 * ospf_sweep_run / ospf_sweep_copy_rows / ospf_sweep_select_dev /
 * ospf_sweep_select / ospf_msweep_select (per part) /
 * ospf_sweep_select_policy_dev / ospf_sweep_select_policy /
 * ospf_msweep_select_policy (per part) / ospf_selstate_prime /
 * ospf_selstate_update / ospf_selstate_copy / ospf_selstate_ucmp /
 * ospf_selstate_ucmp_copy / ospf_selstate_update_policy /
 * ospf_selstate_copy_policy / ospf_selstate_set_policy / ospf_areastate_prime /
 * ospf_areastate_update / ospf_areastate_copy / ospf_areastate_set_policy (on
 * any of the state's contexts) on this context fails with
 * OSPF_E_DEVICE and does nothing (0 = off). Lets the caller's handling of a
 * device error be tested without a faulting GPU. */
int ospf_inject_error(ospf_ctx* ctx, uint32_t after_calls);

/* Box calibration (no reference counterpart: measurement).
 * The HBM store rate of this device, timed with HIP events: 2 * rows * V * 4
 * bytes written with 16-B non-temporal stores per launch, `reps` timed
 * launches after one untimed one, ms_out[reps]. pattern 0 = one buffer in
 * address order; 1 = two [rows][V] u32 arrays written the way the leaf
 * launch writes its dist and next-hop rows (blocks of `group` rows x
 * `ctiles` 1,024-node tiles, chunk-major); 2 = the same blocks group-major;
 * 3 = persistent blocks (`ctiles` per CU) taking (group, tile) items in
 * group-major order (the chip walks the rows in order).
 * Allocates (and frees) its own buffer: OSPF_E_NOMEM when it does not fit.
 * V must be a multiple of 4. */
#define OSPF_PROBE_STREAM 0u
#define OSPF_PROBE_ROWS_CHUNK 1u
#define OSPF_PROBE_ROWS_GROUP 2u
#define OSPF_PROBE_ROWS_WALK 3u
int ospf_probe_store(ospf_ctx* ctx, uint32_t pattern, uint32_t V, uint32_t rows, uint32_t group,
                     uint32_t ctiles, uint32_t reps, float* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* OPENR_SPF_H */
