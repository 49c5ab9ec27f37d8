// knobs.h -- every environment knob of the native libraries, in one table.
//
// Header-only, no HIP: included by the engine (libopenr_spf_hip) and by the
// host LinkState mirror (libopenr_decision). The accessors take an
// enumerator of the table, so a misspelt knob is a compile error, and they
// read the environment on every call: tests and the benchmark's A/B mode set
// variables between calls on a long-lived engine, so nothing is cached.
//
// One X(name, kind, default, lo, hi, description) line per knob:
//   SET      flag, on when the variable exists, whatever its value ("=0" also
//            enables it); default / lo / hi unused
//   NONZERO  flag, on when the variable's integer value is not 0; `default`
//            holds when it is unset
//   INT      integer clamped to [lo, hi]; `default` holds when it is unset
//            (KNOB_AUTO: the caller computes it, see the description)
//   STR      the raw string, interpreted where it is read (see the description)
// DESIGN.md §9 lists the same table; tests/test_knobs.py keeps the two, and
// every knob named by a test, script or document, in step.
#pragma once

#include <climits>
#include <cstdlib>

#define KNOB_AUTO INT_MIN

// clang-format off
#define OPENR_KNOBS(X) \
  /* ---- engine: kernel variant and batch shape */ \
  X(OSPF_FORCE_VARIANT,      INT, KNOB_AUTO, INT_MIN, INT_MAX, "Force batch kernel variant 0..7 when its state fits (auto: chosen from the graph).") \
  X(OSPF_MS_NODEFER,         SET, 0, 0, 0, "Multi-source BFS writes rows per level instead of once at the end; =0 also enables it.") \
  X(OSPF_MS_PACK,            SET, 0, 0, 0, "Multi-source BFS packs several plane sets per 64-bit word; =0 also enables it.") \
  X(OSPF_MS_R,               INT, KNOB_AUTO, 1, 64, "Force the roots per multi-source batch (auto: from the neighbour bound).") \
  X(OSPF_MS_PUSH_DIV,        INT, KNOB_AUTO, 0, INT_MAX, "A level pushes when its frontier's edge mass times this is below E (auto: 8; 16 for level rows).") \
  X(OSPF_MS_NB,              INT, 96, 1, INT_MAX, "Cap on virtual batches per multi-source round.") \
  X(OSPF_MS_ILV,             NONZERO, 0, 0, 0, "When set, forces word-major staging plus interleave of wide rows on (non-zero) or off (0); unset: on for 8..64 words.") \
  X(OSPF_MS_NOMERGE,         SET, 0, 0, 0, "No merged rows kernel for 2..7-word batches; =0 also enables it.") \
  /* ---- engine: bucketed Dial (variant 7) */ \
  X(OSPF_WD_DELTA,           INT, 1, 1, INT_MAX, "Force tagged buckets of at least this many distances (1: off).") \
  X(OSPF_WD_GROUP,           INT, KNOB_AUTO, 1, 16, "Waves per root group (auto: from edges per distance value).") \
  X(OSPF_WD_NGROUPS,         INT, KNOB_AUTO, 1, INT_MAX, "Cap on root groups in flight (auto: 16 / group waves per CU).") \
  X(OSPF_WD_LIST_MB,         INT, 4096, 1, INT_MAX, "Memory budget of the frontier lists, MiB.") \
  X(OSPF_WD_BCAP,            INT, KNOB_AUTO, 1, INT_MAX, "Force the list capacity (auto: from the budget); small values exercise the overflow path.") \
  X(OSPF_WD_PACK,            INT, KNOB_AUTO, INT_MIN, INT_MAX, "Packed state field width: 0 off, 8 or 16 (auto: from the neighbour bound).") \
  X(OSPF_WD_WGSCOPE,         SET, 0, 0, 0, "Workgroup-scope state atomics in the bucketed Dial; =0 also enables it.") \
  /* ---- engine: KSP2 */ \
  X(OSPF_KSP_ROWS,           SET, 0, 0, 0, "Masked reruns as per-run rows instead of the multi-source BFS; =0 also enables it.") \
  X(OSPF_KSP_SLOTS,          INT, KNOB_AUTO, 1, INT_MAX, "Cap on the ring of rerun result slots (auto: <= 16, from memory).") \
  X(OSPF_KSP_NOHEAVY,        SET, 0, 0, 0, "No 16-wave kernel for long traces; =0 also enables it.") \
  X(OSPF_KSP_BUDGET,         INT, 256, 1, INT_MAX, "DFS steps before a trace goes to the 16-wave kernel.") \
  X(OSPF_KSP_LOOK,           INT, 16, 0, INT_MAX, "Trace lookahead: predecessor rows up to this many entries are probed (0: none).") \
  X(OSPF_KSP_D0,             INT, KNOB_AUTO, 2, INT_MAX, "Levels of the first rerun launch (auto: the depth bound); small values exercise the continuation.") \
  X(OSPF_KSP_NODECR,         SET, 0, 0, 0, "Full masked reruns for every destination, no decremental kernel; =0 also enables it.") \
  X(OSPF_KSP_DECR_BPC,       INT, KNOB_AUTO, 1, INT_MAX, "Cap on decremental blocks per CU (auto: from LDS).") \
  X(OSPF_KSP_NOPRUNE,        SET, 0, 0, 0, "No level-order pruning in the heavy decremental kernel; =0 also enables it.") \
  X(OSPF_KSP_NOSPLIT,        SET, 0, 0, 0, "No presplit of runs to the full reruns; =0 also enables it.") \
  X(OSPF_KSP_SRCCUT,         INT, 16, 0, INT_MAX, "Presplit runs that ignore more than this many of the source's links (0: off).") \
  X(OSPF_KSP_NOPRIO,         SET, 0, 0, 0, "Full reruns on the caller's stream, not a high-priority one; =0 also enables it.") \
  X(OSPF_KSP_DEBUG,          INT, 0, 0, INT_MAX, "When set, print decremental statistics; 2 and above also log the heavy runs.") \
  /* ---- engine: level rows and derive launches */ \
  X(OSPF_LV_NB,              INT, 192, 1, INT_MAX, "Cap on 128-root batches per levels round.") \
  X(OSPF_LV_SERIAL,          SET, 0, 0, 0, "Levels rows kernel on the caller's stream, no overlap with the next traversal; =0 also enables it.") \
  X(OSPF_LV_MASKED,          INT, 0, INT_MIN, INT_MAX, "Non-zero: pull scans in masked four-quad steps.") \
  X(OSPF_DERIVE_CTILES,      INT, KNOB_AUTO, 1, INT_MAX, "Tiles per block of the next-hop derive (auto: per kernel).") \
  X(OSPF_DERIVE_QUAD,        SET, 0, 0, 0, "Narrow derive (<= 4 words) on the generic quad kernel; =0 also enables it.") \
  X(OSPF_DERIVE_GENERIC,     SET, 0, 0, 0, "Wide derive (> 4 words) on the generic quad kernel; =0 also enables it.") \
  X(OSPF_DERIVE_WIDE_G,      INT, 64, 1, 64, "Roots per block of the wide derive.") \
  X(OSPF_DERIVE_WIDE1,       SET, 0, 0, 0, "Sweep: wide classes through ospf_nh_derive_dev, not the planned tile-staged kernel; =0 also enables it.") \
  X(OSPF_WIDE_BLOCKS,        INT, 8192, 1, INT_MAX, "Block target of the planned wide derive.") \
  X(OSPF_TWIN_CTILES,        INT, KNOB_AUTO, 1, INT_MAX, "Tiles per block of the twin derive (auto: one block per root).") \
  X(OSPF_TWIN_LV_BLOCKS,     INT, 2048, 1, INT_MAX, "Block target of the twin levels launch.") \
  X(OSPF_TWIN_LV_G,          INT, 8, INT_MIN, INT_MAX, "Roots per twin-levels group: 4 selects the 4-root kernel, anything else 8.") \
  X(OSPF_LEAF_CTILES,        INT, KNOB_AUTO, 1, INT_MAX, "Tiles per block of the leaf derive (auto: ~32768 blocks).") \
  X(OSPF_LEAF_GROUP_MAJOR,   NONZERO, 0, 0, 0, "When set, forces the leaf derive's block order: group-major (non-zero) or chunk-major (0), and skips the sweep's timed choice.") \
  X(OSPF_LEAF_NO_AUTO,       SET, 0, 0, 0, "Skip the sweep's timed choice of the leaf block order; =0 also enables it.") \
  X(OSPF_WD_G,               INT, KNOB_AUTO, 1, INT_MAX, "Roots per block of the weighted derives (auto: per kernel).") \
  X(OSPF_WD_CTILES,          INT, KNOB_AUTO, 1, INT_MAX, "Tiles per block of the weighted derives (auto: per kernel).") \
  X(OSPF_WD_KMAX,            INT, KNOB_AUTO, 1, INT_MAX, "Slot table width of the weighted leaf derive (auto: the caller's neighbour bound).") \
  X(OSPF_WL_CTILES,          INT, KNOB_AUTO, 1, INT_MAX, "Tiles per block of the weighted lane derive (> 4 words); overrides OSPF_WD_CTILES.") \
  X(OSPF_WW_CTILES,          INT, KNOB_AUTO, 1, INT_MAX, "Tiles per block of the weighted wide derive (<= 4 words); overrides OSPF_WD_CTILES.") \
  /* ---- engine: contracted cover and the sweep plan */ \
  X(OSPF_COVER_NOCLOSURE,    SET, 0, 0, 0, "No closure over the contracted cover graph; =0 also enables it.") \
  X(OSPF_COVER_ROWS_IN_DIAL, SET, 0, 0, 0, "Closure rows with next hops inside the cover Dial, not the rows kernel; =0 also enables it.") \
  X(OSPF_COVER_ROWS_TILED,   SET, 0, 0, 0, "Closure rows by node tiles x root chunks; =0 also enables it.") \
  X(OSPF_CLOSURE_NONH,       SET, 0, 0, 0, "Closure computes distances only; =0 also enables it.") \
  X(OSPF_SEED_NONH,          SET, 0, 0, 0, "Seeds' next hops not taken from their Dial; =0 also enables it.") \
  X(OSPF_SEED_ROWS_INLINE,   SET, 0, 0, 0, "Seeds' rows inside the Dial's launch, not on a stream of their own; =0 also enables it.") \
  X(OSPF_WCOVER_STAGE,       SET, 0, 0, 0, "Weighted cover rows in 4 stages; =0 also enables it.") \
  X(OSPF_WNH_HUB,            SET, 0, 0, 0, "Weighted next hops (<= 4 words) through the hub plan; =0 also enables it.") \
  X(OSPF_WNH_RUNS,           SET, 0, 0, 0, "Weighted next hops (> 4 words) through the runs plan; =0 also enables it.") \
  X(OSPF_MSD_MB,             INT, 65536, 64, INT_MAX, "Scratch budget of the multi-source distance kernel, MiB.") \
  X(OSPF_MSD_DELTA,          INT, KNOB_AUTO, 1, INT_MAX, "Bucket width of the multi-source distance kernel (auto: the largest metric).") \
  X(OSPF_MSD_BLOCKS,         INT, KNOB_AUTO, 1, INT_MAX, "Cap on its concurrent blocks (auto: two per CU within the budget).") \
  X(OSPF_MSD_STATS,          SET, 0, 0, 0, "Print the multi-source distance kernel's counters; =0 also enables it.") \
  X(OSPF_SWEEP_ROW_PITCH,    STR, 0, 0, 0, "A value starting with V: row pitch V; otherwise rows padded to 32 entries.") \
  X(OSPF_SWEEP_NOLEAF,       SET, 0, 0, 0, "Sweep plan without the leaf path; =0 also enables it.") \
  X(OSPF_SWEEP_NOTWIN,       SET, 0, 0, 0, "Sweep plan without twin classes; =0 also enables it.") \
  X(OSPF_SWEEP_TWIN,         SET, 0, 0, 0, "Twin derive for every class that can take it; =0 also enables it.") \
  X(OSPF_SWEEP_ALL_LEAF_ROWS, SET, 0, 0, 0, "Every leaf's level row is kept, as without twin classes; =0 also enables it.") \
  X(OSPF_SWEEP_NOTWINLV,     SET, 0, 0, 0, "No twin levels: every cover root is traversed; =0 also enables it.") \
  X(OSPF_SWEEP_TWINLV,       SET, 0, 0, 0, "Twin levels even when most cover roots need a traversal; =0 also enables it.") \
  X(OSPF_SWEEP_MERGE_REPS,   SET, 0, 0, 0, "Leaf representatives' next hops in their groups' leaf launch; =0 also enables it.") \
  X(OSPF_SWEEP_STAGES,       INT, KNOB_AUTO, 1, INT_MAX, "Stages of the staged sweep (auto: from the plan).") \
  X(OSPF_SWEEP_NO_EARLY,     SET, 0, 0, 0, "Ignore OSPF_SWEEP_EARLY_START; =0 also enables it.") \
  X(OSPF_SWEEP_NOLDS,        SET, 0, 0, 0, "Small graphs skip the in-LDS sweep; =0 also enables it.") \
  X(OSPF_SWEEP_FULL_DEPTH,   SET, 0, 0, 0, "Levels run to the depth bound, not the measured depth; =0 also enables it.") \
  X(OSPF_SWEEP_TIMING,       SET, 0, 0, 0, "Print sweep plan and run timings; =0 also enables it.") \
  X(OSPF_SWEEP_DEBUG,        SET, 0, 0, 0, "Print sweep plan decisions; =0 also enables it.") \
  X(OSPF_RCCL,               STR, 0, 0, 0, "A value starting with 0: multi-GPU digests gathered by peer copies, not RCCL.") \
  X(OSPF_ZERO_MEMSET,        SET, 0, 0, 0, "Zero with hipMemsetAsync instead of the fill kernel (read once per process); =0 also enables it.") \
  /* ---- host */ \
  X(OPENR_HOST_THREADS,      INT, KNOB_AUTO, 1, INT_MAX, "Host pool threads (auto: hardware threads, at most 16).") \
  X(ODL_HOST_SPF,            SET, 0, 0, 0, "LinkState mirror computes on the host only; =0 also enables it.") \
  X(ODL_STRICT_ENGINE,       SET, 0, 0, 0, "Engine errors are raised, no degrade to the host path; =0 also enables it.") \
  X(ODL_NO_LINK_PATCH,       SET, 0, 0, 0, "Link events rebuild the snapshot instead of patching it; =0 also enables it.") \
  X(ODL_NO_BULK_INGEST,      SET, 0, 0, 0, "Adjacency databases ingested one by one; =0 also enables it.") \
  X(ODL_NO_PREOPEN,          SET, 0, 0, 0, "Engine opened on first use, not ahead; =0 also enables it.") \
  X(ODL_KSP_CAP,             INT, KNOB_AUTO, 2, 2048, "KSP2 path record capacity (auto: from the graph).") \
  X(ODL_SPF_TIMING,          SET, 0, 0, 0, "Print LinkState SPF timings; =0 also enables it.") \
  X(ODL_SNAP_TIMING,         SET, 0, 0, 0, "Print snapshot build timings; =0 also enables it.") \
  X(ODL_ROUTE_TIMING,        SET, 0, 0, 0, "Print route build timings; =0 also enables it.")
// clang-format on

enum class KnobKind { SET, NONZERO, INT, STR };

enum class Knob {
#define X(name, kind, dflt, lo, hi, help) name,
  OPENR_KNOBS(X)
#undef X
};

struct KnobSpec {
  const char* name;
  KnobKind kind;
  int dflt, lo, hi;
};

inline const KnobSpec& knob_spec(Knob k) {
  static constexpr KnobSpec table[] = {
#define X(name, kind, dflt, lo, hi, help) {#name, KnobKind::kind, dflt, lo, hi},
      OPENR_KNOBS(X)
#undef X
  };
  return table[static_cast<int>(k)];
}

// The variable's value, or null when it is unset (any kind).
inline const char* knob_str(Knob k) { return std::getenv(knob_spec(k).name); }
inline bool knob_set(Knob k) { return knob_str(k) != nullptr; }

// SET: the variable exists. NONZERO: its value is not 0 (unset: the default).
inline bool knob_flag(Knob k) {
  const KnobSpec& s = knob_spec(k);
  const char* e = std::getenv(s.name);
  if (s.kind == KnobKind::SET) return e != nullptr;
  return e ? std::atoi(e) != 0 : s.dflt != 0;
}

// The value clamped to the table's range; `unset` when the variable is unset.
inline int knob_int(Knob k, int unset) {
  const KnobSpec& s = knob_spec(k);
  const char* e = std::getenv(s.name);
  if (!e) return unset;
  const int v = std::atoi(e);
  return v < s.lo ? s.lo : v > s.hi ? s.hi : v;
}
inline int knob_int(Knob k) { return knob_int(k, knob_spec(k).dflt); }
