// kas_impact.h — the impact pass (ABI v6, include/kas_abi.h: kas_node_impact / kas_scenario_impact): launch arguments, the
// host-side work list and the launcher the kernels' translation unit (kas_impact.hip) exports to kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same work list is built in the library and in the CPU emulation under tests/emu/.
//
// The pass runs after a solve, over the cur / out tables that solve used.  Work is a list of items, one workgroup each:
// (scenario, topic, row range).  An item counts its rows into a histogram of N x 6 int32 in the LDS, then
//   DIRECT  the scenario's only item: writes the scenario's node records and its scenario record itself;
//   FLUSH   one of several items of a scenario: adds its non-zero counters to the scenario's region of global scratch
//           (vector atomics), and kas_impact_merge_kernel — one workgroup per such scenario — writes the records from it;
//   GLOBAL  the scenario's N x 6 counters do not fit the LDS budget: every item counts straight into the scenario's region
//           (vector atomics), merged as FLUSH.
#pragma once
#include <stdint.h>

#include <vector>

#include "kas_abi.h"

#define KAS_IMPACT_BLOCK 256           // lanes of an item's workgroup (and of the merge kernel's)
#define KAS_IMPACT_FIELDS 6            // int32 counters per node, in kas_node_impact's order
#define KAS_IMPACT_EXTRA 2             // behind a histogram: departed replicas, leaders moved
#define KAS_IMPACT_LDS_LIMIT (160 * 1024)
#define KAS_IMPACT_SPLIT_BELOW 512     // batches of fewer topics than this cut large topics into row ranges
#define KAS_IMPACT_MIN_ITEM_ROWS 4096  // ... of at least this many rows
#define KAS_IMPACT_TARGET_ITEMS 256    // ... aiming at about this many items for the batch (one per CU)

enum { KAS_IMPACT_DIRECT = 0, KAS_IMPACT_FLUSH = 1, KAS_IMPACT_GLOBAL = 2 };

struct KasImpactItem {
  int32_t scen;                 // scenario (index into the plan's descriptors)
  int32_t topic;                // topic (index into the plan's descriptors), -1: a scenario without topics (writes zeros)
  int32_t row_lo, row_hi;       // rows [row_lo, row_hi) of the topic
  int32_t mode;                 // KAS_IMPACT_DIRECT / _FLUSH / _GLOBAL
  int32_t reserved;
};

// Kernel arguments: device pointers (host pointers in the emulator).
struct KasImpactLaunch {
  const kas_scenario_desc* scen;
  const kas_topic_desc* topics;
  const int32_t* node_id;
  const int32_t* cur;           // int32 broker ids, or uint16 node indices (cells16)
  const int32_t* out;
  const int32_t* aux;
  const kas_topic_result* topic_results;
  const KasImpactItem* items;   // [n_items]
  const int32_t* merge_scen;    // [n_merge] scenarios whose records kas_impact_merge_kernel writes
  const int64_t* node_base;     // [S] first record of the scenario's block in `nodes`
  const int64_t* region_off;    // [S] int32 offset of the scenario's counters in `region` (-1: DIRECT)
  int32_t* region;              // global counters of FLUSH / GLOBAL scenarios, zero when the item kernel starts
  kas_node_impact* nodes;
  kas_scenario_impact* scenarios;
  int32_t n_items, n_merge;
  int32_t node_cap;             // scenarios of at most this many nodes count in the LDS
  int32_t idmap_entries;        // direct id table: scenarios whose id range is 1 .. idmap_entries (int32 cells)
  int32_t off_look, off_red;    // LDS byte offsets: id lookup (direct table or sorted ids), reduction words
  int32_t lds_bytes;            // dynamic LDS of the item kernel
  int32_t cells16;              // cur / out cells are uint16 node indices
};

// The work list of one batch (cached in the plan).
struct KasImpactPlan {
  std::vector<KasImpactItem> items;
  std::vector<int32_t> merge_scen;
  std::vector<int64_t> node_base, region_off;
  int64_t nodes_total = 0;      // records of the nodes table: sum of n_nodes
  int64_t region_ints = 0;
  int32_t node_cap = 0, off_look = 0, off_red = 0, lds_bytes = 0;
};

static inline int64_t kas_impact_align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// Rows of an item: a topic is one item, except in batches of few topics, where topics longer than this are cut.
static inline int64_t kas_impact_rows_per_item(const kas_batch_desc* b) {
  if (b->n_topics >= KAS_IMPACT_SPLIT_BELOW) return INT32_MAX;
  int64_t total = 0;
  for (int32_t t = 0; t < b->n_topics; ++t) total += b->topics[t].n_partitions > 0 ? b->topics[t].n_partitions : 0;
  const int64_t r = (total + KAS_IMPACT_TARGET_ITEMS - 1) / KAS_IMPACT_TARGET_ITEMS;
  return r > KAS_IMPACT_MIN_ITEM_ROWS ? r : KAS_IMPACT_MIN_ITEM_ROWS;
}

// LDS bytes of the id lookup: the direct table (int16 per id of the range) or the sorted ids for a binary search
static inline int64_t kas_impact_look_bytes(int32_t n_max, int32_t idmap_entries, int32_t need_bsearch, int32_t cells16) {
  if (cells16) return 0;
  const int64_t direct = 2 * (int64_t)(idmap_entries > 0 ? idmap_entries : 0);
  const int64_t ids = need_bsearch ? 4 * (int64_t)n_max : 0;
  return kas_impact_align16(direct > ids ? direct : ids);
}

// Build the work list.  n_max / idmap_entries / need_bsearch: the plan's shape (KasShape).  node_cap_limit >= 0 lowers the
// node count up to which scenarios count in the LDS (tests: the GLOBAL path on small batches); rows_per_item: see above.
static inline void kas_impact_plan_build(const kas_batch_desc* b, int32_t n_max, int32_t idmap_entries, int32_t need_bsearch,
                                         int32_t cells16, int32_t node_cap_limit, int64_t rows_per_item, KasImpactPlan* ip) {
  const int32_t S = b->n_scenarios;
  ip->items.clear(); ip->merge_scen.clear();
  ip->node_base.assign((size_t)(S > 0 ? S : 1), 0);
  ip->region_off.assign((size_t)(S > 0 ? S : 1), -1);
  ip->nodes_total = 0; ip->region_ints = 0;
  if (rows_per_item < 1) rows_per_item = 1;
  // LDS: [histogram][id lookup][reduction words]
  const int64_t look = kas_impact_look_bytes(n_max, idmap_entries, need_bsearch, cells16);
  const int64_t red = kas_impact_align16(4 * KAS_IMPACT_FIELDS * (KAS_IMPACT_BLOCK / 64));
  int64_t cap = (KAS_IMPACT_LDS_LIMIT - look - red - 16 - 4 * KAS_IMPACT_EXTRA) / (4 * KAS_IMPACT_FIELDS);
  if (cap > n_max) cap = n_max;
  if (node_cap_limit >= 0 && cap > node_cap_limit) cap = node_cap_limit;
  if (cap < 0) cap = 0;
  ip->node_cap = (int32_t)cap;
  const int64_t hist = kas_impact_align16(4 * (KAS_IMPACT_FIELDS * cap + KAS_IMPACT_EXTRA));
  ip->off_look = (int32_t)hist;
  ip->off_red = (int32_t)(hist + look);
  ip->lds_bytes = (int32_t)(hist + look + red);
  for (int32_t s = 0; s < S; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    const int32_t N = sd.n_nodes > 0 ? sd.n_nodes : 0;
    ip->node_base[(size_t)s] = ip->nodes_total;
    ip->nodes_total += N;
    const size_t first = ip->items.size();
    if (sd.topic_count <= 0) ip->items.push_back(KasImpactItem{s, -1, 0, 0, KAS_IMPACT_DIRECT, 0});
    for (int32_t k = 0; k < sd.topic_count; ++k) {
      const int32_t t = sd.topic_begin + k;
      const int64_t P = b->topics[t].n_partitions > 0 ? b->topics[t].n_partitions : 0;
      int64_t lo = 0;
      do {
        const int64_t hi = P - lo > rows_per_item ? lo + rows_per_item : P;
        ip->items.push_back(KasImpactItem{s, t, (int32_t)lo, (int32_t)hi, KAS_IMPACT_DIRECT, 0});
        lo = hi;
      } while (lo < P);
    }
    const bool in_lds = N <= cap;
    if (in_lds && ip->items.size() - first == 1) continue;
    for (size_t i = first; i < ip->items.size(); ++i) ip->items[i].mode = in_lds ? KAS_IMPACT_FLUSH : KAS_IMPACT_GLOBAL;
    ip->region_off[(size_t)s] = ip->region_ints;
    ip->region_ints += (int64_t)KAS_IMPACT_FIELDS * N + KAS_IMPACT_EXTRA;
    ip->merge_scen.push_back(s);
  }
}

// kas_impact.hip: the item kernel, then (n_merge > 0) the merge kernel, on `hip_stream`; `region` must be zero over the
// work list's region_ints when the item kernel starts.  wc: the plan's width class (cells a row may hold, KasShape::Wc).
// Returns a hipError_t (0 = hipSuccess).
int kas_impact_launch(const KasImpactLaunch* a, int32_t wc, void* hip_stream);
