// kas_topics.h — the topic pass (include/kas_abi.h: kas_topic_impact / kas_scenario_topic_impact): launch arguments, the
// host-side work list and the launcher the kernels' translation unit (kas_topics.hip) exports to kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same work list is built in the library and in the CPU emulation under tests/emu/.
//
// The pass runs after a solve, over the cur / out tables that solve used; it needs nothing of the impact pass.  Work is a list
// of items cut by the impact pass's rule (kas_impact_rows_per_item), one workgroup each: (scenario, topic, row range).  An item
// counts its rows into a histogram of N x 4 int32 in the LDS (replicas after, leaders after, inbound, outbound; two words behind
// it: departed replicas, leaders moved), then — the mode is the TOPIC's, not the scenario's —
//   DIRECT  the topic's only item: reduces max / min over the histogram and writes the topic's record itself;
//   FLUSH   one of several items of a topic: adds its non-zero counters to the topic's region of global scratch (vector
//           atomics), and kas_topic_merge_kernel — one workgroup per such topic — writes the record from it;
//   GLOBAL  the scenario's N x 4 counters do not fit the LDS budget: the item counts straight into the topic's region (vector
//           atomics), merged as FLUSH.
// kas_topic_summary_kernel, one workgroup per scenario behind both, folds the topic records and kas_topic_result into the
// scenario's sixteen words.
#pragma once
#include <stdint.h>

#include <vector>

#include "kas_abi.h"
#include "kas_impact.h"

#define KAS_TOPIC_BLOCK KAS_IMPACT_BLOCK     // lanes of every kernel's workgroup
#define KAS_TOPIC_FIELDS 4                   // int32 counters per node: replicas after, leaders after, inbound, outbound
#define KAS_TOPIC_EXTRA 2                    // behind a histogram: departed replicas, leaders moved
#define KAS_TOPIC_RED 6                      // max / min words per wave when a topic's record is written
#define KAS_TOPIC_WORDS 16                   // int32 words of kas_scenario_topic_impact
#define KAS_TOPIC_LDS_LIMIT KAS_IMPACT_LDS_LIMIT

enum { KAS_TOPIC_DIRECT = KAS_IMPACT_DIRECT, KAS_TOPIC_FLUSH = KAS_IMPACT_FLUSH, KAS_TOPIC_GLOBAL = KAS_IMPACT_GLOBAL };

// a topic whose record kas_topic_merge_kernel writes
struct KasTopicMerge {
  int32_t topic, scen;
};

// Kernel arguments: device pointers (host pointers in the emulator).
struct KasTopicLaunch {
  const kas_scenario_desc* scen;
  const kas_topic_desc* topics;
  const int32_t* node_id;
  const int32_t* cur;           // int32 broker ids, or uint16 node indices (cells16)
  const int32_t* out;
  const int32_t* aux;
  const kas_topic_result* topic_results;
  const KasImpactItem* items;   // [n_items]; mode: KAS_TOPIC_DIRECT / _FLUSH / _GLOBAL of the item's topic
  const KasTopicMerge* merge;   // [n_merge] topics whose records kas_topic_merge_kernel writes
  const int64_t* region_off;    // [T] int32 offset of the topic's counters in `region` (-1: DIRECT)
  int32_t* region;              // global counters of FLUSH / GLOBAL topics, zero when the item kernel starts
  kas_topic_impact* topic_out;  // [T]
  kas_scenario_topic_impact* scenarios;   // [S]
  int32_t n_items, n_merge, n_scenarios;
  int32_t idmap_entries;        // direct id table: scenarios whose id range is 1 .. idmap_entries (int32 cells)
  int32_t off_look, off_red;    // LDS byte offsets: id lookup (direct table or sorted ids), reduction words
  int32_t lds_bytes;            // dynamic LDS of the item kernel
  int32_t cells16;              // cur / out cells are uint16 node indices
};

// The work list of one batch (cached in the plan).
struct KasTopicPlan {
  std::vector<KasImpactItem> items;
  std::vector<KasTopicMerge> merge;
  std::vector<int64_t> region_off;   // [T]
  int64_t region_ints = 0;
  int32_t node_cap = 0, off_look = 0, off_red = 0, lds_bytes = 0;
};

// Build the work list.  n_max / idmap_entries / need_bsearch: the plan's shape (KasShape).  node_cap_limit >= 0 lowers the node
// count up to which topics count in the LDS (tests: the GLOBAL path on small batches); rows_per_item: kas_impact_rows_per_item.
static inline void kas_topic_plan_build(const kas_batch_desc* b, int32_t n_max, int32_t idmap_entries, int32_t need_bsearch,
                                        int32_t cells16, int32_t node_cap_limit, int64_t rows_per_item, KasTopicPlan* tp) {
  const int32_t S = b->n_scenarios, T = b->n_topics;
  tp->items.clear(); tp->merge.clear();
  tp->region_off.assign((size_t)(T > 0 ? T : 1), -1);
  tp->region_ints = 0;
  if (rows_per_item < 1) rows_per_item = 1;
  // LDS: [histogram][id lookup][reduction words]
  const int64_t look = kas_impact_look_bytes(n_max, idmap_entries, need_bsearch, cells16);
  const int64_t red = kas_impact_align16(4 * KAS_TOPIC_RED * (KAS_TOPIC_BLOCK / 64));
  int64_t cap = (KAS_TOPIC_LDS_LIMIT - look - red - 16 - 4 * KAS_TOPIC_EXTRA) / (4 * KAS_TOPIC_FIELDS);
  if (cap > n_max) cap = n_max;
  if (node_cap_limit >= 0 && cap > node_cap_limit) cap = node_cap_limit;
  if (cap < 0) cap = 0;
  tp->node_cap = (int32_t)cap;
  const int64_t hist = kas_impact_align16(4 * (KAS_TOPIC_FIELDS * cap + KAS_TOPIC_EXTRA));
  tp->off_look = (int32_t)hist;
  tp->off_red = (int32_t)(hist + look);
  tp->lds_bytes = (int32_t)(hist + look + red);
  for (int32_t s = 0; s < S; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    const int32_t N = sd.n_nodes > 0 ? sd.n_nodes : 0;
    const bool in_lds = N <= cap;
    for (int32_t k = 0; k < sd.topic_count; ++k) {
      const int32_t t = sd.topic_begin + k;
      const int64_t P = b->topics[t].n_partitions > 0 ? b->topics[t].n_partitions : 0;
      const size_t first = tp->items.size();
      int64_t lo = 0;
      do {
        const int64_t hi = P - lo > rows_per_item ? lo + rows_per_item : P;
        tp->items.push_back(KasImpactItem{s, t, (int32_t)lo, (int32_t)hi, KAS_TOPIC_DIRECT, 0});
        lo = hi;
      } while (lo < P);
      if (in_lds && tp->items.size() - first == 1) continue;
      for (size_t i = first; i < tp->items.size(); ++i) tp->items[i].mode = in_lds ? KAS_TOPIC_FLUSH : KAS_TOPIC_GLOBAL;
      tp->region_off[(size_t)t] = tp->region_ints;
      tp->region_ints += (int64_t)KAS_TOPIC_FIELDS * N + KAS_TOPIC_EXTRA;
      tp->merge.push_back(KasTopicMerge{t, s});
    }
  }
}

// The refusal of include/kas_abi.h: the pass's global counters beyond KAS_TOPIC_SCRATCH_LIMIT bytes.
static inline bool kas_topic_scratch_ok(const KasTopicPlan& tp) {
  return tp.region_ints <= (int64_t)(KAS_TOPIC_SCRATCH_LIMIT / 4);
}
#define KAS_TOPIC_SCRATCH_TEXT "topic pass: the global counters of the batch's cut and large-scenario topics exceed KAS_TOPIC_SCRATCH_LIMIT"

// kas_topics.hip: the item kernel, then (n_merge > 0) the merge kernel, then the summary kernel, on `hip_stream`; `region` must be
// zero over the work list's region_ints when the item kernel starts.  wc: the plan's width class (cells a row may hold,
// KasShape::Wc).  Returns a hipError_t (0 = hipSuccess).
int kas_topic_launch(const KasTopicLaunch* a, int32_t wc, void* hip_stream);
