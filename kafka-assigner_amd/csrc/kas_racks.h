// kas_racks.h — the rack pass behind the impact pass (include/kas_abi.h: kas_rack_impact / kas_scenario_rack_impact): launch
// arguments, the host-side rack tables and the launcher the kernels' translation unit (kas_racks.hip) exports to kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same tables are built in the library and in the CPU emulation under tests/emu/.
//
// Two kernels.  kas_rack_rows_kernel: one workgroup per item of the impact pass's work list (KasImpactPlan::items, unchanged);
// it streams the item's rows, looks every cell's node and rack up and keeps the eight row sums of kas_scenario_rack_impact in
// registers; one wave_sum per field, then vector atomics into int32 [S][8] of global scratch (zero when the kernel starts).
// kas_rack_reduce_kernel: one workgroup per scenario, behind it and behind the impact pass; it folds the scenario's node
// records into R_s x 7 int32 of LDS by rack, writes the rack records and the scenario record.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "kas_abi.h"
#include "kas_impact.h"

#define KAS_RACK_BLOCK KAS_IMPACT_BLOCK     // lanes of either kernel's workgroup
#define KAS_RACK_SUMS 8                      // row sums per scenario, in kas_scenario_rack_impact's order
#define KAS_RACK_FIELDS 7                    // int32 counters per rack, in kas_rack_impact's order
#define KAS_RACK_RED 6                       // max / min words per wave of the reduce kernel
#define KAS_RACK_LDS_LIMIT KAS_IMPACT_LDS_LIMIT

// Kernel arguments: device pointers (host pointers in the emulator).
struct KasRackLaunch {
  const kas_scenario_desc* scen;
  const kas_topic_desc* topics;
  const int32_t* node_id;
  const int32_t* cur;           // int32 broker ids, or uint16 node indices (cells16)
  const int32_t* out;
  const int32_t* aux;
  const kas_topic_result* topic_results;
  const KasImpactItem* items;   // [n_items] the impact pass's work list
  const int32_t* rr;            // report racks, parallel to node_id: node i of scenario s at rr[node_off + i]
  const int64_t* node_base;     // [S] first record of the scenario's block in `nodes`
  const int64_t* rack_off;      // [S + 1] first record of the scenario's block in `racks`
  int32_t* sums;                // [S][KAS_RACK_SUMS], zero when the row kernel starts
  const kas_node_impact* nodes; // what the impact pass wrote
  kas_rack_impact* racks;
  kas_scenario_rack_impact* scenarios;
  int32_t n_items, n_scenarios;
  int32_t idmap_entries;        // direct id table: scenarios whose id range is 1 .. idmap_entries (int32 cells)
  int32_t off_rack;             // row kernel, LDS byte offset of the racks (uint16 per node) behind the id lookup at 0
  int32_t racks_in_lds;         // 0: the row kernel reads rr from global memory
  int32_t lds_bytes;            // dynamic LDS of the row kernel
  int32_t reduce_lds_bytes;     // ... of the reduce kernel: KAS_RACK_FIELDS x r_max int32, then the reduction words
  int32_t cells16;              // cur / out cells are uint16 node indices
};

// The rack tables of one batch and one report table (cached in the plan).
struct KasRackPlan {
  std::vector<int32_t> rr;      // the table the plan was built for: node_pool_len entries (compared on the next call)
  std::vector<int64_t> rack_off;   // [S + 1]
  int32_t r_max = 0;
  int32_t off_rack = 0, racks_in_lds = 1, lds_bytes = 0, reduce_lds_bytes = 0;
};

// Validate a report table against the batch and lay the rack blocks out.  table: node_pool_len entries (the caller's
// report_rack, or the batch's node_rack).  Refusals in the order include/kas_abi.h documents: a negative entry of any
// scenario's table (KAS_E_INVALID_ARG), then a scenario with more than KAS_RACK_LIMIT racks (KAS_E_UNSUPPORTED).
// n_max / idmap_entries / need_bsearch: the plan's shape (KasShape); rack_cap_limit >= 0: batches whose largest scenario has
// more nodes than this read their racks from global memory (tests: that path on small batches).
static inline int kas_rack_plan_build(const kas_batch_desc* b, const int32_t* table, int32_t n_max, int32_t idmap_entries,
                                      int32_t need_bsearch, int32_t cells16, int32_t rack_cap_limit, KasRackPlan* rp, std::string* err) {
  auto fail = [&](int code, const std::string& m) { if (err) *err = m; return code; };
  const int32_t S = b->n_scenarios > 0 ? b->n_scenarios : 0;
  for (int32_t s = 0; s < S; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    if (sd.n_nodes > 0 && (sd.node_off < 0 || sd.node_off + sd.n_nodes > b->node_pool_len || !table))
      return fail(KAS_E_INVALID_ARG, "rack pass: scenario " + std::to_string(s) + ": node table outside the node pool");
    for (int32_t i = 0; i < sd.n_nodes; ++i)
      if (table[sd.node_off + i] < 0)
        return fail(KAS_E_INVALID_ARG, "rack pass: scenario " + std::to_string(s) + ": negative rack index in the report rack table");
  }
  rp->rack_off.assign((size_t)S + 1, 0);
  rp->r_max = 0;
  for (int32_t s = 0; s < S; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    int32_t R = 0;
    for (int32_t i = 0; i < sd.n_nodes; ++i) R = table[sd.node_off + i] >= R ? table[sd.node_off + i] + 1 : R;
    if (R > KAS_RACK_LIMIT)
      return fail(KAS_E_UNSUPPORTED, "rack pass: scenario " + std::to_string(s) + ": more than KAS_RACK_LIMIT (4096) racks");
    rp->rack_off[(size_t)s + 1] = rp->rack_off[(size_t)s] + R;
    if (R > rp->r_max) rp->r_max = R;
  }
  rp->rr.assign(table, table + (b->node_pool_len > 0 ? b->node_pool_len : 0));
  // LDS of the row kernel: [id lookup][racks: uint16 per node]
  const int64_t look = kas_impact_look_bytes(n_max, idmap_entries, need_bsearch, cells16);
  const int64_t racks = kas_impact_align16(2 * (int64_t)(n_max > 0 ? n_max : 0));
  rp->racks_in_lds = look + racks <= KAS_RACK_LDS_LIMIT && !(rack_cap_limit >= 0 && n_max > rack_cap_limit) ? 1 : 0;
  rp->off_rack = (int32_t)look;
  rp->lds_bytes = (int32_t)(look + (rp->racks_in_lds ? racks : 0));
  rp->reduce_lds_bytes = (int32_t)(kas_impact_align16(4 * (int64_t)KAS_RACK_FIELDS * rp->r_max) + 4 * KAS_RACK_RED * (KAS_RACK_BLOCK / 64));
  return KAS_E_OK;
}

// Does the plan built for an earlier call serve this call's table?  The contents decide, not the pointer: a caller may hand
// over another table at the same address, or the same table at another.
static inline bool kas_rack_plan_serves(const KasRackPlan& rp, const int32_t* table, int64_t node_pool_len) {
  const size_t n = (size_t)(node_pool_len > 0 ? node_pool_len : 0);
  return rp.rr.size() == n && (n == 0 || memcmp(rp.rr.data(), table, sizeof(int32_t) * n) == 0);
}

// kas_racks.hip: the row kernel, then the reduce kernel, on `hip_stream`; `sums` must be zero over [S][KAS_RACK_SUMS] when the
// row kernel starts.  wc: the plan's width class (cells a row may hold, KasShape::Wc).  Returns a hipError_t (0 = hipSuccess).
int kas_rack_launch(const KasRackLaunch* a, int32_t wc, void* hip_stream);
