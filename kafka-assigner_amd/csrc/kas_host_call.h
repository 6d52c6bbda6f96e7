// kas_host_call.h — what a host call (kas_solve_host*, kas_solve_host_sharded) will do, decided ONCE and on the CPU.
//
// Pure host C++ (no HIP calls, no environment).  kas_plan_host_call() turns a call's arguments into a KasHostCall: the batch the
// kernels see, its shape, the cell width it is solved on, where selected rows and impact records go, the scenario ranges and the
// byte size of every buffer the call needs.  The library (kas_hip.hip) reserves, enqueues and drains from that value and holds no
// decision of its own; the CPU emulator (tests/emu/emu_driver.cpp) exports the same functions to tests/test_host_call.py.
// Also here: the slicing arithmetic behind kas_shard_range / kas_batch_slice and the pure half of the host path's plan cache.
// Include behind kas_solver_body.h, as kas_launch_plan.h asks.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "kas_plan_math.h"
#include "kas_launch_plan.h"   // kas_cells16_ok, KAS_BUILT_*
#include "kas_choose.h"        // the size and segment tables of kas_solve_host_choose
#include "kas_moves.h"         // the scenario and segment tables of kas_solve_host_moves / kas_solve_host_choose_moves
#include "kas_front.h"         // the spec of kas_solve_host_front
#include "kas_racks.h"         // the rack tables of kas_solve_host_rack_impact
#include "kas_topics.h"        // the work list of kas_solve_host_topic_impact (its scratch decides a refusal)
#include "kas_batches.h"       // the refusals and the LDS layout of kas_solve_host_batches
#include "kas_rounds.h"        // ... and of kas_solve_host_rounds

#ifndef KAS_HOST_STREAMS
#define KAS_HOST_STREAMS 8   // (round 4: 3 -> 8, a chain per scenario range: 11.0k -> 12.9k scenarios/s through kas_solve_host, gpurun_out/r4n)
#endif
#define KAS_HOST_PLAN_CACHE 16
#define KAS_HOST_SPLIT_MIN_BYTES (48ll << 20)   // tables smaller than this are moved and solved as one range
// Scenario ranges of one call.  A range's solve is a chain of ~2.5-3 ms however few scenarios it holds (one workgroup per
// scenario walks its 100,000 rows), so a call lasts upload + that chain + the last range's download, and more ranges only
// shorten the last download — while the runtime maps the ranges' solve streams onto GPU_MAX_HW_QUEUES (default 4) hardware
// queues shared with everything else, where ranges on one queue run one after the other (a kernel + copy trace of eight
// ranges: the last one solved alone, 3.4 ms after the others).  240 scenarios x 100,000 x 3 cells, 16-bit cells, pinned:
// 2 ranges 6.4 ms, 3: 6.0, 4: 7.1 (5.9 with eight hardware queues), 8: 7.8; int32 cells 9.3-10.0 ms whatever the count
// (scripts/e2e_host_path.py; KAS_HOST_RANGES overrides for such measurements).
#define KAS_HOST_SPLIT_MAX 3
static_assert(KAS_HOST_SPLIT_MAX <= KAS_HOST_STREAMS, "one event pair per scenario range");

// ---- slicing ------------------------------------------------------------------------------------------------------------
// kas_shard_range (include/kas_abi.h)
static inline void kas_range_of(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi) {
  if (world < 1) world = 1;
  if (rank < 0) rank = 0;
  if (rank >= world) rank = world - 1;
  if (total < 0) total = 0;
  const int64_t base = total / world, rem = total % world;
  const int64_t l = (int64_t)rank * base + (rank < rem ? rank : rem);
  if (lo) *lo = l;
  if (hi) *hi = l + base + (rank < rem ? 1 : 0);
}

// the tables of a slice that begins at this topic and scenario: the pools as they are, the slice's result records
static inline kas_tables kas_tables_at(kas_tables t, int64_t topic, int64_t scenario) {
  if (t.topic_results) t.topic_results += topic;
  if (t.scenario_results) t.scenario_results += scenario;
  return t;
}

// kas_batch_slice (include/kas_abi.h)
static inline int kas_slice_batch(const kas_batch_desc* b, int64_t lo, int64_t hi, kas_scenario_desc* scratch, kas_batch_desc* out,
                                  const kas_tables* tables, kas_tables* tables_out, std::string* err) {
  auto fail = [&](const std::string& m) { if (err) *err = m; return KAS_E_INVALID_ARG; };
  if (!b || !out || lo < 0 || hi < lo || hi > b->n_scenarios || (hi > lo && (!scratch || !b->scenarios)))
    return fail("kas_batch_slice: bad range / NULL argument");
  int64_t tlo = INT64_MAX, thi = 0, nlo = INT64_MAX, nhi = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const kas_scenario_desc& sd = b->scenarios[i];
    if (sd.topic_begin < 0 || sd.topic_count < 0 || (int64_t)sd.topic_begin + sd.topic_count > b->n_topics || sd.n_nodes < 0 ||
        sd.node_off < 0 || sd.node_off + sd.n_nodes > b->node_pool_len)
      return fail("kas_batch_slice: scenario " + std::to_string(i) + " refers outside the batch");
    if (sd.topic_count > 0) {
      if (sd.topic_begin < tlo) tlo = sd.topic_begin;
      if ((int64_t)sd.topic_begin + sd.topic_count > thi) thi = (int64_t)sd.topic_begin + sd.topic_count;
    }
    if (sd.n_nodes > 0) {
      if (sd.node_off < nlo) nlo = sd.node_off;
      if (sd.node_off + sd.n_nodes > nhi) nhi = sd.node_off + sd.n_nodes;
    }
  }
  if (tlo > thi) tlo = thi = 0;
  if (nlo > nhi) nlo = nhi = 0;
  for (int64_t i = lo; i < hi; ++i) {
    kas_scenario_desc sd = b->scenarios[i];
    sd.topic_begin = sd.topic_count > 0 ? (int32_t)(sd.topic_begin - tlo) : 0;
    sd.node_off = sd.n_nodes > 0 ? sd.node_off - nlo : 0;
    scratch[i - lo] = sd;
  }
  out->n_scenarios = (int32_t)(hi - lo);
  out->n_topics = (int32_t)(thi - tlo);
  out->scenarios = scratch;
  out->topics = b->topics ? b->topics + tlo : nullptr;
  out->node_id = b->node_id ? b->node_id + nlo : nullptr;
  out->node_rack = b->node_rack ? b->node_rack + nlo : nullptr;
  out->node_pool_len = nhi - nlo;
  if (tables && tables_out) *tables_out = kas_tables_at(*tables, tlo, lo);
  return KAS_E_OK;
}

// One scenario range of a batch — a range of a host call, a shard of kas_solve_host_sharded: its slice, and the stretches of the
// pools it touches
struct KasExtent { int64_t lo = 0, hi = 0; };
enum KasPool { KAS_POOL_TOPICS, KAS_POOL_CUR, KAS_POOL_OUT, KAS_POOL_CTX, KAS_POOLS };
struct KasHostRange {
  int64_t lo = 0, hi = 0;                       // scenarios
  std::vector<kas_scenario_desc> scen;          // rebased descriptors of the slice
  kas_batch_desc bd{};
  KasExtent own[KAS_POOLS];                     // topics (absolute indices), cur, out, ctx
};

// [0, n_scenarios) cut into K ranges (kas_range_of), each sliced and — unless it is the whole batch, whose shape the caller has —
// shaped for its extents (an empty one of several is left as it is: all zero).  A KAS_E_* and its text; *bad: the range that was refused.
static inline int kas_cut_ranges(const kas_batch_desc* b, int32_t K, const KasShape* whole, std::vector<KasHostRange>* out, std::string* err,
                                 int32_t* bad = nullptr) {
  out->assign((size_t)K, KasHostRange());
  for (int32_t i = 0; i < K; ++i) {
    KasHostRange& r = (*out)[(size_t)i];
    if (bad) *bad = i;
    kas_range_of(b->n_scenarios, i, K, &r.lo, &r.hi);
    if (r.hi <= r.lo && K > 1) continue;
    r.scen.resize((size_t)(r.hi - r.lo) + 1);
    int rc = kas_slice_batch(b, r.lo, r.hi, r.scen.data(), &r.bd, nullptr, nullptr, err);
    if (rc != KAS_E_OK) return rc;
    const int64_t tlo = r.bd.topics ? (int64_t)(r.bd.topics - b->topics) : 0;
    r.own[KAS_POOL_TOPICS] = {tlo, tlo + r.bd.n_topics};
    KasShape own;
    if (!(K == 1 && whole) && (rc = kas_shape_batch(&r.bd, &own, err, 0, 0)) != KAS_E_OK) return rc;
    const KasShape& sh = K == 1 && whole ? *whole : own;
    r.own[KAS_POOL_CUR] = {sh.cur_lo, sh.cur_need};
    r.own[KAS_POOL_OUT] = {sh.out_lo, sh.out_need};
    r.own[KAS_POOL_CTX] = {sh.ctx_lo, sh.ctx_need};
  }
  return KAS_E_OK;
}

// Do the ranges own ascending, disjoint stretches of every pool in `pools` (bits 1 << KasPool)?  Ranges that do may be moved and
// solved independently: no copy of one overwrites what another delivered.  `empty_counts`: an empty stretch must lie in line as
// well (the ranges of a host call); else it is passed over (the shards of kas_solve_host_sharded).
static inline bool kas_ranges_disjoint(const std::vector<KasHostRange>& ranges, uint32_t pools, bool empty_counts) {
  for (int32_t p = 0; p < KAS_POOLS; ++p) {
    if (!((pools >> p) & 1u)) continue;
    int64_t end = INT64_MIN;
    for (const KasHostRange& r : ranges) {
      const KasExtent& e = r.own[p];
      if (e.hi <= e.lo && !empty_counts) continue;
      if (e.lo < end) return false;
      end = e.hi;
    }
  }
  return true;
}

// 16-bit cells are node indices: the node table the kernels see gives node i the id i (`ids` holds it, `out` = *b with it).
// `ids` may be a table an earlier call filled (the context's): it is rewritten only where the scenarios' node ranges
// differ from the ones it was filled for (`stamp`: a hash of them) — a what-if caller's 1000 x 1000 table stays.
static inline int kas_ident_batch(const kas_batch_desc* b, std::vector<int32_t>* ids, kas_batch_desc* out, uint64_t* stamp, std::string* err) {
  auto fail = [&](int code, const std::string& m) { if (err) *err = m; return code; };
  if (b->n_scenarios < 0 || b->node_pool_len < 0 || (b->n_scenarios > 0 && !b->scenarios))
    return fail(KAS_E_INVALID_ARG, "negative size / scenarios == NULL");
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)b->node_pool_len;
  for (int32_t s = 0; s < b->n_scenarios; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    if (sd.n_nodes < 0 || sd.node_off < 0 || sd.node_off + sd.n_nodes > b->node_pool_len)
      return fail(KAS_E_INVALID_ARG, "scenario " + std::to_string(s) + ": node table outside the node pool");
    // (a cell's bit 15 says "no holder" inside the kernels, mid_to_index: an index is below 32,768 — KAS_N_LIMIT, the
    // limit of every plan; 0xFFFF is the only cell value above it that means anything)
    if (sd.n_nodes > KAS_N_LIMIT)
      return fail(KAS_E_UNSUPPORTED, "scenario " + std::to_string(s) + ": more than 32,767 brokers do not fit 16-bit cells");
    h = (h ^ (((uint64_t)(uint32_t)sd.node_off << 32) | (uint32_t)sd.n_nodes)) * 0x100000001b3ull;
    h ^= h >> 29;
  }
  h |= 1ull;
  if (!(stamp && *stamp == h && ids->size() == (size_t)b->node_pool_len)) {
    ids->assign((size_t)b->node_pool_len, 0);
    for (int32_t s = 0; s < b->n_scenarios; ++s) {
      const kas_scenario_desc& sd = b->scenarios[s];
      for (int32_t i = 0; i < sd.n_nodes; ++i) (*ids)[(size_t)(sd.node_off + i)] = i;
    }
    if (stamp) *stamp = h;
  }
  *out = *b;
  out->node_id = ids->data();
  return KAS_E_OK;
}

// ---- a host call ----------------------------------------------------------------------------------------------------------
// the buffers of a context's host path, in the order they are reserved
enum KasHostBuf {
  KAS_HB_CUR, KAS_HB_OUT, KAS_HB_AUX, KAS_HB_CTX,   // int32 pools on the device
  KAS_HB_CUR16, KAS_HB_OUT16,                       // the 16-bit cells of kas_solve_host16 as they travel (widened / narrowed on the device)
  KAS_HB_TR, KAS_HB_SR,                             // result records on the device
  KAS_HB_TR_PIN, KAS_HB_SR_PIN,                     // ... and their pinned HOST staging
  KAS_HB_IMP_NODES, KAS_HB_IMP_SCEN,                // the impact records of kas_solve_host_impact / 16 on the device
  KAS_HB_COUNT,                                     // the buffers any host call may use end here
  // kas_solve_host_choose / 16 alone (behind KAS_HB_COUNT: whoever lists the buffers above still lists all of them)
  KAS_HB_CH_SIZES = KAS_HB_COUNT, KAS_HB_CH_SEGS,   // the size and segment tables (kas_choose.h) on the device
  KAS_HB_CH_HEAD, KAS_HB_CH_ROWS, KAS_HB_CH_NODES,  // row_off, node_off, rank, chosen, n_ok; the chosen scenarios' packed rows and node blocks
  KAS_HB_CH_HEAD_PIN, KAS_HB_CH_ROWS_PIN, KAS_HB_CH_NODES_PIN,   // ... and their pinned HOST staging
  KAS_HB_TOTAL,                                     // the buffers of the calls above end here
  // kas_solve_host_moves / kas_solve_host_choose_moves / 16 alone (behind KAS_HB_TOTAL, for the same reason)
  KAS_HB_MV_SCEN = KAS_HB_TOTAL, KAS_HB_MV_SEGS,    // the scenario and segment tables (kas_moves.h) on the device
  KAS_HB_MV_SELECT, KAS_HB_MV_SCRATCH,              // the list (a host list; a choice's list is its chosen[]), the (listed scenario, item) table
  KAS_HB_MV_HEAD, KAS_HB_MV_MOVES, KAS_HB_MV_CELLS, // move_off and cell_off; the records and their list cells
  KAS_HB_MV_SIZES0,                                 // a choice without rows: the choose size table with no cells, for the gather
  KAS_HB_MV_HEAD_PIN,                               // pinned HOST staging of the offsets (records and cells go straight to the caller: exactly what was written)
  KAS_HB_ALL,                                       // the buffers of the calls above end here
  // kas_solve_host_front / 16 alone (behind KAS_HB_ALL, for the same reason)
  KAS_HB_FR_CLS = KAS_HB_ALL,                       // the classes the mark kernel leaves for the front rank kernel
  KAS_HB_FR_COUNTS, KAS_HB_FR_COUNTS_PIN,           // n_ok, n_eligible, n_front, 0 and their pinned HOST staging
  KAS_HB_END,                                       // the buffers of the calls above end here
  // kas_solve_host_rack_impact / 16 alone (behind KAS_HB_END, for the same reason)
  KAS_HB_RK_RACKS = KAS_HB_END, KAS_HB_RK_SCEN,     // the rack records and the scenario rack records on the device
  KAS_HB_LAST,                                      // the buffers of the calls above end here
  // kas_solve_host_topic_impact / 16 alone (behind KAS_HB_LAST, for the same reason)
  KAS_HB_TP_TOPICS = KAS_HB_LAST, KAS_HB_TP_SCEN,   // the topic records and the scenario topic records on the device
  KAS_HB_EVERY,                                     // the buffers of the calls above end here
  // kas_solve_host_batches / 16 alone (behind KAS_HB_EVERY, for the same reason; the moves pass's scenario and segment tables
  // go where a moves call puts them, KAS_HB_MV_SCEN / KAS_HB_MV_SEGS)
  KAS_HB_BT_SDESC = KAS_HB_EVERY, KAS_HB_BT_NODE_ID, // the scenario descriptors and (int32 cells) the node id tables of the whole call
  KAS_HB_BT_SELECT,                                 // the list
  KAS_HB_BT_SCEN, KAS_HB_BT_BATCHES,                // the scenario records and the batch records on the device
  KAS_HB_FINAL,                                     // the buffers of the calls above end here
  // kas_solve_host_rounds / 16 alone (behind KAS_HB_FINAL, for the same reason; its tables, descriptors, node ids and list go
  // where a batches call puts them: KAS_HB_MV_SCEN / _SEGS, KAS_HB_BT_SDESC / _NODE_ID / _SELECT)
  KAS_HB_RD_SCEN = KAS_HB_FINAL, KAS_HB_RD_ROUNDS, KAS_HB_RD_OF,   // the scenario records, the round records and round_of on the device
  KAS_HB_BUFFERS
};
static inline bool kas_host_buf_pinned(int32_t id) {
  return id == KAS_HB_TR_PIN || id == KAS_HB_SR_PIN || id == KAS_HB_CH_HEAD_PIN || id == KAS_HB_CH_ROWS_PIN || id == KAS_HB_CH_NODES_PIN ||
         id == KAS_HB_MV_HEAD_PIN || id == KAS_HB_FR_COUNTS_PIN;
}

// everything the decisions read
struct KasHostCallIn {
  const kas_batch_desc* batch = nullptr;
  int64_t cur_len = 0, out_len = 0, aux_len = 0, ctx_len = 0;   // kas_tables: the pool lengths, and which tables are there
  bool have_cur = false, have_out = false, have_aux = false, have_ctx = false, have_topic_results = false, have_scenario_results = false;
  const int32_t* select = nullptr;
  int32_t n_select = -1;                        // < 0: every scenario's rows come back where the descriptors say
  bool cells16 = false;                         // cur / out travel as 16-bit node indices
  std::vector<int32_t>* ident_ids = nullptr;    // ... the identity id table of such a call and its stamp (kas_ident_batch): the context's
  uint64_t* ident_stamp = nullptr;
  bool impact = false, have_imp_nodes = false, have_imp_scenarios = false;   // kas_impact_tables
  // kas_solve_host_choose / 16: rows and node blocks come back for the spec's k best scenarios only (n_select is then 0 and impact set)
  const kas_choose_spec* choose = nullptr;
  int64_t rows_cap = 0, nodes_cap = 0;          // kas_choice
  bool have_ch_rank = false, have_ch_chosen = false, have_ch_row_off = false, have_ch_node_off = false, have_ch_n_ok = false,
       have_ch_rows = false, have_ch_nodes = false;
  // kas_solve_host_moves / kas_solve_host_choose_moves / 16: the moves of a list of scenarios come back (defaults: no moves, and
  // every decision above as it was).  Without `choose` the list is mv_select[0 .. mv_n_select) (host; < 0: every scenario) and
  // no rows come back (n_select is 0); with `choose` it is the choice's chosen[0 .. k), and ch_rows_optional lets the caller
  // leave the rows out (rows == NULL with rows_cap == 0)
  const kas_moves* moves = nullptr;
  const int32_t* mv_select = nullptr;
  int32_t mv_n_select = -1;
  bool ch_rows_optional = false;
  // kas_solve_host_front / 16: the front in place of the ranking (`choose` is then not read: the front's criteria and k take its
  // place in every decision above; ch_rows_optional as in a choice with moves, and `moves` may be left out)
  const kas_front_spec* front = nullptr;
  bool have_fr_counts = false;
  // kas_solve_host_rack_impact / 16: the rack pass behind the impact pass (defaults: no rack pass, and every decision above as
  // it was).  report_rack: the caller's table or NULL (the batch's node_rack); with `racks` the node records may stay on the
  // device (have_imp_nodes false)
  bool racks = false;
  const int32_t* report_rack = nullptr;
  int64_t racks_cap = 0;                        // kas_rack_tables
  bool have_rk_racks = false, have_rk_scenarios = false, have_rk_off = false;
  // kas_solve_host_choose_racks / kas_solve_host_front_racks / 16: `racks` together with `choose` or `front` (the rack refusals then
  // follow the choice's and the moves'), and rack_keys: the spec may name rack criteria (KAS_KEY_RACK_BASE), which need `racks`;
  // the spec's refusals then come first, as a front's always do.  Defaults: every decision above as it was.
  bool rack_keys = false;
  // kas_solve_host_topic_impact / 16: the topic pass behind the solve, with the impact pass (`impact`) or without it (defaults:
  // no topic pass, and every decision above as it was); with `topics` the node records may stay on the device, as with `racks`
  bool topics = false;
  bool have_tp_tables = false, have_tp_topics = false, have_tp_scenarios = false;   // kas_topic_impact_tables
  // kas_solve_host_choose_topics / kas_solve_host_front_topics / 16: `topics` together with `choose` or `front` (the topic refusals
  // then follow the rack pass's, which follow the choice's and the moves'), and topic_keys beside rack_keys: the spec may name
  // topic criteria (KAS_KEY_TOPIC_BASE), which need `topics`.  Defaults: every decision above as it was.
  bool topic_keys = false;
  // kas_solve_host_batches / 16: the batches pass behind the solve, for the list bt_select[0 .. bt_n_select) (host; < 0: every
  // scenario); no rows come back (n_select is 0).  Defaults: no batches pass, and every decision above as it was.
  const kas_batch_spec* batches = nullptr;
  const kas_batches* bt_out = nullptr;
  const int32_t* bt_select = nullptr;
  int32_t bt_n_select = -1;
  // kas_solve_host_rounds / 16: the rounds pass behind the solve, for the list rd_select[0 .. rd_n_select) (host; < 0: every
  // scenario); no rows come back (n_select is 0).  Defaults: no rounds pass, and every decision above as it was.
  const kas_round_spec* rounds = nullptr;
  const kas_rounds* rd_out = nullptr;
  const int32_t* rd_select = nullptr;
  int32_t rd_n_select = -1;
  int32_t lane_order_ok = 1;                    // the context's LDS lane-order verdict
  uint32_t built16[KAS_MAX_WIDTH + 1];          // [width class] the kernel families the build holds for 16-bit cells (KAS_BUILT_*)
  int32_t ranges_override = 0;                  // KAS_HOST_RANGES (0: not set)
  KasHostCallIn() { for (uint32_t& m : built16) m = KAS_BUILT_ALL; }
};

// The header of a choice as it lies in KAS_HB_CH_HEAD and its staging: byte offsets, the int64 arrays first.
struct KasChooseHead {
  size_t row_off = 0, node_off = 0, rank = 0, chosen = 0, n_ok = 0, bytes = 0;
  void lay_out(int64_t S, int64_t k) {
    row_off = 0;
    node_off = row_off + 8 * (size_t)(k + 1);
    rank = node_off + 8 * (size_t)(k + 1);
    chosen = rank + 4 * (size_t)S;
    n_ok = chosen + 4 * (size_t)k;
    bytes = n_ok + 4;
  }
};

struct KasHostCall {
  kas_batch_desc batch{};                       // the batch the kernels see (a 16-bit call: with the identity id table)
  KasShape full;                                // ... validated, with the extents of every pool
  bool all_rows = true;
  bool native16 = false;                        // a 16-bit call solved on its own cells (what kas_plan_create16 accepts)
  bool need32 = true;                           // int32 cell pools on the device: every other call
  std::vector<int64_t> sel_off;                 // [n_select + 1] where each selected scenario's rows go, packed (cells)
  std::vector<int64_t> imp_base;                // [S + 1] impact records: scenario s's node block starts at the sum of the n_nodes before it
  int32_t K = 1;
  std::vector<KasHostRange> ranges;             // [K]
  size_t bytes[KAS_HB_BUFFERS] = {};              // what to reserve of each buffer; 0: this call must not touch it
  // kas_solve_host_choose / 16
  KasChoosePlan choose;                         // the size table and the segment table of the whole call, offsets as the device sees `out`
  int64_t ch_rows_need = 0, ch_nodes_need = 0;  // what the k largest scenarios take: cells, node records
  int64_t ch_chunks = 0;                        // gather workgroups per chosen scenario
  KasChooseHead ch_head;                        // where the arrays of the header lie in KAS_HB_CH_HEAD
  bool ch_gather_rows = true;                   // false: kas_solve_host_choose_moves without rows
  kas_choose_spec ch_spec{};                    // the spec every choose decision was made from: the caller's, or a front's criteria and k
  // kas_solve_host_moves / kas_solve_host_choose_moves / 16
  KasMovesPlan moves;                           // the scenario and segment tables of the whole call, offsets as the device sees the pools
  std::vector<int32_t> mv_list;                 // the list as it is uploaded (empty for a choice: its chosen[] is on the device)
  int64_t mv_n = 0;                             // listed scenarios
  int64_t mv_room_moves = 0, mv_room_cells = 0; // what the list can need at most (a choice: the k largest scenarios)
  int64_t mv_moves_cap = 0, mv_cells_cap = 0;   // the capacities on the device: the caller's, no more than the room
  // kas_solve_host_rack_impact / 16
  KasRackPlan rack;                             // the report table and rack_off of the whole call
  // kas_solve_host_topic_impact / 16
  int64_t tp_region_ints = 0;                   // global counters the pass needs over the whole batch (the ranges' plans hold their own)
  // kas_solve_host_batches / 16 (its segment tables are `moves`)
  std::vector<int32_t> bt_list;                 // the list as it is uploaded
  int64_t bt_n = 0;                             // listed scenarios
  int32_t bt_n_cap = 0;                         // the most nodes of a listed scenario
  // kas_solve_host_rounds / 16 (its segment tables are `moves`)
  std::vector<int32_t> rd_list;                 // the list as it is uploaded
  int64_t rd_n = 0;                             // listed scenarios
  int32_t rd_n_cap = 0;                         // the most nodes of a listed scenario
};

// Scenario ranges of a call that moves `bytes` of cells for S scenarios.  Large tables laid out scenario by scenario are cut so
// that the upload of one range, the solve of the previous one and the download of the one before overlap.
static inline int32_t kas_host_range_count(int64_t bytes, int64_t S, int32_t ranges_override) {
  if (bytes < KAS_HOST_SPLIT_MIN_BYTES || S < 2) return 1;
  int64_t K = bytes / (KAS_HOST_SPLIT_MIN_BYTES / 2);
  if (K > KAS_HOST_SPLIT_MAX) K = KAS_HOST_SPLIT_MAX;
  if (ranges_override >= 1 && ranges_override <= KAS_HOST_STREAMS) K = ranges_override;
  return (int32_t)(K > S ? S : K);
}

// Validate a host call and decide everything about it.  Returns KAS_E_* and fills err; the checks run in the order callers know.
static inline int kas_plan_host_call(const KasHostCallIn& in, KasHostCall* hc, std::string* err) {
  auto fail = [&](int code, const char* m) { if (err) *err = m; return code; };
  int rc;
  if (in.front) {                                               // a front's own refusals come first
    const char* bad = kas_front_spec_error_keys(in.front, in.batch->n_scenarios, in.rack_keys, in.topic_keys);
    if (bad[0]) return fail(KAS_E_INVALID_ARG, bad);
    if (in.rack_keys && !in.racks && kas_front_spec_uses_racks(in.front)) return fail(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
    if (in.topic_keys && !in.topics && kas_front_spec_uses_topics(in.front)) return fail(KAS_E_INVALID_ARG, KAS_NO_TOPIC_RECORDS);
    hc->ch_spec = kas_front_choose_spec(in.front);
  } else if (in.choose) {
    if (in.rack_keys || in.topic_keys) {                        // ... and so do those of a choice that may name rack or topic criteria
      const char* bad = kas_choose_spec_error_keys(in.choose, in.batch->n_scenarios, in.rack_keys, in.topic_keys);
      if (bad[0]) return fail(KAS_E_INVALID_ARG, bad);
      if (in.rack_keys && !in.racks && kas_choose_spec_uses_racks(in.choose)) return fail(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
      if (in.topic_keys && !in.topics && kas_choose_spec_uses_topics(in.choose)) return fail(KAS_E_INVALID_ARG, KAS_NO_TOPIC_RECORDS);
    }
    hc->ch_spec = *in.choose;
  }
  const kas_choose_spec* const choose = in.front ? &hc->ch_spec : in.choose;
  hc->all_rows = in.n_select < 0;
  if (!hc->all_rows && in.n_select > 0 && !in.select) return fail(KAS_E_INVALID_ARG, "select == NULL");
  hc->batch = *in.batch;
  if (in.cells16 && (rc = kas_ident_batch(in.batch, in.ident_ids, &hc->batch, in.ident_stamp, err)) != KAS_E_OK) return rc;
  const kas_batch_desc* b = &hc->batch;
  KasShape& full = hc->full;
  if ((rc = kas_shape_batch(b, &full, err, 0, 0)) != KAS_E_OK) return rc;
  const int64_t S = b->n_scenarios, T = b->n_topics;
  // A 16-bit call is solved on its 16-bit cells where the kernels with that I/O take the batch (what kas_plan_create16
  // accepts, asked HERE on the shape: a batch the 16-bit kernels refuse never reaches the plan cache with the 16-bit bit
  // set); any other batch is widened before and narrowed behind an int32 solve.
  hc->native16 = in.cells16 && kas_cells16_ok(full, in.lane_order_ok, in.built16[full.Wc]);
  hc->need32 = !hc->native16;
  if (in.cur_len < full.cur_need || (hc->all_rows && in.out_len < full.out_need) || in.aux_len < full.aux_need || in.ctx_len < full.ctx_need)
    return fail(KAS_E_INVALID_ARG, "a descriptor offset reaches beyond the pool length given in kas_tables");
  if ((full.cur_need > full.cur_lo && !in.have_cur) || (hc->all_rows && full.out_need > full.out_lo && !in.have_out) ||
      (full.aux_need > full.aux_lo && !in.have_aux) || (full.ctx_need > full.ctx_lo && !in.have_ctx) || (T && !in.have_topic_results) ||
      (S && !in.have_scenario_results))
    return fail(KAS_E_INVALID_ARG, "a table the descriptors refer to is NULL");
  hc->sel_off.clear();
  if (!hc->all_rows) {
    int64_t at = 0;
    hc->sel_off.resize((size_t)in.n_select + 1);
    for (int32_t k = 0; k < in.n_select; ++k) {
      if (in.select[k] < 0 || in.select[k] >= S) return fail(KAS_E_INVALID_ARG, "select: scenario index out of range");
      hc->sel_off[(size_t)k] = at;
      const kas_scenario_desc& sd = b->scenarios[in.select[k]];
      for (int32_t t = 0; t < sd.topic_count; ++t) {
        const kas_topic_desc& td = b->topics[sd.topic_begin + t];
        at += (int64_t)td.n_partitions * td.out_width;
      }
    }
    hc->sel_off[(size_t)in.n_select] = at;
    if (in.out_len < at || (at > 0 && !in.have_out))
      return fail(KAS_E_INVALID_ARG, "select: out / out_len too small for the selected scenarios' rows");
  }
  hc->imp_base.clear();
  if (in.impact) {
    hc->imp_base.assign((size_t)S + 1, 0);
    for (int64_t s = 0; s < S; ++s) hc->imp_base[(size_t)s + 1] = hc->imp_base[(size_t)s] + (b->scenarios[s].n_nodes > 0 ? b->scenarios[s].n_nodes : 0);
    if ((S > 0 && !in.have_imp_scenarios) || (hc->imp_base[(size_t)S] > 0 && !in.have_imp_nodes && !choose && !in.racks && !in.topics))
      return fail(KAS_E_INVALID_ARG, "kas_impact_tables: nodes / scenarios == NULL");
  }
  // the rack pass: the table (a negative entry, then too many racks), then the capacity, then the arrays
  auto rack_pass = [&]() -> int {
    if (!in.impact) return fail(KAS_E_INVALID_ARG, "kas_rack_tables: the rack pass needs the impact pass");
    if (in.report_rack && b->node_pool_len <= 0) return fail(KAS_E_INVALID_ARG, "report_rack: a table for a batch without nodes");
    if ((rc = kas_rack_plan_build(b, in.report_rack ? in.report_rack : b->node_rack, full.n_max, full.idmap_entries, full.need_bsearch,
                                  in.cells16 ? 1 : 0, -1, &hc->rack, err)) != KAS_E_OK)
      return rc;
    if (in.racks_cap < hc->rack.rack_off[(size_t)S]) return fail(KAS_E_INVALID_ARG, "kas_rack_tables: racks_cap below the sum of the scenarios' rack counts");
    if (!in.have_rk_off || (S > 0 && !in.have_rk_scenarios) || (hc->rack.rack_off[(size_t)S] > 0 && !in.have_rk_racks))
      return fail(KAS_E_INVALID_ARG, "kas_rack_tables: racks / scenarios / rack_off == NULL");
    return KAS_E_OK;
  };
  if (in.racks && !choose && (rc = rack_pass()) != KAS_E_OK) return rc;
  // the topic pass: the arrays, then the global counters of its work list
  auto topic_pass = [&]() -> int {
    if (!in.have_tp_tables || (T > 0 && !in.have_tp_topics) || (S > 0 && !in.have_tp_scenarios))
      return fail(KAS_E_INVALID_ARG, "kas_topic_impact_tables: topics / scenarios == NULL");
    KasTopicPlan tp;
    kas_topic_plan_build(b, full.n_max, full.idmap_entries, full.need_bsearch, in.cells16 ? 1 : 0, -1, kas_impact_rows_per_item(b), &tp);
    hc->tp_region_ints = tp.region_ints;
    if (!kas_topic_scratch_ok(tp)) return fail(KAS_E_UNSUPPORTED, KAS_TOPIC_SCRATCH_TEXT);
    return KAS_E_OK;
  };
  if (in.topics && !choose && (rc = topic_pass()) != KAS_E_OK) return rc;
  // a choice: the spec, then the room for any k scenarios (which ones win is not known before the solve), then the arrays
  if (choose) {
    const char* bad = kas_choose_spec_error_keys(choose, S, in.rack_keys, in.topic_keys);
    if (bad[0]) return fail(KAS_E_INVALID_ARG, bad);
    const int64_t k = choose->k;
    kas_choose_plan_build(b, &hc->choose);
    kas_choose_k_largest(hc->choose, (int32_t)k, &hc->ch_rows_need, &hc->ch_nodes_need);
    hc->ch_gather_rows = !(in.ch_rows_optional && in.rows_cap == 0 && !in.have_ch_rows);
    if (!hc->ch_gather_rows) hc->ch_rows_need = 0;
    if (in.rows_cap < hc->ch_rows_need) return fail(KAS_E_INVALID_ARG, "kas_choice: rows_cap below the packed rows of the k largest scenarios");
    if (in.nodes_cap < hc->ch_nodes_need) return fail(KAS_E_INVALID_ARG, "kas_choice: nodes_cap below the node records of the k largest scenarios");
    if ((S > 0 && !in.have_ch_rank) || (k > 0 && !in.have_ch_chosen) || !in.have_ch_row_off || !in.have_ch_node_off || !in.have_ch_n_ok ||
        (hc->ch_rows_need > 0 && !in.have_ch_rows) || (hc->ch_nodes_need > 0 && !in.have_ch_nodes) || (in.front && !in.have_fr_counts))
      return fail(KAS_E_INVALID_ARG, "kas_choice: an array the call writes is NULL");
    hc->ch_chunks = kas_choose_chunks(hc->choose, in.cells16 ? 2 : 4);
    if (k * hc->ch_chunks > INT32_MAX) return fail(KAS_E_UNSUPPORTED, "kas_choice: k scenarios of this size are more than one gather launch takes");
    hc->ch_head.lay_out(S, k);
  }
  // moves, in the order include/kas_abi.h documents: the mask, the capacities, the arrays, their alignment, the list, the shape
  if (in.moves) {
    const char* bad = kas_moves_args_error(in.moves, in.cells16 ? 2 : 4);
    if (bad[0]) return fail(KAS_E_INVALID_ARG, bad);
    hc->mv_list.clear();
    if (choose) {
      hc->mv_n = choose->k;
    } else if (in.mv_n_select < 0) {
      hc->mv_n = S;
      for (int64_t s = 0; s < S; ++s) hc->mv_list.push_back((int32_t)s);
    } else {
      if (in.mv_n_select > 0 && !in.mv_select) return fail(KAS_E_INVALID_ARG, "kas_moves: select == NULL");
      hc->mv_n = in.mv_n_select;
      for (int32_t j = 0; j < in.mv_n_select; ++j) {
        if (in.mv_select[j] < -1 || in.mv_select[j] >= S) return fail(KAS_E_INVALID_ARG, "kas_moves: select: scenario index out of range");
        hc->mv_list.push_back(in.mv_select[j]);
      }
    }
    kas_moves_plan_build(b, &hc->moves);
    bad = kas_moves_shape_error(hc->moves, hc->mv_n);
    if (bad[0]) return fail(KAS_E_UNSUPPORTED, bad);
    if (choose) kas_moves_k_largest(hc->moves, choose->k, &hc->mv_room_moves, &hc->mv_room_cells);
    else kas_moves_room(hc->moves, hc->mv_list.data(), hc->mv_n, &hc->mv_room_moves, &hc->mv_room_cells);
    hc->mv_moves_cap = in.moves->moves_cap < hc->mv_room_moves ? in.moves->moves_cap : hc->mv_room_moves;
    hc->mv_cells_cap = in.moves->cells_cap < hc->mv_room_cells ? in.moves->cells_cap : hc->mv_room_cells;
  }
  // batches, in the order include/kas_abi.h documents: the spec, the stride, the arrays, their alignment, the list, the node
  // limit, the room
  if (in.batches || in.bt_out) {
    if (in.bt_n_select > 0 && !in.bt_select) return fail(KAS_E_INVALID_ARG, "kas_batches: select == NULL");
    hc->bt_n = in.bt_n_select < 0 ? S : in.bt_n_select;
    int code = KAS_E_OK;
    const char* bad = kas_batches_list_error(b, in.bt_n_select < 0 ? nullptr : in.bt_select, hc->bt_n, in.batches, in.bt_out, &code, &hc->bt_n_cap);
    if (bad[0]) return fail(code, bad);
    hc->bt_list.clear();
    for (int64_t j = 0; j < hc->bt_n; ++j) hc->bt_list.push_back(in.bt_n_select < 0 ? (int32_t)j : in.bt_select[j]);
    kas_moves_plan_build(b, &hc->moves);
  }
  // rounds: the same order with the round spec, the two strides, KAS_ROUND_NODE_LIMIT and, behind it, the caps against the rows
  if (in.rounds || in.rd_out) {
    if (in.rd_n_select > 0 && !in.rd_select) return fail(KAS_E_INVALID_ARG, "kas_rounds: select == NULL");
    hc->rd_n = in.rd_n_select < 0 ? S : in.rd_n_select;
    int code = KAS_E_OK;
    kas_moves_plan_build(b, &hc->moves);
    const char* bad = kas_rounds_list_error(b, in.rd_n_select < 0 ? nullptr : in.rd_select, hc->rd_n, in.rounds, in.rd_out, &code, &hc->rd_n_cap, &hc->moves);
    if (bad[0]) return fail(code, bad);
    hc->rd_list.clear();
    for (int64_t j = 0; j < hc->rd_n; ++j) hc->rd_list.push_back(in.rd_n_select < 0 ? (int32_t)j : in.rd_select[j]);
  }
  if (in.racks && choose && (rc = rack_pass()) != KAS_E_OK) return rc;   // (behind a choice's refusals and its moves')
  if (in.topics && choose && (rc = topic_pass()) != KAS_E_OK) return rc; // (... and behind the rack pass's)
  // scenario ranges; batches whose ranges would share or interleave tables (what-if: every scenario reads one `cur`) stay whole
  const int64_t cell = in.cells16 ? 2 : 4;                     // bytes of a cur / out cell as it travels
  const int64_t cur_cells = full.cur_need - full.cur_lo, out_cells = full.out_need - full.out_lo;
  hc->K = kas_host_range_count(cell * (cur_cells + (hc->all_rows ? out_cells : 0)), S, in.ranges_override);
  const uint32_t own = (1u << KAS_POOL_TOPICS) | (1u << KAS_POOL_CUR) | (1u << KAS_POOL_OUT);
  if ((rc = kas_cut_ranges(b, hc->K, &full, &hc->ranges, err)) != KAS_E_OK) return rc;
  if (hc->K > 1 && !kas_ranges_disjoint(hc->ranges, own, true)) {
    hc->K = 1;
    if ((rc = kas_cut_ranges(b, 1, &full, &hc->ranges, err)) != KAS_E_OK) return rc;
  }
  // device pools: only [lo, need) of each is ever touched (+ 8 cells: the fill kernel's full-row loads re-read the last row for
  // lanes past the end); a 16-bit call solved on its own cells never touches the int32 pools
  size_t* by = hc->bytes;
  by[KAS_HB_CUR] = hc->need32 ? 4 * (size_t)(cur_cells + 8) : 0;
  by[KAS_HB_OUT] = hc->need32 ? 4 * (size_t)(out_cells + 8) : 0;
  by[KAS_HB_AUX] = 4 * (size_t)(full.aux_need - full.aux_lo + 8);
  by[KAS_HB_CTX] = 4 * (size_t)(full.ctx_need - full.ctx_lo + 8);
  by[KAS_HB_CUR16] = in.cells16 ? 2 * (size_t)(cur_cells + 8) : 0;
  by[KAS_HB_OUT16] = in.cells16 ? 2 * (size_t)(out_cells + 8) : 0;
  by[KAS_HB_TR] = by[KAS_HB_TR_PIN] = sizeof(kas_topic_result) * (size_t)(T + 1);
  by[KAS_HB_SR] = by[KAS_HB_SR_PIN] = sizeof(kas_scenario_result) * (size_t)(S + 1);
  by[KAS_HB_IMP_NODES] = in.impact ? sizeof(kas_node_impact) * (size_t)(hc->imp_base[(size_t)S] + 1) : 0;
  by[KAS_HB_IMP_SCEN] = in.impact ? sizeof(kas_scenario_impact) * (size_t)(S + 1) : 0;
  if (choose) {
    by[KAS_HB_CH_SIZES] = sizeof(KasChooseSize) * (hc->choose.sizes.size() + 1);
    by[KAS_HB_CH_SEGS] = sizeof(KasChooseSeg) * (hc->choose.segs.size() + 1);
    by[KAS_HB_CH_HEAD] = by[KAS_HB_CH_HEAD_PIN] = hc->ch_head.bytes;
    by[KAS_HB_CH_ROWS] = by[KAS_HB_CH_ROWS_PIN] = (size_t)cell * (size_t)(hc->ch_rows_need + 8);
    by[KAS_HB_CH_NODES] = by[KAS_HB_CH_NODES_PIN] = sizeof(kas_node_impact) * (size_t)(hc->ch_nodes_need + 1);
  }
  if (in.moves) {
    by[KAS_HB_MV_SCEN] = sizeof(KasMovesScen) * (hc->moves.scen.size() + 1);
    by[KAS_HB_MV_SEGS] = sizeof(KasMovesSeg) * (hc->moves.segs.size() + 1);
    by[KAS_HB_MV_SELECT] = choose ? 0 : 4 * (size_t)(hc->mv_n + 1);
    by[KAS_HB_MV_SCRATCH] = sizeof(KasMovesCount) * ((size_t)hc->mv_n * (size_t)hc->moves.max_items + 1);
    by[KAS_HB_MV_HEAD] = by[KAS_HB_MV_HEAD_PIN] = 16 * (size_t)(hc->mv_n + 1);
    by[KAS_HB_MV_MOVES] = sizeof(kas_move) * (size_t)(hc->mv_moves_cap + 1);
    by[KAS_HB_MV_CELLS] = (size_t)cell * (size_t)(hc->mv_cells_cap + 8);
    by[KAS_HB_MV_SIZES0] = choose && !hc->ch_gather_rows ? sizeof(KasChooseSize) * (hc->choose.sizes.size() + 1) : 0;
  }
  if (choose && !hc->ch_gather_rows) by[KAS_HB_MV_SIZES0] = sizeof(KasChooseSize) * (hc->choose.sizes.size() + 1);   // (with or without moves)
  if (in.racks) {
    by[KAS_HB_RK_RACKS] = sizeof(kas_rack_impact) * (size_t)(hc->rack.rack_off[(size_t)S] + 1);
    by[KAS_HB_RK_SCEN] = sizeof(kas_scenario_rack_impact) * (size_t)(S + 1);
  }
  if (in.topics) {
    by[KAS_HB_TP_TOPICS] = sizeof(kas_topic_impact) * (size_t)(T + 1);
    by[KAS_HB_TP_SCEN] = sizeof(kas_scenario_topic_impact) * (size_t)(S + 1);
  }
  if (in.batches) {
    by[KAS_HB_MV_SCEN] = sizeof(KasMovesScen) * (hc->moves.scen.size() + 1);
    by[KAS_HB_MV_SEGS] = sizeof(KasMovesSeg) * (hc->moves.segs.size() + 1);
    by[KAS_HB_BT_SDESC] = sizeof(kas_scenario_desc) * (size_t)(S + 1);
    by[KAS_HB_BT_NODE_ID] = hc->native16 ? 0 : 4 * (size_t)(b->node_pool_len + 1);
    by[KAS_HB_BT_SELECT] = 4 * (size_t)(hc->bt_n + 1);
    by[KAS_HB_BT_SCEN] = sizeof(kas_scenario_batches) * (size_t)(hc->bt_n + 1);
    by[KAS_HB_BT_BATCHES] = sizeof(kas_move_batch) * ((size_t)hc->bt_n * (size_t)in.bt_out->stride + 1);
  }
  if (in.rounds) {
    by[KAS_HB_MV_SCEN] = sizeof(KasMovesScen) * (hc->moves.scen.size() + 1);
    by[KAS_HB_MV_SEGS] = sizeof(KasMovesSeg) * (hc->moves.segs.size() + 1);
    by[KAS_HB_BT_SDESC] = sizeof(kas_scenario_desc) * (size_t)(S + 1);
    by[KAS_HB_BT_NODE_ID] = hc->native16 ? 0 : 4 * (size_t)(b->node_pool_len + 1);
    by[KAS_HB_BT_SELECT] = 4 * (size_t)(hc->rd_n + 1);
    by[KAS_HB_RD_SCEN] = sizeof(kas_scenario_rounds) * (size_t)(hc->rd_n + 1);
    by[KAS_HB_RD_ROUNDS] = sizeof(kas_move_round) * ((size_t)hc->rd_n * (size_t)in.rd_out->round_stride + 1);
    by[KAS_HB_RD_OF] = 4 * ((size_t)hc->rd_n * (size_t)in.rd_out->move_stride + 1);
  }
  if (in.front) {
    by[KAS_HB_FR_CLS] = 4 * (size_t)(S + 1);
    by[KAS_HB_FR_COUNTS] = by[KAS_HB_FR_COUNTS_PIN] = 4 * sizeof(int32_t);
  }
  return KAS_E_OK;
}

// ---- the plan cache's pure half -------------------------------------------------------------------------------------------
// word-at-a-time hash of the descriptor bytes (a what-if call hashes megabytes of node tables)
// (four independent lanes over 32-byte blocks: one dependent multiply chain ran at ~4 GB/s and made the 8 MB of
// descriptors and node tables of a 1000-variant what-if call cost 2 of its 5 ms)
static inline uint64_t kas_hash64(uint64_t h, const void* data, size_t n) {
  const unsigned char* p = (const unsigned char*)data;
  const uint64_t M = 0x9E3779B97F4A7C15ull;
  uint64_t a = h, b = h ^ 0x243F6A8885A308D3ull, c = h ^ 0x13198A2E03707344ull, d = h ^ 0xA4093822299F31D0ull;
  size_t i = 0;
  for (; i + 32 <= n; i += 32) {
    uint64_t w[4];
    memcpy(w, p + i, 32);
    a = (a ^ w[0]) * M; a ^= a >> 29;
    b = (b ^ w[1]) * M; b ^= b >> 29;
    c = (c ^ w[2]) * M; c ^= c >> 29;
    d = (d ^ w[3]) * M; d ^= d >> 29;
  }
  h = a;
  h = (h ^ b) * M; h ^= h >> 29;
  h = (h ^ c) * M; h ^= h >> 29;
  h = (h ^ d) * M; h ^= h >> 29;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, p + i, 8);
    h = (h ^ w) * M;
    h ^= h >> 29;
  }
  for (; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
  return h;
}

// What identifies a batch to the cache: (S, T, node pool length, cell width), scenario and topic descriptors, node tables — hashed
// and compared where they lie; a copy is made only when a plan is built for them.
struct KasBatchIdent {
  int64_t hdr[2];
  const void* seg[5];
  size_t seg_bytes[5], total = 0;
  uint64_t key = 0;             // every byte
  uint64_t sig = 0;             // (S, T) + topic descriptors + the cell width: what-if variants of one snapshot share it, and a plan
                                // for the other cell width is never the one rebuilt in place
  KasBatchIdent(const kas_batch_desc* b, int cells16) {
    const size_t nb = sizeof(int32_t) * (size_t)b->node_pool_len;
    hdr[0] = ((int64_t)b->n_scenarios << 32) | (uint32_t)b->n_topics;
    hdr[1] = b->node_pool_len | ((int64_t)(cells16 ? 1 : 0) << 62);   // (a plan for 16-bit cells is another plan)
    const void* s[5] = {hdr, b->scenarios, b->topics, b->node_id, b->node_rack};
    const size_t n[5] = {16, sizeof(kas_scenario_desc) * (size_t)b->n_scenarios, sizeof(kas_topic_desc) * (size_t)b->n_topics, nb, nb};
    key = 0xcbf29ce484222325ull;
    for (int i = 0; i < 5; ++i) {
      seg[i] = s[i]; seg_bytes[i] = n[i]; total += n[i];
      if (n[i]) key = kas_hash64(key, s[i], n[i]);
    }
    sig = kas_hash64(0x84222325cbf29ce4ull, hdr, 8) ^ kas_hash64(0, b->topics, n[2]) ^ (cells16 ? 0x5bd1e995c16c16c1ull : 0ull);
  }
  KasBatchIdent(const KasBatchIdent&) = delete;                 // (seg[0] points into the object)
  bool same_bytes(const std::vector<unsigned char>& have) const {
    if (have.size() != total) return false;
    size_t off = 0;
    for (int i = 0; i < 5; ++i) {
      if (seg_bytes[i] && memcmp(have.data() + off, seg[i], seg_bytes[i]) != 0) return false;
      off += seg_bytes[i];
    }
    return true;
  }
  void copy_to(std::vector<unsigned char>* to) const {
    to->resize(total);
    size_t off = 0;
    for (int i = 0; i < 5; ++i) { if (seg_bytes[i]) memcpy(to->data() + off, seg[i], seg_bytes[i]); off += seg_bytes[i]; }
  }
};
static inline bool kas_batch_ident_ok(const kas_batch_desc* b) {
  return !(b->n_scenarios < 0 || b->n_topics < 0 || b->node_pool_len < 0 || (b->n_scenarios > 0 && !b->scenarios) ||
           (b->n_topics > 0 && !b->topics) || (b->node_pool_len > 0 && (!b->node_id || !b->node_rack)));
}

// what the choice reads of a cache entry
struct KasCacheEntry {
  int32_t occupied = 0;
  uint64_t key = 0, sig = 0;
  uint64_t last_use = 0;
  uint64_t call = 0;            // host call that last used the entry (its ranges must not evict each other)
};
// Which entry serves a batch with this key and signature.  hits: the occupied entries whose key is the batch's (bit i: entry i) —
// the caller confirms one with the byte compare, lowest first, and a confirmed hit beats everything.  victim: where the plan is
// built on a miss — the least recently used entry of the same signature rebuilt in place (a what-if caller: same snapshot, other
// broker sets — every buffer is already large enough), else a free entry, else the least recently used entry of any shape; never an
// entry this call already uses (the other scenario ranges of a split call).  -1: every entry is this call's.
struct KasCacheChoice { uint32_t hits = 0; int32_t victim = -1; };
static inline KasCacheChoice kas_cache_choose(const KasCacheEntry* e, int32_t n, uint64_t key, uint64_t sig, uint64_t this_call) {
  KasCacheChoice c;
  int32_t same = -1, empty = -1, lru = -1;
  for (int32_t i = 0; i < n; ++i) {
    if (!e[i].occupied) { if (empty < 0) empty = i; continue; }
    if (e[i].key == key) c.hits |= 1u << i;
    if (e[i].call == this_call) continue;
    if (e[i].sig == sig && (same < 0 || e[i].last_use < e[same].last_use)) same = i;
    if (lru < 0 || e[i].last_use < e[lru].last_use) lru = i;
  }
  c.victim = same >= 0 ? same : (empty >= 0 ? empty : lru);
  return c;
}
