// kas_batches.h — the batches pass (include/kas_abi.h: kas_batch_spec / kas_move_batch / kas_scenario_batches / kas_batches):
// launch arguments, the LDS layout, the refusals and the launcher the kernel's translation unit (kas_batches.hip) exports to
// kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same layout and refusals are used in the library and in the CPU emulation under tests/emu/.
//
// The pass runs after a solve, over the cur / out tables that solve used, for a list of n scenarios: ONE workgroup per listed
// scenario walks the scenario's rows in (topic, row) order — the segment and scenario tables are those of the moves pass
// (kas_moves.h), an item of KAS_MOVES_ITEM_ROWS rows a tile — compacts each tile's REPLICAS moves into a queue in the LDS and
// consumes the queue in groups of KAS_BATCH_GROUP moves against two counters per node, also in the LDS.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kas_abi.h"
#include "kas_moves.h"

#define KAS_BATCH_BLOCK KAS_MOVES_BLOCK          // lanes of the workgroup: the tile is loaded as the moves pass loads an item
#define KAS_BATCH_GROUP 256                      // moves tried at once: one per lane
#define KAS_BATCH_QUEUE (KAS_MOVES_ITEM_ROWS + KAS_BATCH_GROUP)   // entries: a tile's moves behind what the tile before left (< a group)
#define KAS_BATCH_LDS_LIMIT (160 * 1024)
#define KAS_BATCH_MISC_BYTES 256                 // flags, the published batch size, the tile's (u, wavefront) counts, reduction words
#define KAS_BATCH_NODE_NONE 0xFFFFu              // a queue cell that names no node

static_assert(KAS_BATCH_GROUP == KAS_BATCH_BLOCK, "one move of a group per lane");

// bytes of one queue entry: In and Out node indices as uint16 (W each), then topic and partition
static inline constexpr int64_t kas_batch_entry_bytes(int32_t W) { return 2 * 2 * (int64_t)W + 8; }
// per node: two int32 counters and 4 bytes of lookup (a sorted id, or two entries of the direct int16 table)
#define KAS_BATCH_NODE_BYTES 12
static_assert(KAS_BATCH_NODE_LIMIT == (KAS_BATCH_LDS_LIMIT - KAS_BATCH_QUEUE * kas_batch_entry_bytes(KAS_MAX_WIDTH) - KAS_BATCH_MISC_BYTES - 32) /
                                          KAS_BATCH_NODE_BYTES,
              "KAS_BATCH_NODE_LIMIT is what the widest kernel's layout leaves");

// LDS of the kernel, byte offsets: [in[n_cap] out[n_cap]] [lookup: 4 x n_cap] [misc] [queue nodes] [queue topic, partition]
struct KasBatchesLds { int32_t off_look, off_misc, off_qn, off_qtp, total; };
static inline KasBatchesLds kas_batches_lds(int32_t n_cap, int32_t W, int32_t cells16) {
  const int64_t n = n_cap > 0 ? n_cap : 0;
  auto a16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  KasBatchesLds L;
  int64_t o = a16(8 * n);
  L.off_look = (int32_t)o; o = a16(o + (cells16 ? 0 : 4 * n));
  L.off_misc = (int32_t)o; o += KAS_BATCH_MISC_BYTES;
  L.off_qn = (int32_t)o; o = a16(o + (int64_t)KAS_BATCH_QUEUE * 4 * W);
  L.off_qtp = (int32_t)o; o += (int64_t)KAS_BATCH_QUEUE * 8;
  L.total = (int32_t)o;
  return L;
}

// Kernel arguments: device pointers (host pointers in the emulator).
struct KasBatchesLaunch {
  const KasMovesScen* scen;     // [S] the moves pass's tables
  const KasMovesSeg* segs;
  const kas_scenario_desc* sdesc;   // [S] n_nodes and node_off are read
  const int32_t* node_id;       // int32 cells: the scenarios' ascending id tables
  const int32_t* select;        // [n]
  const void* cur;              // int32 broker ids, or uint16 node indices (src16)
  const void* out;
  const int32_t* aux;
  const kas_topic_result* topic_results;
  kas_scenario_batches* scenarios;   // [n]
  kas_move_batch* batches;      // [n * stride]
  int64_t stride;
  kas_batch_spec spec;
  int32_t n, S;                 // listed scenarios; scenarios of the tables: an entry of select outside 0..S-1 is an empty slot
  int32_t n_cap;                // no listed scenario has more nodes: what the LDS is laid out for
  int32_t src16;
  KasBatchesLds lds;
};

// "" or why the spec / the outputs cannot be served (KAS_E_INVALID_ARG), in the documented order
static inline const char* kas_batches_args_error(const kas_batch_spec* sp, const kas_batches* o, int64_t n) {
  if (!sp || !o) return "kas_batch_spec / kas_batches == NULL";
  if (sp->cap_inbound < 0 || sp->cap_outbound < 0 || sp->max_moves < 0) return "kas_batch_spec: a negative bound";
  if (sp->cap_inbound == 0 && sp->cap_outbound == 0 && sp->max_moves == 0) return "kas_batch_spec: no bound at all";
  if (sp->reserved != 0) return "kas_batch_spec: reserved != 0";
  if (o->stride < 0) return "kas_batches: negative stride";
  if ((n > 0 && !o->scenarios) || (o->stride > 0 && n > 0 && !o->batches)) return "kas_batches: an array the call writes is NULL";
  if (((uintptr_t)o->scenarios | (uintptr_t)o->batches) % 4 != 0) return "kas_batches: records must be 4-byte aligned";
  return "";
}
#define KAS_BATCH_NODES_TEXT "kas_batches: a scenario of more than KAS_BATCH_NODE_LIMIT nodes (its counters do not fit the LDS)"
#define KAS_BATCH_ROOM_TEXT "kas_batches: n_select x stride x 32 bytes are more than 2^31"
static inline bool kas_batches_room_ok(int64_t n, int64_t stride) {
  return n <= 0 || stride <= 0 || stride <= (((int64_t)1 << 31) / 32) / n;
}

// The refusals of a list in host memory, in the documented order: "" or the text, with *code.  list == NULL: every scenario.
// *n_cap <- the most nodes of a listed scenario (what the LDS is laid out for).
static inline const char* kas_batches_list_error(const kas_batch_desc* b, const int32_t* list, int64_t n, const kas_batch_spec* sp,
                                                 const kas_batches* o, int* code, int32_t* n_cap) {
  *code = KAS_E_INVALID_ARG; *n_cap = 0;
  const char* bad = kas_batches_args_error(sp, o, n);
  if (bad[0]) return bad;
  const int64_t S = b->n_scenarios > 0 ? b->n_scenarios : 0;
  for (int64_t j = 0; list && j < n; ++j)
    if (list[j] < -1 || list[j] >= S) return "kas_batches: select: scenario index out of range";
  *code = KAS_E_UNSUPPORTED;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t s = list ? list[j] : j;
    if (s < 0) continue;
    const int32_t N = b->scenarios[s].n_nodes;
    if (N > KAS_BATCH_NODE_LIMIT) return KAS_BATCH_NODES_TEXT;
    if (N > *n_cap) *n_cap = N;
  }
  if (!kas_batches_room_ok(n, o->stride)) return KAS_BATCH_ROOM_TEXT;
  *code = KAS_E_OK;
  return "";
}

// kas_batches.hip: the kernel on `hip_stream`, a->n workgroups.  wc: the plan's width class.  Returns a hipError_t.
int kas_batches_launch(const KasBatchesLaunch* a, int32_t wc, void* hip_stream);
