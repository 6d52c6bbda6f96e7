// kas_rounds.h — the rounds pass (include/kas_abi.h: kas_round_spec / kas_move_round / kas_scenario_rounds / kas_rounds):
// launch arguments, the LDS layout, the refusals and the launcher the kernel's translation unit (kas_rounds.hip) exports to
// kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same layout and refusals are used in the library and in the CPU emulation under tests/emu/.
//
// The pass runs where the batches pass runs (kas_batches.h) and walks the same tiles: ONE workgroup per listed scenario loads
// each tile of KAS_MOVES_ITEM_ROWS rows into the batches pass's queue (kasb::load_tile, shared by inclusion), wavefront 0 gives
// the queue's moves their rounds one move a step against one word per node and direction, and all lanes add the moves to a
// window of round counters, all in the LDS.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kas_abi.h"
#include "kas_batches.h"

#define KAS_ROUND_BLOCK KAS_BATCH_BLOCK
#define KAS_ROUND_QUEUE KAS_MOVES_ITEM_ROWS      // entries: the queue is drained behind every tile
#define KAS_ROUND_WINDOW 1024                    // rounds whose counters the LDS holds at a time; a scenario of more rounds is walked again per window
#define KAS_ROUND_LDS_LIMIT KAS_BATCH_LDS_LIMIT
#define KAS_ROUND_MISC_BYTES KAS_BATCH_MISC_BYTES
#define KAS_ROUND_WINDOW_BYTES (12 * KAS_ROUND_WINDOW)   // per round: moves, replicas, first move

static_assert(KAS_ROUND_QUEUE <= KAS_BATCH_QUEUE, "a tile's moves fit the queue as the batches pass lays an entry out");

// per node: one 32-bit word for In and one for Out — (round << shift) | used — and 4 bytes of lookup
#define KAS_ROUND_NODE_BYTES 12
static_assert(KAS_ROUND_NODE_LIMIT == (KAS_ROUND_LDS_LIMIT - KAS_ROUND_QUEUE * kas_batch_entry_bytes(KAS_MAX_WIDTH) - KAS_ROUND_WINDOW_BYTES -
                                       KAS_ROUND_MISC_BYTES - 32) / KAS_ROUND_NODE_BYTES,
              "KAS_ROUND_NODE_LIMIT is what the widest kernel's layout leaves");
static_assert(KAS_ROUND_NODE_LIMIT < 0xFFFF, "node indices fit the queue's uint16 cells");

// How a node's word is split for a scenario of `rows` rows: a round is below the scenario's moves, so it fits the bits that hold
// `rows`; the moves a node holds in its round (at most the cap) get the rest.  A cap above `rows` can never bind and is applied
// as no bound; any other cap must fit its bits, or the scenario cannot be served (kas_rounds_caps_fit).
static inline constexpr int32_t kas_round_bits(int64_t rows) {   // (constexpr: the kernel calls it too)
  int32_t b = 1;
  while (b < 31 && ((int64_t)1 << b) <= rows) ++b;
  return b;
}
static inline bool kas_round_cap_fits(int32_t cap, int64_t rows) {
  return cap == 0 || cap > rows || (int64_t)cap < ((int64_t)1 << (32 - kas_round_bits(rows)));
}
// rows of scenario s in the moves pass's tables (what the kernel sums, whatever the topics' statuses)
static inline constexpr int64_t kas_round_rows(const KasMovesScen* scen, const KasMovesSeg* segs, int64_t s) {
  int64_t rows = 0;
  for (int32_t t = 0; t < scen[s].seg_count; ++t) rows += segs[scen[s].seg_begin + t].rows > 0 ? segs[scen[s].seg_begin + t].rows : 0;
  return rows;
}
static inline bool kas_rounds_caps_fit(const kas_round_spec* sp, const KasMovesScen* scen, const KasMovesSeg* segs, int64_t s) {
  const int64_t rows = kas_round_rows(scen, segs, s);
  return kas_round_cap_fits(sp->cap_inbound, rows) && kas_round_cap_fits(sp->cap_outbound, rows);
}

// LDS of the kernel, byte offsets: [in[n_cap] out[n_cap]: 4 bytes each] [lookup: 4 x n_cap] [misc] [queue nodes] [queue topic,
// partition] [window: moves[R] replicas[R] first[R]]
struct KasRoundsLds { int32_t off_look, off_misc, off_qn, off_qtp, off_win, total; };
static inline KasRoundsLds kas_rounds_lds(int32_t n_cap, int32_t W, int32_t cells16) {
  const int64_t n = n_cap > 0 ? n_cap : 0;
  auto a16 = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  KasRoundsLds L;
  int64_t o = a16(8 * n);
  L.off_look = (int32_t)o; o = a16(o + (cells16 ? 0 : 4 * n));
  L.off_misc = (int32_t)o; o += KAS_ROUND_MISC_BYTES;
  L.off_qn = (int32_t)o; o = a16(o + (int64_t)KAS_ROUND_QUEUE * 4 * W);
  L.off_qtp = (int32_t)o; o += (int64_t)KAS_ROUND_QUEUE * 8;
  L.off_win = (int32_t)o; o += KAS_ROUND_WINDOW_BYTES;
  L.total = (int32_t)o;
  return L;
}

// Kernel arguments: device pointers (host pointers in the emulator).
struct KasRoundsLaunch {
  const KasMovesScen* scen;     // [S] the moves pass's tables
  const KasMovesSeg* segs;
  const kas_scenario_desc* sdesc;   // [S] n_nodes and node_off are read
  const int32_t* node_id;       // int32 cells: the scenarios' ascending id tables
  const int32_t* select;        // [n]
  const void* cur;              // int32 broker ids, or uint16 node indices (src16)
  const void* out;
  const int32_t* aux;
  const kas_topic_result* topic_results;
  kas_scenario_rounds* scenarios;   // [n]
  kas_move_round* rounds;       // [n * round_stride]
  int32_t* round_of;            // [n * move_stride]
  int64_t round_stride, move_stride;
  kas_round_spec spec;
  int32_t n, S;                 // listed scenarios; scenarios of the tables: an entry of select outside 0..S-1 is an empty slot
  int32_t n_cap;                // no listed scenario has more nodes: what the LDS is laid out for
  int32_t src16;
  KasRoundsLds lds;
};

// "" or why the spec / the outputs cannot be served (KAS_E_INVALID_ARG), in the documented order
static inline const char* kas_rounds_args_error(const kas_round_spec* sp, const kas_rounds* o, int64_t n) {
  if (!sp || !o) return "kas_round_spec / kas_rounds == NULL";
  if (sp->cap_inbound < 0 || sp->cap_outbound < 0) return "kas_round_spec: a negative cap";
  if (sp->cap_inbound == 0 && sp->cap_outbound == 0) return "kas_round_spec: no cap at all";
  if (sp->policy != KAS_ROUNDS_MONOTONE) return "kas_round_spec: unknown policy";
  if (sp->reserved != 0) return "kas_round_spec: reserved != 0";
  if (o->round_stride < 0 || o->move_stride < 0) return "kas_rounds: negative stride";
  if ((n > 0 && !o->scenarios) || (o->round_stride > 0 && n > 0 && !o->rounds) || (o->move_stride > 0 && n > 0 && !o->round_of))
    return "kas_rounds: an array the call writes is NULL";
  if (((uintptr_t)o->scenarios | (uintptr_t)o->rounds | (uintptr_t)o->round_of) % 4 != 0) return "kas_rounds: records must be 4-byte aligned";
  return "";
}
#define KAS_ROUND_NODES_TEXT "kas_rounds: a scenario of more than KAS_ROUND_NODE_LIMIT nodes (its round words do not fit the LDS)"
#define KAS_ROUND_CAPS_TEXT "kas_rounds: a cap of 2^(32 - bits of the scenario's rows) or more that is not above its rows (the round words are 32 bits)"
#define KAS_ROUND_ROOM_TEXT "kas_rounds: n_select x round_stride x 16 bytes are more than 2^31"
#define KAS_ROUND_MOVE_ROOM_TEXT "kas_rounds: n_select x move_stride x 4 bytes are more than 2^31"
// "" or which of the two strides asks for more than 2^31 bytes
static inline const char* kas_rounds_room_error(int64_t n, const kas_rounds* o) {
  if (n <= 0) return "";
  if (o->round_stride > 0 && o->round_stride > (((int64_t)1 << 31) / 16) / n) return KAS_ROUND_ROOM_TEXT;
  if (o->move_stride > 0 && o->move_stride > (((int64_t)1 << 31) / 4) / n) return KAS_ROUND_MOVE_ROOM_TEXT;
  return "";
}

// The refusals of a list in host memory, in the documented order: "" or the text, with *code.  list == NULL: every scenario.
// *n_cap <- the most nodes of a listed scenario (what the LDS is laid out for).
// mp: the moves pass's tables of `b` (kas_moves_plan_build): the caps are held against the listed scenarios' rows.
static inline const char* kas_rounds_list_error(const kas_batch_desc* b, const int32_t* list, int64_t n, const kas_round_spec* sp,
                                                const kas_rounds* o, int* code, int32_t* n_cap, const KasMovesPlan* mp) {
  *code = KAS_E_INVALID_ARG; *n_cap = 0;
  const char* bad = kas_rounds_args_error(sp, o, n);
  if (bad[0]) return bad;
  const int64_t S = b->n_scenarios > 0 ? b->n_scenarios : 0;
  for (int64_t j = 0; list && j < n; ++j)
    if (list[j] < -1 || list[j] >= S) return "kas_rounds: select: scenario index out of range";
  *code = KAS_E_UNSUPPORTED;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t s = list ? list[j] : j;
    if (s < 0) continue;
    const int32_t N = b->scenarios[s].n_nodes;
    if (N > KAS_ROUND_NODE_LIMIT) return KAS_ROUND_NODES_TEXT;
    if (N > *n_cap) *n_cap = N;
  }
  for (int64_t j = 0; j < n; ++j) {
    const int64_t s = list ? list[j] : j;
    if (s >= 0 && !kas_rounds_caps_fit(sp, mp->scen.data(), mp->segs.data(), s)) return KAS_ROUND_CAPS_TEXT;
  }
  bad = kas_rounds_room_error(n, o);
  if (bad[0]) return bad;
  *code = KAS_E_OK;
  return "";
}

// kas_rounds.hip: the kernel on `hip_stream`, a->n workgroups.  wc: the plan's width class.  Returns a hipError_t.
int kas_rounds_launch(const KasRoundsLaunch* a, int32_t wc, void* hip_stream);
