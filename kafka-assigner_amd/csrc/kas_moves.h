// kas_moves.h — the moves pass (include/kas_abi.h: kas_move / kas_moves): launch arguments, the host-built scenario and segment
// tables and the launcher the kernels' translation unit (kas_moves.hip) exports to kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same tables are built in the library and in the CPU emulation under tests/emu/.
//
// The pass runs after a solve, over the cur / out tables that solve used, for a list of n scenarios.  An *item* is a block of
// KAS_MOVES_ITEM_ROWS rows of one topic; a scenario's items are numbered topic by topic in descriptor order, so item order is
// (topic, row) order.  Three kernels, nothing between workgroups but the kernel boundaries:
//   count  grid n x (items of the largest scenario), one workgroup per (listed j, item i).  It reads select[j], leaves if the
//          entry is -1 or the scenario has no item i, counts the item's moves and their list cells (wave ballots) and stores the
//          pair at scratch[j * stride + i].
//   scan   ONE workgroup: an exclusive scan of the scratch table in (j, item) order, tile by tile with a carry (entries of
//          empty slots and of items a scenario does not have count as zero); it overwrites each pair with its prefix and
//          writes move_off / cell_off.
//   emit   the count kernel's grid again: it re-reads the rows; a move's position is the item's prefix + its rank within the
//          item in row order (ballots again: no atomics), its cells go behind the cell prefix the same way.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "kas_abi.h"

#define KAS_MOVES_BLOCK 256            // lanes of a workgroup of every kernel
#define KAS_MOVES_ROWS_PER_LANE 4      // rows a lane holds in registers
#define KAS_MOVES_ITEM_ROWS (KAS_MOVES_BLOCK * KAS_MOVES_ROWS_PER_LANE)   // 1024 rows: an item

// per scenario: its segments (one per topic, in descriptor order) and what it may need at most
struct KasMovesScen {
  int64_t rows;                 // sum of P: the most moves it can have
  int64_t cells;                // sum of P x out_width: the most list cells
  int32_t seg_begin, seg_count;
  int32_t items;                // sum over its topics of ceil(P / KAS_MOVES_ITEM_ROWS)
  int32_t reserved;
};

// one topic of one scenario: everything a workgroup needs of the descriptor (the plan's own descriptor tables are per
// scenario range in a host call; this table covers the whole call)
struct KasMovesSeg {
  int64_t cur_off, out_off;     // cells into the cur / out pools, as the device sees them
  int64_t cur_len_off;          // aux: int32 len[P], or -1
  int64_t part_id_off;          // aux: int32 partition ids[P], or -1
  int32_t topic;                // index of its kas_topic_result (the topic's index in the batch)
  int32_t rows;                 // P
  int32_t cur_width, out_width;
  int32_t item_begin;           // items of the scenario's earlier topics
  int32_t reserved;
};

// what the count kernel leaves per (j, item), and the scan turns into the pair's exclusive prefix over the whole list
struct KasMovesCount { int64_t moves, cells; };

// Kernel arguments of the three kernels: device pointers (host pointers in the emulator).
struct KasMovesLaunch {
  const KasMovesScen* scen;     // [S]
  const KasMovesSeg* segs;
  const int32_t* select;        // [n]
  const void* cur;              // int32 broker ids, or uint16 node indices (src16)
  const void* out;
  const int32_t* aux;
  const kas_topic_result* topic_results;
  KasMovesCount* scratch;       // [n * stride]
  int64_t* move_off;            // [n + 1]
  int64_t* cell_off;            // [n + 1]
  kas_move* moves;
  void* cells;                  // int32 cells, or uint16 (dst16)
  int64_t moves_cap, cells_cap;
  int32_t n, stride;            // listed scenarios; items of the largest scenario (at least 1)
  int32_t S;                    // scenarios of the tables: an entry of select outside 0..S-1 is an empty slot
  int32_t mask;
  int32_t src16, dst16;         // cur / out cells are uint16; the cells written are uint16 (an int32 solve of a 16-bit call: narrowed on the way)
};

struct KasMovesPlan {
  std::vector<KasMovesScen> scen;       // [S]
  std::vector<KasMovesSeg> segs;
  int32_t max_items = 1;                // the launch stride: items of the largest scenario, at least 1
  int64_t max_cells = 0;                // the largest scenario's packed cells
};

static inline void kas_moves_plan_build(const kas_batch_desc* b, KasMovesPlan* mp) {
  const int32_t S = b->n_scenarios > 0 ? b->n_scenarios : 0;
  mp->scen.assign((size_t)S, KasMovesScen{});
  mp->segs.clear();
  mp->max_items = 1; mp->max_cells = 0;
  for (int32_t s = 0; s < S; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    KasMovesScen& z = mp->scen[(size_t)s];
    z.seg_begin = (int32_t)mp->segs.size();
    int64_t items = 0;
    for (int32_t t = 0; t < sd.topic_count; ++t) {
      const kas_topic_desc& td = b->topics[sd.topic_begin + t];
      const int32_t P = td.n_partitions > 0 ? td.n_partitions : 0;
      const int32_t ow = td.out_width > 0 ? td.out_width : 0;
      KasMovesSeg g{};
      g.cur_off = td.cur_off; g.out_off = td.out_off; g.cur_len_off = td.cur_len_off; g.part_id_off = td.part_id_off;
      g.topic = sd.topic_begin + t; g.rows = P;
      g.cur_width = td.cur_width > 0 ? td.cur_width : 0; g.out_width = ow;
      g.item_begin = (int32_t)(items > INT32_MAX ? INT32_MAX : items);
      mp->segs.push_back(g);
      items += ((int64_t)P + KAS_MOVES_ITEM_ROWS - 1) / KAS_MOVES_ITEM_ROWS;
      z.rows += P;
      z.cells += (int64_t)P * ow;
    }
    z.seg_count = (int32_t)mp->segs.size() - z.seg_begin;
    z.items = (int32_t)(items > INT32_MAX ? INT32_MAX : items);
    if (z.items > mp->max_items) mp->max_items = z.items;
    if (z.cells > mp->max_cells) mp->max_cells = z.cells;
  }
}

// The room that is always enough for a list: the rows and the packed cells of the listed scenarios (entries outside 0..S-1,
// the -1 of an empty slot among them, take none).  select == NULL: every scenario once.
static inline void kas_moves_room(const KasMovesPlan& mp, const int32_t* select, int64_t n_select, int64_t* rows, int64_t* cells) {
  *rows = 0; *cells = 0;
  const int64_t S = (int64_t)mp.scen.size();
  const int64_t n = select ? n_select : S;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t s = select ? select[j] : j;
    if (s < 0 || s >= S) continue;
    *rows += mp.scen[(size_t)s].rows; *cells += mp.scen[(size_t)s].cells;
  }
}

// ... and for the k best of a choice, whichever scenarios win: the k largest of either
static inline void kas_moves_k_largest(const KasMovesPlan& mp, int32_t k, int64_t* rows, int64_t* cells) {
  std::vector<int64_t> r, c;
  for (const KasMovesScen& z : mp.scen) { r.push_back(z.rows); c.push_back(z.cells); }
  const size_t kk = (size_t)(k < 0 ? 0 : k) < r.size() ? (size_t)(k < 0 ? 0 : k) : r.size();
  std::partial_sort(r.begin(), r.begin() + (ptrdiff_t)kk, r.end(), std::greater<int64_t>());
  std::partial_sort(c.begin(), c.begin() + (ptrdiff_t)kk, c.end(), std::greater<int64_t>());
  *rows = 0; *cells = 0;
  for (size_t i = 0; i < kk; ++i) { *rows += r[i]; *cells += c[i]; }
}

// "" or why a kas_moves cannot be served (the text of the refusal), in the documented order: the mask, the capacities, the
// arrays, their alignment.  cell: bytes of a cell written.  *code: KAS_E_INVALID_ARG.
static inline const char* kas_moves_args_error(const kas_moves* mv, int32_t cell) {
  if (!mv) return "kas_moves == NULL";
  if (mv->mask < 1 || mv->mask > 7) return "kas_moves: mask outside 1..7";
  if (mv->moves_cap < 0 || mv->cells_cap < 0) return "kas_moves: negative capacity";
  if (!mv->move_off || !mv->cell_off || (mv->moves_cap > 0 && !mv->moves) || (mv->cells_cap > 0 && !mv->cells))
    return "kas_moves: an array the call writes is NULL";
  if ((uintptr_t)mv->moves % 4 != 0 || ((uintptr_t)mv->move_off | (uintptr_t)mv->cell_off) % 8 != 0 || (uintptr_t)mv->cells % (uintptr_t)cell != 0)
    return "kas_moves: records must be 4-byte aligned, the offset arrays 8-byte aligned, cells cell-aligned";
  return "";
}

// "" or why the plan's shape cannot be served (KAS_E_UNSUPPORTED): cell_at is an int32, and the grid one launch
static inline const char* kas_moves_shape_error(const KasMovesPlan& mp, int64_t n_select) {
  if (mp.max_cells >= ((int64_t)1 << 31)) return "kas_moves: a scenario's packed cells reach 2^31 (kas_move.cell_at is an int32)";
  if (n_select * (int64_t)mp.max_items > INT32_MAX) return "kas_moves: the list x the largest scenario's row blocks are more than one launch takes";
  return "";
}

// kas_moves.hip: the three kernels on `hip_stream`.  wc: the plan's width class (cells a row may hold).  Returns a hipError_t.
int kas_moves_launch(const KasMovesLaunch* a, int32_t wc, void* hip_stream);
