// kas_moves_body.h — device code of the moves pass (tables and launch arguments: kas_moves.h).
//
// Rows are loaded as the impact pass loads them: consecutive lanes on consecutive rows, a row's cells in registers (at most
// KAS_MAX_WIDTH, so set membership is a few compares), templated on the width class and on 16-bit source cells.  A lane holds
// KAS_MOVES_ROWS_PER_LANE rows: row u * KAS_MOVES_BLOCK + tid of the item for u = 0 .. 3, so row order within an item is
// (u, wavefront, lane) order, and a move's rank within its item is the moves of the earlier (u, wavefront) groups — sixteen
// pairs in the LDS — plus the set bits of its group's ballot below its lane.  List cells are placed the same way: a list is
// at most 8 cells long, so the cells of the lanes below are four ballots, one per bit of the length.  No atomics anywhere.
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/moves_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_moves.h"
#include "kas_wave.h"

namespace kasm {

constexpr int WAVES = KAS_MOVES_BLOCK / 64;
constexpr int U = KAS_MOVES_ROWS_PER_LANE;
constexpr int GROUPS = U * WAVES;          // (u, wavefront) groups of an item, in row order
constexpr int LEN_BITS = 4;                // a list length is 0 .. KAS_MAX_WIDTH = 8
static_assert(KAS_MAX_WIDTH < (1 << LEN_BITS), "a list length fits LEN_BITS ballots");

// one cell as an int32: a broker id (int32 cells) or a node index (16-bit cells, KAS_CELL16_NONE -> -1)
template <bool C16>
KAS_DEV int32_t cell(const void* pool, int64_t i) {
  if constexpr (C16) {
    const uint32_t v = reinterpret_cast<const uint16_t*>(pool)[i];
    return v == KAS_CELL16_NONE ? -1 : (int32_t)v;
  } else {
    return reinterpret_cast<const int32_t*>(pool)[i];
  }
}

// the item of workgroup (j, i): its topic's segment and its rows
struct Item {
  KasMovesSeg g;
  int32_t topic_rel;            // the topic's index within the scenario
  int32_t row_lo, row_hi;
  bool ok;                      // the topic's status is KAS_OK
};

// false: the list entry is an empty slot (-1, or no scenario of the tables) or the scenario has no item i.  The same for
// every lane of the workgroup.
KAS_DEV bool find_item(const KasMovesLaunch& a, int32_t j, int32_t i, Item& it) {
  const int32_t s = a.select[j];
  if (s < 0 || s >= a.S) return false;
  const KasMovesScen z = a.scen[s];
  if (i >= z.items) return false;
  int32_t lo = 0, hi = z.seg_count - 1;                         // the last segment with item_begin <= i (topics without rows
  while (lo < hi) {                                             // share the item_begin of the topic behind them)
    const int32_t mid = (lo + hi + 1) >> 1;
    if (a.segs[z.seg_begin + mid].item_begin <= i) lo = mid; else hi = mid - 1;
  }
  it.g = a.segs[z.seg_begin + lo];
  it.topic_rel = lo;
  it.row_lo = (i - it.g.item_begin) * KAS_MOVES_ITEM_ROWS;
  it.row_hi = it.g.rows - it.row_lo > KAS_MOVES_ITEM_ROWS ? it.row_lo + KAS_MOVES_ITEM_ROWS : it.g.rows;
  it.ok = a.topic_results[it.g.topic].status == KAS_OK;
  return true;
}

// A row's record word: flags | olen << 8 | gained << 16 | lost << 24 — bytes 8 .. 11 of its kas_move.
template <int W>
KAS_DEV uint32_t row_word(const int32_t (&c)[W], int32_t clen, const int32_t (&o)[W], int32_t olen) {
  int32_t gained = 0, lost = 0;
  bool same_lists = olen == clen;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    bool in_c = false, in_o = false;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      in_c = in_c || (j < clen && c[j] == o[k]);
      in_o = in_o || (j < olen && o[j] == c[k]);
    }
    gained += (k < olen && !in_c) ? 1 : 0;
    lost += (k < clen && !in_o) ? 1 : 0;
    same_lists = same_lists && (k >= olen || o[k] == c[k]);
  }
  if (olen == 0) return 0u;
  const bool same_sets = gained == 0 && lost == 0;
  uint32_t flags = same_sets ? 0u : (uint32_t)KAS_MOVE_REPLICAS;
  if (clen == 0 || o[0] != c[0]) flags |= KAS_MOVE_LEADER;
  if (same_sets && !same_lists) flags |= KAS_MOVE_ORDER;
  return flags | ((uint32_t)olen << 8) | ((uint32_t)gained << 16) | ((uint32_t)lost << 24);
}

// the item's rows of this lane: o[u] = the out cells of row row_lo + u * KAS_MOVES_BLOCK + tid, word[u] = its record word
// (0 for a row beyond the item: no flags, never a move)
template <int W, bool C16>
KAS_DEV void load_rows(const KasMovesLaunch& a, const Item& it, int32_t (&o)[U][W], uint32_t (&word)[U]) {
  const KasMovesSeg& g = it.g;
  const int32_t tid = kasw::tid();
  const int32_t cw = g.cur_width < W ? g.cur_width : W, ow = g.out_width < W ? g.out_width : W;
  const int32_t* lens = g.cur_len_off >= 0 ? a.aux + g.cur_len_off : nullptr;
  int32_t c[U][W], clen[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int32_t p = it.row_lo + u * KAS_MOVES_BLOCK + tid;
    const bool live = p < it.row_hi;
    const int32_t cl = live ? (lens ? lens[p] : cw) : 0;
    clen[u] = cl < 0 ? 0 : (cl > cw ? cw : cl);
    const int64_t crow = g.cur_off + (int64_t)p * g.cur_width, orow = g.out_off + (int64_t)p * g.out_width;
#pragma unroll
    for (int k = 0; k < W; ++k) c[u][k] = (live && k < cw) ? cell<C16>(a.cur, crow + k) : -1;
#pragma unroll
    for (int k = 0; k < W; ++k) o[u][k] = (live && k < ow) ? cell<C16>(a.out, orow + k) : -1;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int32_t olen = 0;
    bool open = true;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      open = open && k < ow && o[u][k] != -1;                   // (the pad: -1, KAS_CELL16_NONE)
      olen += open ? 1 : 0;
    }
    word[u] = row_word<W>(c[u], clen[u], o[u], olen);
  }
}

KAS_DEV bool is_move(uint32_t word, int32_t mask) { return (word & 0xffu & (uint32_t)mask) != 0u; }
KAS_DEV int32_t len_of(uint32_t word) { return (int32_t)((word >> 8) & 0xffu); }

// Count kernel body: workgroup `block` = (j, i).  red: 2 * WAVES int32 of LDS.
template <int W, bool C16>
KAS_DEV void count_item(const KasMovesLaunch& a, int32_t block, int32_t* red) {
  const int32_t j = block / a.stride, i = block % a.stride;
  Item it;
  if (!find_item(a, j, i, it)) return;                          // (the scan counts such an entry as zero)
  int32_t moves = 0, cells = 0;
  if (it.ok) {
    int32_t o[U][W];
    uint32_t word[U];
    load_rows<W, C16>(a, it, o, word);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool mv = is_move(word[u], a.mask);
      moves += kasw::popc(kasw::ballot(mv));
#pragma unroll
      for (int b = 0; b < LEN_BITS; ++b) cells += kasw::popc(kasw::ballot(mv && ((len_of(word[u]) >> b) & 1))) << b;
    }
  }
  if (kasw::lane() == 0) { red[2 * kasw::wave_id()] = moves; red[2 * kasw::wave_id() + 1] = cells; }
  kasw::sync();
  if (kasw::tid() == 0) {
    KasMovesCount c{0, 0};
    for (int w = 0; w < WAVES; ++w) { c.moves += red[2 * w]; c.cells += red[2 * w + 1]; }
    a.scratch[(int64_t)j * a.stride + i] = c;
  }
}

// inclusive prefix sum over the wavefront's lanes
KAS_DEV int32_t wave_scan(int32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t t = kasw::shfl(v, kasw::lane() - o);
    v += kasw::lane() >= o ? t : 0;
  }
  return v;
}

// Scan kernel body: the ONE workgroup.  red: 2 * WAVES int32 of LDS.
KAS_DEV void scan_all(const KasMovesLaunch& a, int32_t* red) {
  const int32_t tid = kasw::tid(), lane = kasw::lane(), wave = kasw::wave_id();
  const int64_t E = (int64_t)a.n * a.stride;
  int64_t carry_m = 0, carry_c = 0;
  for (int64_t base = 0; base < E; base += KAS_MOVES_BLOCK) {
    const int64_t e = base + tid;
    const bool in = e < E;
    const int32_t j = in ? (int32_t)((uint32_t)e / (uint32_t)a.stride) : 0;
    const int32_t i = in ? (int32_t)((uint32_t)e % (uint32_t)a.stride) : 0;
    bool valid = false;
    if (in) {
      const int32_t s = a.select[j];
      valid = s >= 0 && s < a.S && i < a.scen[s].items;
    }
    int32_t vm = 0, vc = 0;                                     // (an item has at most 1024 moves of 8 cells: a tile's sums fit)
    if (valid) { const KasMovesCount c = a.scratch[e]; vm = (int32_t)c.moves; vc = (int32_t)c.cells; }
    const int32_t im = wave_scan(vm), ic = wave_scan(vc);
    kasw::sync();                                               // (every lane has read the tile before's totals)
    if (lane == 63) { red[2 * wave] = im; red[2 * wave + 1] = ic; }
    kasw::sync();
    int64_t pm = carry_m, pc = carry_c;
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) { pm += red[2 * w]; pc += red[2 * w + 1]; }
      carry_m += red[2 * w]; carry_c += red[2 * w + 1];
    }
    pm += im - vm; pc += ic - vc;
    if (valid) a.scratch[e] = KasMovesCount{pm, pc};
    if (in && i == 0) { a.move_off[j] = pm; a.cell_off[j] = pc; }
  }
  if (tid == 0) { a.move_off[a.n] = carry_m; a.cell_off[a.n] = carry_c; }
}

// Emit kernel body: workgroup `block` = (j, i).  sub: 2 * GROUPS int32 of LDS.
template <int W, bool C16>
KAS_DEV void emit_item(const KasMovesLaunch& a, int32_t block, int32_t* sub) {
  const int32_t j = block / a.stride, i = block % a.stride;
  Item it;
  if (!find_item(a, j, i, it) || !it.ok) return;
  const int32_t tid = kasw::tid(), wave = kasw::wave_id();
  int32_t o[U][W];
  uint32_t word[U];
  load_rows<W, C16>(a, it, o, word);
  int32_t rank[U], below[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool mv = is_move(word[u], a.mask);
    const uint64_t m = kasw::ballot(mv);
    rank[u] = kasw::count_below(m);
    int32_t cb = 0, ct = 0;
#pragma unroll
    for (int b = 0; b < LEN_BITS; ++b) {
      const uint64_t mb = kasw::ballot(mv && ((len_of(word[u]) >> b) & 1));
      cb += kasw::count_below(mb) << b;
      ct += kasw::popc(mb) << b;
    }
    below[u] = cb;
    if (kasw::lane() == 0) { sub[2 * (u * WAVES + wave)] = kasw::popc(m); sub[2 * (u * WAVES + wave) + 1] = ct; }
  }
  kasw::sync();
  const KasMovesCount at = a.scratch[(int64_t)j * a.stride + i];
  const int64_t block_cells = a.cell_off[j];
  const int32_t* part = it.g.part_id_off >= 0 ? a.aux + it.g.part_id_off : nullptr;
  int32_t pm = 0, pc = 0;                                       // moves and cells of the groups before (u, wave)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    for (int w = 0; w < WAVES; ++w) {
      const int q = u * WAVES + w;
      if (w == wave) {
        const int32_t p = it.row_lo + u * KAS_MOVES_BLOCK + tid;
        const int32_t len = len_of(word[u]);
        const int64_t idx = at.moves + pm + rank[u], cpos = at.cells + pc + below[u];
        if (is_move(word[u], a.mask) && idx < a.moves_cap && cpos + len <= a.cells_cap) {
          kas_move r;
          r.topic = it.topic_rel;
          r.partition = part ? part[p] : p;
          r.flags = (uint8_t)word[u]; r.len = (uint8_t)(word[u] >> 8);
          r.gained = (uint8_t)(word[u] >> 16); r.lost = (uint8_t)(word[u] >> 24);
          r.cell_at = (int32_t)(cpos - block_cells);
          a.moves[idx] = r;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            if (k < len) {
              if (a.dst16) reinterpret_cast<uint16_t*>(a.cells)[cpos + k] = (uint16_t)o[u][k];
              else reinterpret_cast<int32_t*>(a.cells)[cpos + k] = o[u][k];
            }
          }
        }
      }
      pm += sub[2 * q]; pc += sub[2 * q + 1];
    }
  }
}

}  // namespace kasm
