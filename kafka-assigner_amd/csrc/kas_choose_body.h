// kas_choose_body.h — device code of the rank and gather kernels (launch arguments and tables: kas_choose.h).
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/choose_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_choose.h"
#include "kas_wave.h"

namespace kasc {

// ---- rank ---------------------------------------------------------------------------------------------------------------
// A scenario's key as two words compared most significant first: the criteria in spec order, two to a word, each biased so
// that unsigned order is int32 order; unused criteria are 0.  The scenario index, which breaks every tie, is not stored: an
// entry's index is its place in the tile.
struct Entry {
  uint64_t hi, lo;
  int64_t cells;                // 0 for a scenario that is not OK: it adds nothing to anybody's offsets
  int32_t nodes;
  int32_t ok;
};
static_assert(sizeof(Entry) == 32, "an LDS tile entry is two 16-byte reads");

KAS_DEV int32_t criterion(const kas_scenario_result& r, const kas_scenario_impact& m, int32_t key) {
  switch (key) {
    case KAS_KEY_MOVED_REPLICAS: return r.moved_replicas;
    case KAS_KEY_MOVED_PARTITIONS: return r.moved_partitions;
    case KAS_KEY_LEADERS_MOVED: return m.leaders_moved;
    case KAS_KEY_DEPARTED_REPLICAS: return m.departed_replicas;
    case KAS_KEY_MAX_INBOUND: return m.max_inbound;
    case KAS_KEY_MAX_OUTBOUND: return m.max_outbound;
    case KAS_KEY_REPLICA_SPREAD: return m.max_replicas_after - m.min_replicas_after;
    case KAS_KEY_LEADER_SPREAD: return m.max_leaders_after - m.min_leaders_after;
    case KAS_KEY_MAX_REPLICAS_AFTER: return m.max_replicas_after;
    default: return m.max_leaders_after;
  }
}

// Where a scenario's criteria come from, chosen at compile time.  Records: the scenario record and the impact record alone (the
// instances that were always there).  RackRecords: also the scenario rack records — a rack criterion is int32 word key -
// KAS_KEY_RACK_BASE of the 64-byte record, loaded alone (two words for a spread); the key is uniform, so is the branch.
struct Records {};
struct RackRecords { const kas_scenario_rack_impact* srk; };
static_assert(sizeof(kas_scenario_rack_impact) == 64 && KAS_KEY_RACK_END - KAS_KEY_RACK_BASE == 17, "fifteen words and two spreads");
KAS_DEV int32_t criterion_of(const Records&, const kas_scenario_result& r, const kas_scenario_impact& m, int32_t, int32_t key) {
  return criterion(r, m, key);
}
KAS_DEV int32_t criterion_of(const RackRecords& x, const kas_scenario_result& r, const kas_scenario_impact& m, int32_t s, int32_t key) {
  if (key < KAS_KEY_RACK_BASE) return criterion(r, m, key);
  const int32_t* w = reinterpret_cast<const int32_t*>(x.srk + s);
  if (key == KAS_KEY_RACK_REPLICA_SPREAD) return w[KAS_KEY_MAX_RACK_REPLICAS_AFTER - KAS_KEY_RACK_BASE] - w[KAS_KEY_MIN_RACK_REPLICAS_AFTER - KAS_KEY_RACK_BASE];
  if (key == KAS_KEY_RACK_LEADER_SPREAD) return w[KAS_KEY_MAX_RACK_LEADERS_AFTER - KAS_KEY_RACK_BASE] - w[KAS_KEY_MIN_RACK_LEADERS_AFTER - KAS_KEY_RACK_BASE];
  return w[key - KAS_KEY_RACK_BASE];
}

// TopicRecords: also the scenario topic records.  A topic criterion is int32 word key - KAS_KEY_TOPIC_BASE of the 64-byte record,
// one 4-byte load (the record holds the spreads: no derived keys); a rack criterion is loaded as RackRecords loads it, and srk may
// be NULL when the spec names none.
struct TopicRecords { const kas_scenario_rack_impact* srk; const kas_scenario_topic_impact* stp; };
static_assert(sizeof(kas_scenario_topic_impact) == 64 && KAS_KEY_TOPIC_END - KAS_KEY_TOPIC_BASE == 15, "fifteen words, the sixteenth reserved");
KAS_DEV int32_t criterion_of(const TopicRecords& x, const kas_scenario_result& r, const kas_scenario_impact& m, int32_t s, int32_t key) {
  if (key < KAS_KEY_RACK_BASE) return criterion(r, m, key);
  if (key < KAS_KEY_TOPIC_BASE) return criterion_of(RackRecords{x.srk}, r, m, s, key);
  return reinterpret_cast<const int32_t*>(x.stp + s)[key - KAS_KEY_TOPIC_BASE];
}

// Who takes part in a ranking, and what the ranking leaves for those who do not.  ByStatus: the scenarios that solved
// (kas_choose_spec); kas_front_body.h has the other one, the members of a front.
struct ByStatus {};
KAS_DEV int32_t takes_part(const ByStatus&, const KasChooseLaunch&, int32_t, const kas_scenario_result& r) { return r.status == KAS_OK ? 1 : 0; }
KAS_DEV int32_t outside(const ByStatus&, const KasChooseLaunch&, int32_t) { return -1; }
KAS_DEV void count(const ByStatus&, const KasChooseLaunch& a, int32_t n) { a.n_ok[0] = n; }

template <class Part, class Src>
KAS_DEV Entry entry_of(const KasChooseLaunch& a, int32_t s, const Part& part, const Src& src) {
  const kas_scenario_result r = a.sr[s];
  const kas_scenario_impact m = a.si[s];
  Entry e;
  e.ok = takes_part(part, a, s, r);
  uint32_t c[KAS_CHOOSE_MAX_KEYS];
#pragma unroll
  for (int i = 0; i < KAS_CHOOSE_MAX_KEYS; ++i)
    c[i] = i < a.n_keys ? (uint32_t)criterion_of(src, r, m, s, a.key[i]) ^ 0x80000000u : 0u;
  e.hi = ((uint64_t)c[0] << 32) | c[1];
  e.lo = ((uint64_t)c[2] << 32) | c[3];
  e.cells = e.ok && a.sizes ? a.sizes[s].cells : 0;
  e.nodes = e.ok && a.sizes ? a.sizes[s].n_nodes : 0;
  return e;
}

// Workgroup `block` of the rank kernel.  tile: KAS_CHOOSE_TILE entries of LDS.  The grid covers S + 1 lanes: lane g < S is
// scenario g, and lane g <= k is also slot g of chosen / row_off / node_off, which it writes when no scenario has that rank.
template <class Part = ByStatus, class Src = Records>
KAS_DEV void rank_block(const KasChooseLaunch& a, int32_t block, Entry* tile, const Part& part = Part(), const Src& src = Src()) {
  const int32_t tid = kasw::tid();
  const int32_t g = block * KAS_CHOOSE_BLOCK + tid;
  const bool live = g < a.S;
  Entry mine;
  mine.hi = 0; mine.lo = 0; mine.cells = 0; mine.nodes = 0; mine.ok = 0;
  if (live) mine = entry_of(a, g, part, src);
  int32_t smaller = 0, n_ok = 0;
  int64_t cells = 0, nodes = 0, all_cells = 0, all_nodes = 0;
  for (int32_t base = 0; base < a.S; base += KAS_CHOOSE_TILE) {
    const int32_t n = a.S - base < KAS_CHOOSE_TILE ? a.S - base : KAS_CHOOSE_TILE;
    kasw::sync();                                               // (every lane has left the tile before)
    for (int32_t i = tid; i < n; i += KAS_CHOOSE_BLOCK) tile[i] = entry_of(a, base + i, part, src);
    kasw::sync();
    for (int32_t i = 0; i < n; ++i) {                           // (every lane reads the same entry: an LDS broadcast)
      const Entry e = tile[i];
      const bool before = e.hi < mine.hi || (e.hi == mine.hi && (e.lo < mine.lo || (e.lo == mine.lo && base + i < g)));
      const bool lt = e.ok != 0 && before;
      smaller += lt ? 1 : 0;
      cells += lt ? e.cells : 0;
      nodes += lt ? (int64_t)e.nodes : 0;
      n_ok += e.ok;
      all_cells += e.cells;
      all_nodes += e.nodes;
    }
  }
  if (live) {
    a.rank[g] = mine.ok ? smaller : outside(part, a, g);
    if (mine.ok && smaller <= a.k) {
      if (smaller < a.k) a.chosen[smaller] = g;
      if (a.sizes) { a.row_off[smaller] = cells; a.node_off[smaller] = nodes; }
    }
  }
  if (g >= n_ok && g <= a.k) {                                  // a slot behind the last scenario that takes part
    if (g < a.k) a.chosen[g] = -1;
    if (a.sizes) { a.row_off[g] = all_cells; a.node_off[g] = all_nodes; }
  }
  if (g == 0) count(part, a, n_ok);
}

// ---- gather -------------------------------------------------------------------------------------------------------------
struct alignas(16) V16 { uint32_t x, y, z, w; };
struct alignas(8) V8 { uint32_t x, y; };

template <class T>
KAS_DEV void copy_as(unsigned char* dst, const unsigned char* src, int64_t n) {
  T* d = reinterpret_cast<T*>(dst);
  const T* s = reinterpret_cast<const T*>(src);
  for (int64_t i = kasw::tid(); i < n; i += KAS_CHOOSE_BLOCK) d[i] = s[i];
}

// n bytes from src to dst by the whole workgroup; both addresses and n are multiples of 2 (the entries refuse pools that are not
// cell-aligned).  The widest access is the one at which the two addresses are congruent (a packed destination behind an
// odd-sized scenario is off by one cell), never narrower than 2 bytes; the bytes before the first and behind the last aligned
// unit go two at a time.
KAS_DEV void copy_bytes(unsigned char* dst, const unsigned char* src, int64_t n) {
  const uint32_t diff = ((uint32_t)(uintptr_t)dst ^ (uint32_t)(uintptr_t)src) & 14u;
  const int64_t A = diff == 0u ? 16 : (int64_t)(diff & (0u - diff));   // 16, 8, 4 or 2
  int64_t head = (A - (int64_t)((uintptr_t)dst & (uintptr_t)(A - 1))) & (A - 1);
  if (head > n) head = n;
  const int64_t units = (n - head) / A, tail_at = head + units * A;
  copy_as<uint16_t>(dst, src, head >> 1);
  if (A == 16) copy_as<V16>(dst + head, src + head, units);
  else if (A == 8) copy_as<V8>(dst + head, src + head, units);
  else if (A == 4) copy_as<uint32_t>(dst + head, src + head, units);
  else copy_as<uint16_t>(dst + head, src + head, units);
  copy_as<uint16_t>(dst + tail_at, src + tail_at, (n - tail_at) >> 1);
}

// int32 cells to 16-bit cells (a node index is below 32,768 and the pad is -1: the low half of the cell is the 16-bit cell)
KAS_DEV void copy_narrow(uint16_t* dst, const int32_t* src, int64_t cells) {
  for (int64_t i = kasw::tid(); i < cells; i += KAS_CHOOSE_BLOCK) dst[i] = (uint16_t)src[i];
}

// Workgroup `item` of the gather kernel: chunk item % chunks of chosen scenario item / chunks.
KAS_DEV void gather_item(const KasChooseLaunch& a, int64_t item) {
  const int32_t j = (int32_t)(item / a.chunks);
  const int64_t c = item % a.chunks;
  const int32_t s = a.chosen[j];
  if (s < 0) return;                                            // (behind min(k, n_ok))
  const KasChooseSize z = a.sizes[s];
  const int64_t row_bytes = z.cells * a.dst_cell;
  const int64_t row_chunks = kas_choose_chunks_of(row_bytes);
  if (c < row_chunks) {
    const int64_t lo = c * KAS_CHOOSE_CHUNK, hi = lo + KAS_CHOOSE_CHUNK < row_bytes ? lo + KAS_CHOOSE_CHUNK : row_bytes;
    unsigned char* dst = reinterpret_cast<unsigned char*>(a.rows) + a.row_off[j] * a.dst_cell;
    for (int32_t t = 0; t < z.seg_count; ++t) {
      const KasChooseSeg g = a.segs[z.seg_begin + t];
      const int64_t g_lo = g.packed_at * a.dst_cell, g_hi = g_lo + g.cells * a.dst_cell;
      const int64_t x_lo = lo > g_lo ? lo : g_lo, x_hi = hi < g_hi ? hi : g_hi;
      if (x_lo >= x_hi) continue;
      const int64_t first = (x_lo - g_lo) / a.dst_cell;         // cell of the topic
      const unsigned char* src = reinterpret_cast<const unsigned char*>(a.out) + (g.out_off + first) * a.src_cell;
      if (a.src_cell == a.dst_cell) copy_bytes(dst + x_lo, src, x_hi - x_lo);
      else copy_narrow(reinterpret_cast<uint16_t*>(dst + x_lo), reinterpret_cast<const int32_t*>(src), (x_hi - x_lo) / a.dst_cell);
    }
    return;
  }
  const int64_t node_bytes = (int64_t)z.n_nodes * (int64_t)sizeof(kas_node_impact);
  const int64_t lo = (c - row_chunks) * KAS_CHOOSE_CHUNK;
  if (lo >= node_bytes) return;
  const int64_t hi = lo + KAS_CHOOSE_CHUNK < node_bytes ? lo + KAS_CHOOSE_CHUNK : node_bytes;
  copy_bytes(reinterpret_cast<unsigned char*>(a.nodes + a.node_off[j]) + lo,
             reinterpret_cast<const unsigned char*>(a.src_nodes + z.node_base) + lo, hi - lo);
}

}  // namespace kasc
