// kas_impact_body.h — device code of the impact pass (work list and launch arguments: kas_impact.h).
//
// Item kernel: one workgroup of KAS_IMPACT_BLOCK lanes per (scenario, topic, row range).  It reads the topic's status once,
// stages the scenario's id -> node lookup in the LDS (int32 cells: the direct table where the plan has one, else the sorted
// ids for a binary search; 16-bit cells are node indices already), zeroes a histogram of N x 6 int32, and streams the rows:
// consecutive lanes on consecutive rows, a row's cells in registers (at most KAS_MAX_WIDTH, so set membership is a few
// compares), every count a no-return LDS add.  Merge kernel: one workgroup per scenario whose counters sit in global scratch.
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/impact_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_impact.h"
#include "kas_wave.h"

namespace kasi {

constexpr int F = KAS_IMPACT_FIELDS;
constexpr int WAVES = KAS_IMPACT_BLOCK / 64;
constexpr int ROWS_PER_LANE = 2;   // rows a lane loads before it counts them

// one cell as an int32: a broker id (int32 cells) or a node index (16-bit cells, KAS_CELL16_NONE -> -1)
template <bool C16>
KAS_DEV int32_t cell(const int32_t* pool, int64_t i) {
  if constexpr (C16) {
    const uint32_t v = reinterpret_cast<const uint16_t*>(pool)[i];
    return v == KAS_CELL16_NONE ? -1 : (int32_t)v;
  } else {
    return pool[i];
  }
}

// cell value -> node index of the scenario, -1 for none
struct Lookup {
  const int16_t* map;     // direct table: id - min_id -> node index or -1
  const int32_t* ids;     // else the sorted ids
  int32_t min_id;
  uint32_t range;         // > 0: the direct table
  int32_t n;
};

template <bool C16>
KAS_DEV int32_t node_of(const Lookup& L, int32_t v) {
  if constexpr (C16) {
    return (uint32_t)v < (uint32_t)L.n ? v : -1;
  } else {
    if (L.range != 0u) {
      const uint32_t d = (uint32_t)v - (uint32_t)L.min_id;
      return d < L.range ? (int32_t)L.map[d] : -1;
    }
    int32_t lo = 0, hi = L.n;                        // first id >= v
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (L.ids[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo < L.n && L.ids[lo] == v ? lo : -1;
  }
}

template <bool GLOBAL>
KAS_DEV void bump(int32_t* h, int32_t i, int32_t v) {
  if constexpr (GLOBAL) kasw::global_atomic_add(h + i, v);
  else kasw::lds_add_u32(reinterpret_cast<uint32_t*>(h + i), (uint32_t)v);
}

// one row: C = c[0, clen), O = o[0, olen)
template <int W, bool C16, bool GLOBAL>
KAS_DEV void count_row(const Lookup& L, const int32_t (&c)[W], int32_t clen, const int32_t (&o)[W], int32_t olen, int32_t* h,
                       int32_t& departed, int32_t& leaders_moved) {
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (k < olen) {
      const int32_t n = node_of<C16>(L, o[k]);
      bool in_c = false;
#pragma unroll
      for (int j = 0; j < W; ++j) in_c = in_c || (j < clen && c[j] == o[k]);
      if (n >= 0) {
        bump<GLOBAL>(h, n * F + 1, 1);                          // replicas_after
        if (k == 0) bump<GLOBAL>(h, n * F + 3, 1);              // leaders_after
        if (!in_c) bump<GLOBAL>(h, n * F + 4, 1);               // inbound
      }
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (j < clen) {
      const int32_t n = node_of<C16>(L, c[j]);
      bool in_o = false;
#pragma unroll
      for (int k = 0; k < W; ++k) in_o = in_o || (k < olen && o[k] == c[j]);
      if (n >= 0) {
        bump<GLOBAL>(h, n * F + 0, 1);                          // replicas_before
        if (j == 0) bump<GLOBAL>(h, n * F + 2, 1);              // leaders_before
        if (!in_o) bump<GLOBAL>(h, n * F + 5, 1);               // outbound
      } else {
        departed += 1;
      }
    }
  }
  if (olen > 0 && (clen == 0 || o[0] != c[0])) leaders_moved += 1;
}

// rows [lo, hi) of topic td into h (LDS histogram, or the scenario's global region); h[F * N + 0 / 1] = departed / leaders moved
template <int W, bool C16, bool GLOBAL>
KAS_DEV void count_rows(const KasImpactLaunch& a, const kas_topic_desc& td, int32_t lo, int32_t hi, const Lookup& L, int32_t* h,
                        int32_t N) {
  const int32_t tid = kasw::tid();
  const int32_t cw = td.cur_width < W ? td.cur_width : W, ow = td.out_width < W ? td.out_width : W;
  const int32_t* lens = td.cur_len_off >= 0 ? a.aux + td.cur_len_off : nullptr;
  int32_t departed = 0, leaders_moved = 0;
  for (int32_t base = lo; base < hi; base += ROWS_PER_LANE * KAS_IMPACT_BLOCK) {
    int32_t c[ROWS_PER_LANE][W], o[ROWS_PER_LANE][W], clen[ROWS_PER_LANE];
#pragma unroll
    for (int u = 0; u < ROWS_PER_LANE; ++u) {
      const int32_t p = base + u * KAS_IMPACT_BLOCK + tid;
      const bool live = p < hi;
      int32_t cl = live ? (lens ? lens[p] : cw) : 0;
      clen[u] = cl < 0 ? 0 : (cl > cw ? cw : cl);
      const int64_t crow = td.cur_off + (int64_t)p * td.cur_width, orow = td.out_off + (int64_t)p * td.out_width;
#pragma unroll
      for (int k = 0; k < W; ++k) c[u][k] = (live && k < cw) ? cell<C16>(a.cur, crow + k) : -1;
#pragma unroll
      for (int k = 0; k < W; ++k) o[u][k] = (live && k < ow) ? cell<C16>(a.out, orow + k) : -1;
    }
#pragma unroll
    for (int u = 0; u < ROWS_PER_LANE; ++u) {
      int32_t olen = 0;
      bool open = true;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        open = open && k < ow && o[u][k] != -1;                 // (the pad: -1, KAS_CELL16_NONE)
        olen += open ? 1 : 0;
      }
      count_row<W, C16, GLOBAL>(L, c[u], clen[u], o[u], olen, h, departed, leaders_moved);
    }
  }
  departed = kasw::wave_sum(departed);
  leaders_moved = kasw::wave_sum(leaders_moved);
  if (kasw::lane() == 0) {
    if (departed != 0) bump<GLOBAL>(h, F * N, departed);
    if (leaders_moved != 0) bump<GLOBAL>(h, F * N + 1, leaders_moved);
  }
}

KAS_DEV int32_t imax(int32_t x, int32_t y) { return x > y ? x : y; }
KAS_DEV int32_t imin(int32_t x, int32_t y) { return x < y ? x : y; }

// The scenario's node records and its scenario record from its N x 6 counters (+ the two behind them).  red: LDS words.
KAS_DEV void write_records(const KasImpactLaunch& a, int32_t s, int32_t N, const int32_t* h, int32_t* red) {
  const int32_t tid = kasw::tid();
  kas_node_impact* dst = a.nodes + a.node_base[s];
  int32_t v[F] = {0, 0, INT32_MAX, 0, INT32_MAX, 0};   // max inbound, max outbound, min / max replicas after, min / max leaders after
  for (int32_t i = tid; i < N; i += KAS_IMPACT_BLOCK) {
    kas_node_impact r;
    r.replicas_before = h[F * i + 0]; r.replicas_after = h[F * i + 1];
    r.leaders_before = h[F * i + 2]; r.leaders_after = h[F * i + 3];
    r.inbound = h[F * i + 4]; r.outbound = h[F * i + 5];
    r.reserved[0] = 0; r.reserved[1] = 0;
    dst[i] = r;
    v[0] = imax(v[0], r.inbound); v[1] = imax(v[1], r.outbound);
    v[2] = imin(v[2], r.replicas_after); v[3] = imax(v[3], r.replicas_after);
    v[4] = imin(v[4], r.leaders_after); v[5] = imax(v[5], r.leaders_after);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const int32_t w = kasw::shfl(v[f], kasw::lane() ^ o);
      v[f] = (f == 2 || f == 4) ? imin(v[f], w) : imax(v[f], w);
    }
  }
  if (kasw::lane() == 0)
    for (int f = 0; f < F; ++f) red[kasw::wave_id() * F + f] = v[f];
  kasw::sync();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w)
      for (int f = 0; f < F; ++f) v[f] = (f == 2 || f == 4) ? imin(v[f], red[w * F + f]) : imax(v[f], red[w * F + f]);
    kas_scenario_impact r;
    const bool any = N > 0;
    r.departed_replicas = any ? h[F * N] : 0;
    r.leaders_moved = any ? h[F * N + 1] : 0;
    r.max_inbound = any ? v[0] : 0; r.max_outbound = any ? v[1] : 0;
    r.min_replicas_after = any ? v[2] : 0; r.max_replicas_after = any ? v[3] : 0;
    r.min_leaders_after = any ? v[4] : 0; r.max_leaders_after = any ? v[5] : 0;
    a.scenarios[s] = r;
  }
}

// Item kernel body: workgroup `item` of the work list.
template <int W, bool C16>
KAS_DEV void impact_item(const KasImpactLaunch& a, int32_t item, unsigned char* lds) {
  const KasImpactItem it = a.items[item];
  const int32_t s = it.scen;
  const kas_scenario_desc sd = a.scen[s];
  const int32_t N = sd.n_nodes > 0 ? sd.n_nodes : 0;
  const int32_t tid = kasw::tid();
  const bool global = it.mode == KAS_IMPACT_GLOBAL;
  int32_t* const h = global ? a.region + a.region_off[s] : reinterpret_cast<int32_t*>(lds);
  const int32_t status = it.topic >= 0 ? a.topic_results[it.topic].status : -1;
  const bool rows = status == KAS_OK && N > 0 && it.row_hi > it.row_lo;
  if (!global)
    for (int32_t i = tid; i < F * N + KAS_IMPACT_EXTRA; i += KAS_IMPACT_BLOCK) h[i] = 0;
  Lookup L;
  L.map = reinterpret_cast<const int16_t*>(lds + a.off_look);
  L.ids = reinterpret_cast<const int32_t*>(lds + a.off_look);
  L.min_id = 0; L.range = 0u; L.n = N;
  if constexpr (!C16) {
    if (rows) {
      const int32_t* g_id = a.node_id + sd.node_off;
      const int64_t lo_id = g_id[0], range = (int64_t)g_id[N - 1] - lo_id + 1;
      if (range >= 1 && range <= (int64_t)a.idmap_entries) {
        int16_t* map = reinterpret_cast<int16_t*>(lds + a.off_look);
        for (int32_t i = tid; i < (int32_t)range; i += KAS_IMPACT_BLOCK) map[i] = -1;
        kasw::sync();
        for (int32_t i = tid; i < N; i += KAS_IMPACT_BLOCK) {
          const int64_t d = (int64_t)g_id[i] - lo_id;
          if (d >= 0 && d < range) map[d] = (int16_t)i;
        }
        L.min_id = (int32_t)lo_id; L.range = (uint32_t)range;
      } else {
        int32_t* ids = reinterpret_cast<int32_t*>(lds + a.off_look);
        for (int32_t i = tid; i < N; i += KAS_IMPACT_BLOCK) ids[i] = g_id[i];
      }
    }
  }
  kasw::sync();
  if (rows) {
    const kas_topic_desc td = a.topics[it.topic];
    if (global) count_rows<W, C16, true>(a, td, it.row_lo, it.row_hi, L, h, N);
    else count_rows<W, C16, false>(a, td, it.row_lo, it.row_hi, L, h, N);
  }
  kasw::sync();
  if (it.mode == KAS_IMPACT_DIRECT) {
    write_records(a, s, N, h, reinterpret_cast<int32_t*>(lds + a.off_red));
  } else if (it.mode == KAS_IMPACT_FLUSH) {
    int32_t* g = a.region + a.region_off[s];
    for (int32_t i = tid; i < F * N + KAS_IMPACT_EXTRA; i += KAS_IMPACT_BLOCK) {
      const int32_t c = h[i];
      if (c != 0) kasw::global_atomic_add(g + i, c);
    }
  }
}

// Merge kernel body: the records of scenario merge_scen[m] from its global counters.  red: F * WAVES int32 of LDS.
KAS_DEV void impact_merge(const KasImpactLaunch& a, int32_t m, int32_t* red) {
  const int32_t s = a.merge_scen[m];
  const int32_t N = a.scen[s].n_nodes > 0 ? a.scen[s].n_nodes : 0;
  write_records(a, s, N, a.region + a.region_off[s], red);
}

}  // namespace kasi
