// kas_racks_body.h — device code of the rack pass (launch arguments and host tables: kas_racks.h).
//
// Row kernel: one workgroup of KAS_RACK_BLOCK lanes per item of the impact pass's work list.  It stages the scenario's
// id -> node lookup in the LDS exactly as kasi::impact_item does and, next to it, the scenario's report racks as uint16 per node
// (where the two do not fit, the racks are read from global memory), then streams the rows as kasi::count_rows does: consecutive
// lanes on consecutive rows, two rows per lane per step, a row's cells in registers.  A cell is the first of its rack if no
// earlier known cell of its list has its rack: dB, dA and new_rack_replicas are pairwise compares in registers, the eight row
// sums live in per-lane registers, and the only atomics are eight per wave at the end.
// Reduce kernel: one workgroup per scenario; the node records by rack into the LDS, then the records.
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/rack_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_impact_body.h"
#include "kas_racks.h"
#include "kas_wave.h"

namespace kasr {

constexpr int NS = KAS_RACK_SUMS;
constexpr int RF = KAS_RACK_FIELDS;
constexpr int WAVES = KAS_RACK_BLOCK / 64;

// node index -> report rack
struct Racks {
  const uint16_t* lds;    // staged racks, or
  const int32_t* glob;    // the scenario's stretch of the global table
};

template <bool LDS>
KAS_DEV int32_t rack_of(const Racks& R, int32_t n) {
  if (n < 0) return -1;
  if constexpr (LDS) return (int32_t)R.lds[n];
  else return R.glob[n];
}

// one row: C = c[0, clen), O = o[0, olen) into the lane's eight sums
template <int W, bool C16, bool LDS>
KAS_DEV void rack_row(const kasi::Lookup& L, const Racks& R, const int32_t (&c)[W], int32_t clen, const int32_t (&o)[W], int32_t olen,
                      int32_t (&sum)[NS]) {
  int32_t rc[W], ro[W];                                          // a cell's rack; -1: names no node (or beyond the list)
#pragma unroll
  for (int j = 0; j < W; ++j) rc[j] = j < clen ? rack_of<LDS>(R, kasi::node_of<C16>(L, c[j])) : -1;
#pragma unroll
  for (int k = 0; k < W; ++k) ro[k] = k < olen ? rack_of<LDS>(R, kasi::node_of<C16>(L, o[k])) : -1;
  int32_t kB = 0, dB = 0, kA = 0, dA = 0, fresh = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    bool first = rc[j] >= 0;
#pragma unroll
    for (int i = 0; i < j; ++i) first = first && rc[i] != rc[j];
    kB += rc[j] >= 0 ? 1 : 0;
    dB += first ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    bool first = ro[k] >= 0, in_c = false, rack_in_c = false;
#pragma unroll
    for (int i = 0; i < k; ++i) first = first && ro[i] != ro[k];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      in_c = in_c || (j < clen && c[j] == o[k]);
      rack_in_c = rack_in_c || rc[j] == ro[k];                   // (rc[j] >= 0 where it equals a known rack)
    }
    kA += ro[k] >= 0 ? 1 : 0;
    dA += first ? 1 : 0;
    fresh += (ro[k] >= 0 && !in_c && !rack_in_c) ? 1 : 0;
  }
  sum[0] += kB - dB; sum[1] += kA - dA;
  sum[2] += kB > dB ? 1 : 0; sum[3] += kA > dA ? 1 : 0;
  sum[4] += (kB >= 2 && dB == 1) ? 1 : 0; sum[5] += (kA >= 2 && dA == 1) ? 1 : 0;
  sum[6] += fresh;
  sum[7] += dA < dB ? 1 : 0;
}

// rows [lo, hi) of topic td into the scenario's eight words of a.sums
template <int W, bool C16, bool LDS>
KAS_DEV void rack_rows(const KasRackLaunch& a, const kas_topic_desc& td, int32_t lo, int32_t hi, const kasi::Lookup& L, const Racks& R,
                       int32_t* g) {
  constexpr int RPL = kasi::ROWS_PER_LANE;
  const int32_t tid = kasw::tid();
  const int32_t cw = td.cur_width < W ? td.cur_width : W, ow = td.out_width < W ? td.out_width : W;
  const int32_t* lens = td.cur_len_off >= 0 ? a.aux + td.cur_len_off : nullptr;
  int32_t sum[NS];
#pragma unroll
  for (int f = 0; f < NS; ++f) sum[f] = 0;
  for (int32_t base = lo; base < hi; base += RPL * KAS_RACK_BLOCK) {
    int32_t c[RPL][W], o[RPL][W], clen[RPL];
#pragma unroll
    for (int u = 0; u < RPL; ++u) {
      const int32_t p = base + u * KAS_RACK_BLOCK + tid;
      const bool live = p < hi;
      int32_t cl = live ? (lens ? lens[p] : cw) : 0;
      clen[u] = cl < 0 ? 0 : (cl > cw ? cw : cl);
      const int64_t crow = td.cur_off + (int64_t)p * td.cur_width, orow = td.out_off + (int64_t)p * td.out_width;
#pragma unroll
      for (int k = 0; k < W; ++k) c[u][k] = (live && k < cw) ? kasi::cell<C16>(a.cur, crow + k) : -1;
#pragma unroll
      for (int k = 0; k < W; ++k) o[u][k] = (live && k < ow) ? kasi::cell<C16>(a.out, orow + k) : -1;
    }
#pragma unroll
    for (int u = 0; u < RPL; ++u) {
      int32_t olen = 0;
      bool open = true;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        open = open && k < ow && o[u][k] != -1;                 // (the pad: -1, KAS_CELL16_NONE)
        olen += open ? 1 : 0;
      }
      rack_row<W, C16, LDS>(L, R, c[u], clen[u], o[u], olen, sum);
    }
  }
#pragma unroll
  for (int f = 0; f < NS; ++f) {
    const int32_t v = kasw::wave_sum(sum[f]);
    if (kasw::lane() == 0 && v != 0) kasw::global_atomic_add(g + f, v);
  }
}

// Row kernel body: workgroup `item` of the impact pass's work list.
template <int W, bool C16>
KAS_DEV void rack_item(const KasRackLaunch& a, int32_t item, unsigned char* lds) {
  const KasImpactItem it = a.items[item];
  const int32_t s = it.scen;
  const kas_scenario_desc sd = a.scen[s];
  const int32_t N = sd.n_nodes > 0 ? sd.n_nodes : 0;
  const int32_t tid = kasw::tid();
  const int32_t status = it.topic >= 0 ? a.topic_results[it.topic].status : -1;
  if (!(status == KAS_OK && N > 0 && it.row_hi > it.row_lo)) return;       // (uniform over the workgroup: nobody waits at a barrier)
  kasi::Lookup L;
  L.map = reinterpret_cast<const int16_t*>(lds);
  L.ids = reinterpret_cast<const int32_t*>(lds);
  L.min_id = 0; L.range = 0u; L.n = N;
  if constexpr (!C16) {
    const int32_t* g_id = a.node_id + sd.node_off;
    const int64_t lo_id = g_id[0], range = (int64_t)g_id[N - 1] - lo_id + 1;
    if (range >= 1 && range <= (int64_t)a.idmap_entries) {
      int16_t* map = reinterpret_cast<int16_t*>(lds);
      for (int32_t i = tid; i < (int32_t)range; i += KAS_RACK_BLOCK) map[i] = -1;
      kasw::sync();
      for (int32_t i = tid; i < N; i += KAS_RACK_BLOCK) {
        const int64_t d = (int64_t)g_id[i] - lo_id;
        if (d >= 0 && d < range) map[d] = (int16_t)i;
      }
      L.min_id = (int32_t)lo_id; L.range = (uint32_t)range;
    } else {
      int32_t* ids = reinterpret_cast<int32_t*>(lds);
      for (int32_t i = tid; i < N; i += KAS_RACK_BLOCK) ids[i] = g_id[i];
    }
  }
  Racks R;
  R.lds = reinterpret_cast<const uint16_t*>(lds + a.off_rack);
  R.glob = a.rr + sd.node_off;
  if (a.racks_in_lds) {
    uint16_t* r16 = reinterpret_cast<uint16_t*>(lds + a.off_rack);
    for (int32_t i = tid; i < N; i += KAS_RACK_BLOCK) r16[i] = (uint16_t)R.glob[i];
  }
  kasw::sync();
  const kas_topic_desc td = a.topics[it.topic];
  int32_t* g = a.sums + (int64_t)s * NS;
  if (a.racks_in_lds) rack_rows<W, C16, true>(a, td, it.row_lo, it.row_hi, L, R, g);
  else rack_rows<W, C16, false>(a, td, it.row_lo, it.row_hi, L, R, g);
}

// Reduce kernel body: the rack records and the scenario record of scenario s.  lds: KAS_RACK_FIELDS x r_max int32, then
// KAS_RACK_RED x WAVES reduction words (a.reduce_lds_bytes in all).
KAS_DEV void rack_reduce(const KasRackLaunch& a, int32_t s, unsigned char* lds) {
  const int32_t tid = kasw::tid();
  const kas_scenario_desc sd = a.scen[s];
  const int32_t N = sd.n_nodes > 0 ? sd.n_nodes : 0;
  const int32_t R = (int32_t)(a.rack_off[s + 1] - a.rack_off[s]);
  int32_t* h = reinterpret_cast<int32_t*>(lds);
  int32_t* red = reinterpret_cast<int32_t*>(lds + a.reduce_lds_bytes - 4 * KAS_RACK_RED * WAVES);
  for (int32_t i = tid; i < RF * R; i += KAS_RACK_BLOCK) h[i] = 0;
  kasw::sync();
  const kas_node_impact* src = a.nodes + a.node_base[s];
  const int32_t* rr = a.rr + sd.node_off;
  for (int32_t i = tid; i < N; i += KAS_RACK_BLOCK) {
    const kas_node_impact r = src[i];
    const int32_t k = rr[i];
    if ((uint32_t)k >= (uint32_t)R) continue;                    // (the host refused such a table: never taken)
    uint32_t* w = reinterpret_cast<uint32_t*>(h + RF * k);
    kasw::lds_add_u32(w + 0, 1u);
    if (r.replicas_before != 0) kasw::lds_add_u32(w + 1, (uint32_t)r.replicas_before);
    if (r.replicas_after != 0) kasw::lds_add_u32(w + 2, (uint32_t)r.replicas_after);
    if (r.leaders_before != 0) kasw::lds_add_u32(w + 3, (uint32_t)r.leaders_before);
    if (r.leaders_after != 0) kasw::lds_add_u32(w + 4, (uint32_t)r.leaders_after);
    if (r.inbound != 0) kasw::lds_add_u32(w + 5, (uint32_t)r.inbound);
    if (r.outbound != 0) kasw::lds_add_u32(w + 6, (uint32_t)r.outbound);
  }
  kasw::sync();
  kas_rack_impact* dst = a.racks + a.rack_off[s];
  int32_t v[KAS_RACK_RED] = {0, 0, INT32_MAX, 0, INT32_MAX, 0};   // max inbound, max outbound, min / max replicas after, min / max leaders after
  for (int32_t k = tid; k < R; k += KAS_RACK_BLOCK) {
    kas_rack_impact r;
    r.nodes = h[RF * k + 0];
    r.replicas_before = h[RF * k + 1]; r.replicas_after = h[RF * k + 2];
    r.leaders_before = h[RF * k + 3]; r.leaders_after = h[RF * k + 4];
    r.inbound = h[RF * k + 5]; r.outbound = h[RF * k + 6];
    r.reserved = 0;
    dst[k] = r;
    v[0] = kasi::imax(v[0], r.inbound); v[1] = kasi::imax(v[1], r.outbound);
    v[2] = kasi::imin(v[2], r.replicas_after); v[3] = kasi::imax(v[3], r.replicas_after);
    v[4] = kasi::imin(v[4], r.leaders_after); v[5] = kasi::imax(v[5], r.leaders_after);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int f = 0; f < KAS_RACK_RED; ++f) {
      const int32_t w = kasw::shfl(v[f], kasw::lane() ^ o);
      v[f] = (f == 2 || f == 4) ? kasi::imin(v[f], w) : kasi::imax(v[f], w);
    }
  }
  if (kasw::lane() == 0)
    for (int f = 0; f < KAS_RACK_RED; ++f) red[kasw::wave_id() * KAS_RACK_RED + f] = v[f];
  kasw::sync();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w)
      for (int f = 0; f < KAS_RACK_RED; ++f)
        v[f] = (f == 2 || f == 4) ? kasi::imin(v[f], red[w * KAS_RACK_RED + f]) : kasi::imax(v[f], red[w * KAS_RACK_RED + f]);
    const int32_t* g = a.sums + (int64_t)s * NS;
    const bool any = N > 0 && R > 0;
    kas_scenario_rack_impact r;
    r.colocated_before = any ? g[0] : 0; r.colocated_after = any ? g[1] : 0;
    r.rows_colocated_before = any ? g[2] : 0; r.rows_colocated_after = any ? g[3] : 0;
    r.single_rack_rows_before = any ? g[4] : 0; r.single_rack_rows_after = any ? g[5] : 0;
    r.new_rack_replicas = any ? g[6] : 0; r.rows_losing_racks = any ? g[7] : 0;
    r.n_racks = any ? R : 0;
    r.max_rack_inbound = any ? v[0] : 0; r.max_rack_outbound = any ? v[1] : 0;
    r.min_rack_replicas_after = any ? v[2] : 0; r.max_rack_replicas_after = any ? v[3] : 0;
    r.min_rack_leaders_after = any ? v[4] : 0; r.max_rack_leaders_after = any ? v[5] : 0;
    r.reserved = 0;
    a.scenarios[s] = r;
  }
}

}  // namespace kasr
