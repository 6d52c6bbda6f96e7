// kas_topics_body.h — device code of the topic pass (work list and launch arguments: kas_topics.h).
//
// Item kernel: one workgroup of KAS_TOPIC_BLOCK lanes per (scenario, topic, row range).  It reads the topic's status once, stages
// the scenario's id -> node lookup in the LDS as the impact pass does (kasi::Lookup), zeroes a histogram of N x 4 int32 and
// streams the rows: consecutive lanes on consecutive rows, two rows per lane per step, a row's cells in registers, set
// membership by compares, every count a no-return LDS add.  Merge kernel: one workgroup per topic whose counters sit in global
// scratch.  Summary kernel: one workgroup per scenario over the topic records, no atomics.
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/topic_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_impact_body.h"   // kasi::cell, Lookup, node_of, bump, imax / imin
#include "kas_topics.h"
#include "kas_wave.h"

namespace kast {

constexpr int F = KAS_TOPIC_FIELDS;       // per node: 0 replicas after, 1 leaders after, 2 inbound, 3 outbound
constexpr int WAVES = KAS_TOPIC_BLOCK / 64;
constexpr int ROWS_PER_LANE = 2;          // rows a lane loads before it counts them
using kasi::imax;
using kasi::imin;

// one row: C = c[0, clen), O = o[0, olen)
template <int W, bool C16, bool GLOBAL>
KAS_DEV void count_topic_row(const kasi::Lookup& L, const int32_t (&c)[W], int32_t clen, const int32_t (&o)[W], int32_t olen, int32_t* h,
                       int32_t& departed, int32_t& leaders_moved) {
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (k < olen) {
      const int32_t n = kasi::node_of<C16>(L, o[k]);
      bool in_c = false;
#pragma unroll
      for (int j = 0; j < W; ++j) in_c = in_c || (j < clen && c[j] == o[k]);
      if (n >= 0) {
        kasi::bump<GLOBAL>(h, n * F + 0, 1);                        // replicas after
        if (k == 0) kasi::bump<GLOBAL>(h, n * F + 1, 1);            // leaders after
        if (!in_c) kasi::bump<GLOBAL>(h, n * F + 2, 1);             // inbound
      }
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (j < clen) {
      const int32_t n = kasi::node_of<C16>(L, c[j]);
      bool in_o = false;
#pragma unroll
      for (int k = 0; k < W; ++k) in_o = in_o || (k < olen && o[k] == c[j]);
      if (n >= 0) {
        if (!in_o) kasi::bump<GLOBAL>(h, n * F + 3, 1);             // outbound
      } else {
        departed += 1;
      }
    }
  }
  if (olen > 0 && (clen == 0 || o[0] != c[0])) leaders_moved += 1;
}

// rows [lo, hi) of topic td into h (LDS histogram, or the topic's global region); h[F * N + 0 / 1] = departed / leaders moved
template <int W, bool C16, bool GLOBAL>
KAS_DEV void count_topic_rows(const KasTopicLaunch& a, const kas_topic_desc& td, int32_t lo, int32_t hi, const kasi::Lookup& L, int32_t* h,
                        int32_t N) {
  const int32_t tid = kasw::tid();
  const int32_t cw = td.cur_width < W ? td.cur_width : W, ow = td.out_width < W ? td.out_width : W;
  const int32_t* lens = td.cur_len_off >= 0 ? a.aux + td.cur_len_off : nullptr;
  int32_t departed = 0, leaders_moved = 0;
  for (int32_t base = lo; base < hi; base += ROWS_PER_LANE * KAS_TOPIC_BLOCK) {
    int32_t c[ROWS_PER_LANE][W], o[ROWS_PER_LANE][W], clen[ROWS_PER_LANE];
#pragma unroll
    for (int u = 0; u < ROWS_PER_LANE; ++u) {
      const int32_t p = base + u * KAS_TOPIC_BLOCK + tid;
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
    for (int u = 0; u < ROWS_PER_LANE; ++u) {
      int32_t olen = 0;
      bool open = true;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        open = open && k < ow && o[u][k] != -1;                 // (the pad: -1, KAS_CELL16_NONE)
        olen += open ? 1 : 0;
      }
      count_topic_row<W, C16, GLOBAL>(L, c[u], clen[u], o[u], olen, h, departed, leaders_moved);
    }
  }
  departed = kasw::wave_sum(departed);
  leaders_moved = kasw::wave_sum(leaders_moved);
  if (kasw::lane() == 0) {
    if (departed != 0) kasi::bump<GLOBAL>(h, F * N, departed);
    if (leaders_moved != 0) kasi::bump<GLOBAL>(h, F * N + 1, leaders_moved);
  }
}

// Topic t's record from its N x 4 counters (+ the two behind them).  red: KAS_TOPIC_RED * WAVES int32 of LDS.
KAS_DEV void write_record(const KasTopicLaunch& a, int32_t t, int32_t N, const int32_t* h, int32_t* red) {
  const int32_t tid = kasw::tid();
  constexpr int R = KAS_TOPIC_RED;
  int32_t v[R] = {0, 0, INT32_MAX, 0, INT32_MAX, 0};   // max inbound, max outbound, min / max replicas after, min / max leaders after
  for (int32_t i = tid; i < N; i += KAS_TOPIC_BLOCK) {
    const int32_t ra = h[F * i + 0], la = h[F * i + 1];
    v[0] = imax(v[0], h[F * i + 2]); v[1] = imax(v[1], h[F * i + 3]);
    v[2] = imin(v[2], ra); v[3] = imax(v[3], ra);
    v[4] = imin(v[4], la); v[5] = imax(v[5], la);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int f = 0; f < R; ++f) {
      const int32_t w = kasw::shfl(v[f], kasw::lane() ^ o);
      v[f] = (f == 2 || f == 4) ? imin(v[f], w) : imax(v[f], w);
    }
  }
  if (kasw::lane() == 0)
    for (int f = 0; f < R; ++f) red[kasw::wave_id() * R + f] = v[f];
  kasw::sync();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w)
      for (int f = 0; f < R; ++f) v[f] = (f == 2 || f == 4) ? imin(v[f], red[w * R + f]) : imax(v[f], red[w * R + f]);
    kas_topic_impact r;
    const bool any = N > 0 && a.topic_results[t].status == KAS_OK;
    r.departed_replicas = any ? h[F * N] : 0;
    r.leaders_moved = any ? h[F * N + 1] : 0;
    r.max_inbound = any ? v[0] : 0; r.max_outbound = any ? v[1] : 0;
    r.min_replicas_after = any ? v[2] : 0; r.max_replicas_after = any ? v[3] : 0;
    r.min_leaders_after = any ? v[4] : 0; r.max_leaders_after = any ? v[5] : 0;
    a.topic_out[t] = r;
  }
}

// Item kernel body: workgroup `item` of the work list.
template <int W, bool C16>
KAS_DEV void topic_item(const KasTopicLaunch& a, int32_t item, unsigned char* lds) {
  const KasImpactItem it = a.items[item];
  const int32_t s = it.scen, t = it.topic;
  const kas_scenario_desc sd = a.scen[s];
  const int32_t N = sd.n_nodes > 0 ? sd.n_nodes : 0;
  const int32_t tid = kasw::tid();
  const bool global = it.mode == KAS_TOPIC_GLOBAL;
  int32_t* const h = global ? a.region + a.region_off[t] : reinterpret_cast<int32_t*>(lds);
  const bool rows = a.topic_results[t].status == KAS_OK && N > 0 && it.row_hi > it.row_lo;
  if (!global)
    for (int32_t i = tid; i < F * N + KAS_TOPIC_EXTRA; i += KAS_TOPIC_BLOCK) h[i] = 0;
  kasi::Lookup L;
  L.map = reinterpret_cast<const int16_t*>(lds + a.off_look);
  L.ids = reinterpret_cast<const int32_t*>(lds + a.off_look);
  L.min_id = 0; L.range = 0u; L.n = N;
  if constexpr (!C16) {
    if (rows) {
      const int32_t* g_id = a.node_id + sd.node_off;
      const int64_t lo_id = g_id[0], range = (int64_t)g_id[N - 1] - lo_id + 1;
      if (range >= 1 && range <= (int64_t)a.idmap_entries) {
        int16_t* map = reinterpret_cast<int16_t*>(lds + a.off_look);
        for (int32_t i = tid; i < (int32_t)range; i += KAS_TOPIC_BLOCK) map[i] = -1;
        kasw::sync();
        for (int32_t i = tid; i < N; i += KAS_TOPIC_BLOCK) {
          const int64_t d = (int64_t)g_id[i] - lo_id;
          if (d >= 0 && d < range) map[d] = (int16_t)i;
        }
        L.min_id = (int32_t)lo_id; L.range = (uint32_t)range;
      } else {
        int32_t* ids = reinterpret_cast<int32_t*>(lds + a.off_look);
        for (int32_t i = tid; i < N; i += KAS_TOPIC_BLOCK) ids[i] = g_id[i];
      }
    }
  }
  kasw::sync();
  if (rows) {
    const kas_topic_desc td = a.topics[t];
    if (global) count_topic_rows<W, C16, true>(a, td, it.row_lo, it.row_hi, L, h, N);
    else count_topic_rows<W, C16, false>(a, td, it.row_lo, it.row_hi, L, h, N);
  }
  kasw::sync();
  if (it.mode == KAS_TOPIC_DIRECT) {
    write_record(a, t, N, h, reinterpret_cast<int32_t*>(lds + a.off_red));
  } else if (it.mode == KAS_TOPIC_FLUSH) {
    int32_t* g = a.region + a.region_off[t];
    for (int32_t i = tid; i < F * N + KAS_TOPIC_EXTRA; i += KAS_TOPIC_BLOCK) {
      const int32_t c = h[i];
      if (c != 0) kasw::global_atomic_add(g + i, c);
    }
  }
}

// Merge kernel body: the record of topic merge[m] from its global counters.  red: KAS_TOPIC_RED * WAVES int32 of LDS.
KAS_DEV void topic_merge(const KasTopicLaunch& a, int32_t m, int32_t* red) {
  const KasTopicMerge mt = a.merge[m];
  const int32_t N = a.scen[mt.scen].n_nodes > 0 ? a.scen[mt.scen].n_nodes : 0;
  write_record(a, mt.topic, N, a.region + a.region_off[mt.topic], red);
}

// Summary kernel body: scenario s's sixteen words from its topics' records and results.  red: KAS_TOPIC_WORDS * WAVES int32 of
// LDS.  Words 0-3, 13 and 14 are sums, the others maxima; every word is non-negative, so both start from 0.
KAS_DEV bool summed(int f) { return f < 4 || f == 13 || f == 14; }

KAS_DEV void topic_summary(const KasTopicLaunch& a, int32_t s, int32_t* red) {
  constexpr int Wn = KAS_TOPIC_WORDS;
  const int32_t tid = kasw::tid();
  const kas_scenario_desc sd = a.scen[s];
  int32_t v[Wn];
#pragma unroll
  for (int f = 0; f < Wn; ++f) v[f] = 0;
  for (int32_t k = tid; k < sd.topic_count; k += KAS_TOPIC_BLOCK) {
    const int32_t t = sd.topic_begin + k;
    const kas_topic_result tr = a.topic_results[t];
    if (tr.status != KAS_OK) continue;
    const kas_topic_impact r = a.topic_out[t];
    const int32_t rs = r.max_replicas_after - r.min_replicas_after, ls = r.max_leaders_after - r.min_leaders_after;
    v[0] += 1;
    v[1] += tr.moved_replicas > 0 ? 1 : 0;
    v[2] += r.leaders_moved > 0 ? 1 : 0;
    v[3] += r.departed_replicas > 0 ? 1 : 0;
    v[4] = imax(v[4], tr.moved_replicas); v[5] = imax(v[5], tr.moved_partitions);
    v[6] = imax(v[6], r.leaders_moved);
    v[7] = imax(v[7], r.max_inbound); v[8] = imax(v[8], r.max_outbound);
    v[9] = imax(v[9], rs); v[10] = imax(v[10], ls);
    v[11] = imax(v[11], r.max_replicas_after); v[12] = imax(v[12], r.max_leaders_after);
    v[13] += rs; v[14] += ls;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int f = 0; f < Wn - 1; ++f) {
      const int32_t w = kasw::shfl(v[f], kasw::lane() ^ o);
      v[f] = summed(f) ? v[f] + w : imax(v[f], w);
    }
  }
  if (kasw::lane() == 0)
    for (int f = 0; f < Wn - 1; ++f) red[kasw::wave_id() * Wn + f] = v[f];
  kasw::sync();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w)
      for (int f = 0; f < Wn - 1; ++f) v[f] = summed(f) ? v[f] + red[w * Wn + f] : imax(v[f], red[w * Wn + f]);
    kas_scenario_topic_impact r;
    r.topics_ok = v[0]; r.topics_moved = v[1]; r.topics_leaders_moved = v[2]; r.topics_departed = v[3];
    r.max_topic_moved_replicas = v[4]; r.max_topic_moved_partitions = v[5]; r.max_topic_leaders_moved = v[6];
    r.max_topic_inbound = v[7]; r.max_topic_outbound = v[8];
    r.max_topic_replica_spread = v[9]; r.max_topic_leader_spread = v[10];
    r.max_topic_replicas_after = v[11]; r.max_topic_leaders_after = v[12];
    r.sum_topic_replica_spread = v[13]; r.sum_topic_leader_spread = v[14];
    r.reserved = 0;
    a.scenarios[s] = r;
  }
}

}  // namespace kast
