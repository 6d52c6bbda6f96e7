// kas_rounds_body.h — device code of the rounds pass (launch arguments and LDS layout: kas_rounds.h).
//
// One workgroup of KAS_ROUND_BLOCK lanes per listed scenario.  It stages the scenario's id -> node lookup in the LDS as the
// batches pass does, zeroes one 32-bit word per node and direction — (round the node is filling) << shift | moves it holds
// there, the split chosen for the scenario's row count (kas_round_bits) — and walks the scenario's rows tile by tile:
//   load     kasb::load_tile (kas_batches_body.h, shared by inclusion): the tile's REPLICAS moves become queue entries in row
//            order, In and Out node indices as uint16; positions come from ballots.
//   walk     wavefront 0 takes the queue one move a step — exactly the loop of include/kas_abi.h.  Lane k < W holds the move's
//            k-th In cell, lane W + k its k-th Out cell; each reads its node's word, the candidates are gathered with
//            v_readlane into scalar maxima (In and Out apart: which side raised the move), and the lanes write their words
//            back.  The nodes of one move are distinct per direction, so the lanes of a step never share a word.  The round
//            goes into the entry's topic word, which this pass has no use for.
//   count    all lanes: one entry each, the round's counters in the LDS window get no-return adds (moves, replicas) and a
//            no-return min (first move) — sums and minima do not depend on the order — and round_of[i] a plain vector store.
// The window holds the counters of KAS_ROUND_WINDOW rounds.  At the scenario's end its rounds below n_rounds give the maxima and
// go out as records with plain stores; a scenario of more rounds than the window is walked again for the next window (the walk
// is a function of the tables alone, so every walk gives every move the round it had).  Nothing is zeroed or added to in global
// memory, so nothing at or beyond the written prefixes is touched.
//
// No position and no decision comes from the return value of an atomic, and nothing depends on the order in which the LDS serves
// the lanes of one instruction.  Every sync() is in workgroup-uniform control flow.
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/rounds_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_rounds.h"
#include "kas_batches_body.h"  // kasb::load_tile, kasb::Lds; kasi::Lookup, kasi::node_of
#include "kas_wave.h"

namespace kasr {

constexpr uint32_t NONE = KAS_BATCH_NODE_NONE;
constexpr int32_t NO_MOVE = 0x7fffffff;

// words of the misc region this pass uses itself (kasb::load_tile uses those from kasb::M_SUB on)
enum { M_NR = 0, M_MAXM = 1, M_MAXR = 2 };
static_assert(M_MAXR < kasb::M_SUB && 4 * kasb::M_WORDS <= KAS_ROUND_MISC_BYTES, "the misc words fit their region");

// the scenario's sums: wavefront 0 holds them, every lane of it alike
struct State { int32_t moves, reps, top, by_in, by_out; };   // top: 1 + the highest round so far

// Wavefront 0, all 64 lanes: the queue's moves [0, g), one a step.  capi / capo: the caps as they apply to this scenario (0: no
// bound); shift: where a word's round begins.
template <int W>
KAS_DEV void walk(uint32_t capi, uint32_t capo, int32_t shift, int32_t N, uint32_t* st, const kasb::Lds<W>& l, State& s, int32_t g) {
  const int32_t lane = kasw::lane();
  const bool has = lane < 2 * W, inb = lane < W;
  const uint32_t cap = inb ? capi : capo;
  const uint32_t used_mask = (1u << shift) - 1u;
  uint32_t node = (has && g > 0) ? (uint32_t)l.qn[lane] : NONE;
  for (int32_t m = 0; m < g; ++m) {
    // (the next move's cell is asked for before this move's word: one LDS round trip a move, not two)
    const uint32_t next = (has && m + 1 < g) ? (uint32_t)l.qn[(m + 1) * 2 * W + lane] : NONE;
    const bool named = node != NONE;
    const bool on = named && cap != 0u;
    uint32_t* const word = st + (inb ? 0 : N) + (on ? (int32_t)node : 0);
    const uint32_t w = on ? *word : 0u;
    const int32_t rd = (int32_t)(w >> shift);
    const uint32_t used = w & used_mask;
    const int32_t cand = on ? (used < cap ? rd : rd + 1) : 0;
    int32_t ri = 0, ro = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const int32_t ci = kasw::read_lane(cand, k), co = kasw::read_lane(cand, W + k);
      ri = ci > ri ? ci : ri; ro = co > ro ? co : ro;
    }
    const int32_t r = ri > ro ? ri : ro;
    if (on) *word = ((uint32_t)r << shift) | (rd == r ? used + 1u : 1u);
    s.reps += kasw::popc(kasw::ballot(named && inb));
    s.moves += 1;
    s.top = r + 1 > s.top ? r + 1 : s.top;
    s.by_in += (r > 0 && ri == r) ? 1 : 0;
    s.by_out += (r > 0 && ri < r) ? 1 : 0;
    if (lane == 0) l.qtp[2 * m] = r;
    kasw::lockstep();
    node = next;
  }
}

// Kernel body: workgroup j = listed scenario j.
template <int W, bool C16>
KAS_DEV void rounds_scenario(const KasRoundsLaunch& a, int32_t j, unsigned char* lds) {
  const int32_t tid = kasw::tid(), wave = kasw::wave_id();
  const int32_t sidx = a.select[j];
  if (sidx < 0 || sidx >= a.S) {                                // an empty slot: zeros (the same for every lane)
    if (tid == 0) { kas_scenario_rounds r = {0, 0, 0, 0, 0, 0, 0, 0}; a.scenarios[j] = r; }
    return;
  }
  const KasMovesScen z = a.scen[sidx];
  const kas_scenario_desc sd = a.sdesc[sidx];
  const int32_t N = sd.n_nodes > 0 ? (sd.n_nodes < a.n_cap ? sd.n_nodes : a.n_cap) : 0;
  uint32_t* const st = reinterpret_cast<uint32_t*>(lds);        // in[N] then out[N]
  uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + a.lds.off_misc);
  uint32_t* const win_m = reinterpret_cast<uint32_t*>(lds + a.lds.off_win);
  uint32_t* const win_r = win_m + KAS_ROUND_WINDOW;
  int32_t* const win_f = reinterpret_cast<int32_t*>(win_r + KAS_ROUND_WINDOW);
  kasb::Lds<W> l;
  l.ctr = nullptr;
  l.misc = misc;
  l.qn = reinterpret_cast<uint16_t*>(lds + a.lds.off_qn);
  l.qtp = reinterpret_cast<int32_t*>(lds + a.lds.off_qtp);
  KasBatchesLaunch b = {};                                      // what kasb::load_tile reads of its launch: the tables
  b.cur = a.cur; b.out = a.out; b.aux = a.aux;
  kasi::Lookup L;
  L.map = reinterpret_cast<const int16_t*>(lds + a.lds.off_look);
  L.ids = reinterpret_cast<const int32_t*>(lds + a.lds.off_look);
  L.min_id = 0; L.range = 0u; L.n = N;
  if constexpr (!C16) {
    if (N > 0) {
      const int32_t* g_id = a.node_id + sd.node_off;
      const int64_t lo_id = g_id[0], range = (int64_t)g_id[N - 1] - lo_id + 1;
      if (range >= 1 && range <= 2 * (int64_t)a.n_cap) {        // (the lookup words hold 2 x n_cap int16)
        int16_t* map = reinterpret_cast<int16_t*>(lds + a.lds.off_look);
        for (int32_t i = tid; i < (int32_t)range; i += KAS_ROUND_BLOCK) map[i] = -1;
        kasw::sync();
        for (int32_t i = tid; i < N; i += KAS_ROUND_BLOCK) {
          const int64_t d = (int64_t)g_id[i] - lo_id;
          if (d >= 0 && d < range) map[d] = (int16_t)i;
        }
        L.min_id = (int32_t)lo_id; L.range = (uint32_t)range;
      } else {
        int32_t* ids = reinterpret_cast<int32_t*>(lds + a.lds.off_look);
        for (int32_t i = tid; i < N; i += KAS_ROUND_BLOCK) ids[i] = g_id[i];
      }
    }
  }
  if (tid == 0) { misc[M_MAXM] = 0u; misc[M_MAXR] = 0u; }
  // the word's split and the caps as they apply here: a cap above the scenario's rows never binds (kas_rounds.h; the host has
  // refused a cap that does not fit its bits)
  const int64_t rows = kas_round_rows(a.scen, a.segs, sidx);
  const int32_t shift = 32 - kas_round_bits(rows);
  const uint32_t capi = (int64_t)a.spec.cap_inbound > rows ? 0u : (uint32_t)a.spec.cap_inbound;
  const uint32_t capo = (int64_t)a.spec.cap_outbound > rows ? 0u : (uint32_t)a.spec.cap_outbound;
  State s;
  for (int32_t base = 0;; base += KAS_ROUND_WINDOW) {           // one walk per window of rounds: nearly always one
    for (int32_t i = tid; i < 2 * N; i += KAS_ROUND_BLOCK) st[i] = 0u;
    for (int32_t i = tid; i < KAS_ROUND_WINDOW; i += KAS_ROUND_BLOCK) { win_m[i] = 0u; win_r[i] = 0u; win_f[i] = NO_MOVE; }
    kasw::sync();
    s.moves = 0; s.reps = 0; s.top = 0; s.by_in = 0; s.by_out = 0;
    int32_t consumed = 0;
    for (int32_t t = 0; t < z.seg_count; ++t) {
      const KasMovesSeg seg = a.segs[z.seg_begin + t];
      if (a.topic_results[seg.topic].status != KAS_OK) continue;  // (uniform: one word every lane reads)
      for (int32_t row_lo = 0; row_lo < seg.rows; row_lo += KAS_MOVES_ITEM_ROWS) {
        const int32_t row_hi = seg.rows - row_lo > KAS_MOVES_ITEM_ROWS ? row_lo + KAS_MOVES_ITEM_ROWS : seg.rows;
        const int32_t g = kasb::load_tile<W, C16>(b, seg, t, row_lo, row_hi, L, l, 0);
        if (g == 0) continue;                                   // (uniform: the tile's counts, read by every lane alike)
        if (wave == 0) walk<W>(capi, capo, shift, N, st, l, s, g);
        kasw::sync();
        for (int32_t e = tid; e < g; e += KAS_ROUND_BLOCK) {
          const int32_t r = l.qtp[2 * e], i = consumed + e;
          uint32_t rep = 0u;
#pragma unroll
          for (int k = 0; k < W; ++k) rep += l.qn[e * 2 * W + k] != NONE ? 1u : 0u;
          const int32_t idx = r - base;
          if (idx >= 0 && idx < KAS_ROUND_WINDOW) {
            kasw::lds_add_u32(win_m + idx, 1u);
            if (rep != 0u) kasw::lds_add_u32(win_r + idx, rep);
            kasw::lds_atomic_min(win_f + idx, i);
          }
          if (base == 0 && (int64_t)i < a.move_stride) a.round_of[(int64_t)j * a.move_stride + i] = r;
        }
        consumed += g;
        kasw::sync();
      }
    }
    if (tid == 0) misc[M_NR] = (uint32_t)s.top;
    kasw::sync();
    const int32_t nr = (int32_t)misc[M_NR];
    int32_t mm = 0, mr = 0;
    for (int32_t idx = tid; idx < KAS_ROUND_WINDOW && base + idx < nr; idx += KAS_ROUND_BLOCK) {
      const int32_t m = (int32_t)win_m[idx], rp = (int32_t)win_r[idx];
      mm = m > mm ? m : mm; mr = rp > mr ? rp : mr;
      if ((int64_t)(base + idx) < a.round_stride) {
        kas_move_round rec;
        rec.n_moves = m; rec.replicas = rp; rec.first_move = win_f[idx]; rec.reserved = 0;
        a.rounds[(int64_t)j * a.round_stride + base + idx] = rec;
      }
    }
    if (mm > 0) kasw::lds_atomic_max(reinterpret_cast<int*>(misc + M_MAXM), mm);
    if (mr > 0) kasw::lds_atomic_max(reinterpret_cast<int*>(misc + M_MAXR), mr);
    kasw::sync();
    if (nr - base <= KAS_ROUND_WINDOW) break;                   // (uniform: one word every lane read between two barriers)
  }
  if (tid == 0) {
    kas_scenario_rounds r;
    r.n_rounds = s.top; r.n_moves = s.moves; r.replicas = s.reps;
    r.max_round_moves = (int32_t)misc[M_MAXM]; r.max_round_replicas = (int32_t)misc[M_MAXR];
    r.raised_by_inbound = s.by_in; r.raised_by_outbound = s.by_out; r.reserved = 0;
    a.scenarios[j] = r;
  }
}

}  // namespace kasr
