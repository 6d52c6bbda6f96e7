// kas_batches_body.h — device code of the batches pass (launch arguments and LDS layout: kas_batches.h).
//
// One workgroup of KAS_BATCH_BLOCK lanes per listed scenario.  It stages the scenario's id -> node lookup in the LDS as the
// impact pass does (kasi::Lookup / node_of: a direct int16 table where the id range fits the lookup words, else the sorted ids),
// zeroes two counters per node (in[N], out[N]) and walks the scenario's rows tile by tile, a moves-pass item of
// KAS_MOVES_ITEM_ROWS rows a tile:
//   load     rows as the moves count kernel loads them (consecutive lanes on consecutive rows, four rows a lane, a row's cells
//            in registers); a row with the KAS_MOVE_REPLICAS flag becomes a queue entry: its In and Out node indices as
//            uint16, its (topic, partition).  Positions come from ballots and the sixteen (u, wavefront) counts: row order.
//   consume  groups of KAS_BATCH_GROUP moves, one per lane, optimistically: every lane adds its move to the counters with
//            no-return adds, the lanes synchronise and read their nodes' counters back.  Counts only grow within a batch, so
//            if no counter read back exceeds its cap and the batch stays within max_moves, every prefix of the group fits too:
//            the whole group is in.  Otherwise the lanes take their adds back and wavefront 0 replays the group one move at
//            a time — exactly the loop of include/kas_abi.h; its lanes hold the cells of the one move, ballots name the reason.
//   close    wavefront 0 reads every counter once — the batch's maxima — and zeroes it; lane 0 stores the record.
// What is left of the queue (fewer moves than a group) waits for the next tile; the scenario's last group is a short one.
//
// No position and no decision comes from the return value of an atomic; the sums do not depend on the order of the adds and
// the replay is one wavefront's program order, so the same inputs give the same bytes.  Every sync() is in workgroup-uniform
// control flow: "did the group fit" is read by every lane from one LDS word between two barriers.
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/batches_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_batches.h"
#include "kas_impact_body.h"   // kasi::cell, kasi::Lookup, kasi::node_of
#include "kas_wave.h"

namespace kasb {

constexpr int WAVES = KAS_BATCH_BLOCK / 64;
constexpr int U = KAS_MOVES_ROWS_PER_LANE;
constexpr int GROUPS = U * WAVES;          // (u, wavefront) groups of a tile, in row order
constexpr uint32_t NONE = KAS_BATCH_NODE_NONE;

// words of the misc region
enum { M_FLAG0 = 0, M_FLAG1 = 1, M_BN = 2, M_MAXIN = 3, M_MAXOUT = 4, M_REP = 8 /* [WAVES] */, M_SUB = 16 /* [GROUPS] */, M_WORDS = 32 };
static_assert(4 * M_WORDS <= KAS_BATCH_MISC_BYTES && M_REP + WAVES <= M_SUB && M_SUB + GROUPS <= M_WORDS, "the misc words fit their region");

// the batch being filled and the scenario's sums: wavefront 0 holds them, every lane of it alike
struct State {
  int32_t first, n, rep, topic, part;      // the open batch (n == 0: none)
  int32_t nb, moves, reps, max_moves, max_reps, by_moves, by_in, by_out;   // the scenario's sums
};

template <int W>
struct Lds {
  uint32_t* ctr;          // in[n_cap] then out[n_cap]
  uint32_t* misc;
  uint16_t* qn;           // [KAS_BATCH_QUEUE][2 * W]: In nodes, Out nodes (NONE: no node)
  int32_t* qtp;           // [KAS_BATCH_QUEUE][2]: topic, partition
};

// Wavefront 0, all 64 lanes: read and zero the 2 * N counters; with a batch open, emit its record.
KAS_DEV void close_batch(const KasBatchesLaunch& a, int32_t j, int32_t N, uint32_t* ctr, uint32_t* misc, State& s, int32_t why) {
  const int32_t lane = kasw::lane();
  int32_t mi = 0, mo = 0;
  for (int32_t i = lane; i < N; i += 64) {
    const int32_t vi = (int32_t)ctr[i], vo = (int32_t)ctr[N + i];
    mi = vi > mi ? vi : mi; mo = vo > mo ? vo : mo;
    ctr[i] = 0u; ctr[N + i] = 0u;
  }
  if (lane == 0) { misc[M_MAXIN] = 0u; misc[M_MAXOUT] = 0u; }
  kasw::lockstep();
  if (mi > 0) kasw::lds_atomic_max(reinterpret_cast<int*>(misc + M_MAXIN), mi);
  if (mo > 0) kasw::lds_atomic_max(reinterpret_cast<int*>(misc + M_MAXOUT), mo);
  kasw::lockstep();
  if (s.n > 0) {
    if (lane == 0 && (int64_t)s.nb < a.stride) {
      kas_move_batch r;
      r.first_move = s.first; r.n_moves = s.n; r.topic = s.topic; r.partition = s.part; r.replicas = s.rep;
      r.max_inbound = (int32_t)misc[M_MAXIN]; r.max_outbound = (int32_t)misc[M_MAXOUT]; r.closed_by = why;
      a.batches[(int64_t)j * a.stride + s.nb] = r;
    }
    s.nb += 1; s.moves += s.n; s.reps += s.rep;
    s.max_moves = s.n > s.max_moves ? s.n : s.max_moves;
    s.max_reps = s.rep > s.max_reps ? s.rep : s.max_reps;
    s.by_moves += why == KAS_BATCH_MAX_MOVES ? 1 : 0;
    s.by_in += why == KAS_BATCH_INBOUND ? 1 : 0;
    s.by_out += why == KAS_BATCH_OUTBOUND ? 1 : 0;
  }
  s.n = 0; s.rep = 0;
  kasw::lockstep();
}

// Wavefront 0: moves [head, head + g) of the queue, one at a time.  Lane k < W holds In cell k, lane W + k Out cell k.
template <int W>
KAS_DEV void replay(const KasBatchesLaunch& a, int32_t j, int32_t N, const Lds<W>& l, State& s, int32_t head, int32_t g, int32_t base) {
  const int32_t lane = kasw::lane();
  const uint32_t capi = (uint32_t)a.spec.cap_inbound, capo = (uint32_t)a.spec.cap_outbound;
  const bool has = lane < 2 * W;
  uint32_t node = (has && g > 0) ? (uint32_t)l.qn[head * 2 * W + lane] : NONE;
  for (int32_t m = 0; m < g; ++m) {
    const int32_t e = head + m;
    // (the next move's cell is asked for before this move's counter: one LDS round trip a move, not two)
    const uint32_t next = (has && m + 1 < g) ? (uint32_t)l.qn[(e + 1) * 2 * W + lane] : NONE;
    const bool named = node != NONE;
    const bool inb = lane < W;
    uint32_t* const word = l.ctr + (inb ? 0 : N) + (named ? (int32_t)node : 0);
    const uint32_t cnt = named ? *word : 0u;
    const uint64_t hit_in = kasw::ballot(named && inb && capi != 0u && cnt >= capi);
    const uint64_t hit_out = kasw::ballot(named && !inb && capo != 0u && cnt >= capo);
    const int32_t why = (a.spec.max_moves != 0 && s.n == a.spec.max_moves) ? KAS_BATCH_MAX_MOVES
                        : (hit_in != 0ull ? KAS_BATCH_INBOUND : (hit_out != 0ull ? KAS_BATCH_OUTBOUND : 0));
    if (why != 0) close_batch(a, j, N, l.ctr, l.misc, s, why);
    if (s.n == 0) { s.first = base + m; s.topic = l.qtp[2 * e]; s.part = l.qtp[2 * e + 1]; }
    s.n += 1;
    s.rep += kasw::popc(kasw::ballot(named && inb));
    if (named) kasw::lds_add_u32(word, 1u);
    kasw::lockstep();
    node = next;
  }
}

// One group: moves [head, head + g) of the queue, g <= KAS_BATCH_GROUP.  Every lane of the workgroup calls it; `parity`
// alternates from group to group (the flag word a slow wavefront still reads is not the one the next group clears).
template <int W>
KAS_DEV void consume(const KasBatchesLaunch& a, int32_t j, int32_t N, const Lds<W>& l, State& s, int32_t head, int32_t g, int32_t base,
                     int32_t parity) {
  const int32_t tid = kasw::tid(), wave = kasw::wave_id();
  const bool mine = tid < g;
  uint32_t* const flag = l.misc + (parity ? M_FLAG1 : M_FLAG0);
  uint32_t in_n[W], out_n[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    in_n[k] = mine ? (uint32_t)l.qn[(head + tid) * 2 * W + k] : NONE;
    out_n[k] = mine ? (uint32_t)l.qn[(head + tid) * 2 * W + W + k] : NONE;
  }
  if (tid == 0) { *flag = 0u; l.misc[M_BN] = (uint32_t)s.n; }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (in_n[k] != NONE) kasw::lds_add_u32(l.ctr + in_n[k], 1u);
    if (out_n[k] != NONE) kasw::lds_add_u32(l.ctr + N + out_n[k], 1u);
  }
  kasw::sync();
  const uint32_t capi = (uint32_t)a.spec.cap_inbound, capo = (uint32_t)a.spec.cap_outbound;
  const int32_t open_n = (int32_t)l.misc[M_BN];
  bool over = false;
  int32_t rep = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (in_n[k] != NONE) { rep += 1; over = over || (capi != 0u && l.ctr[in_n[k]] > capi); }
    if (out_n[k] != NONE) over = over || (capo != 0u && l.ctr[N + out_n[k]] > capo);
  }
  const uint64_t any_over = kasw::ballot(over);
  rep = kasw::wave_sum(rep);
  if (kasw::lane() == 0) {
    if (any_over != 0ull) kasw::store_shared_u32(flag, 1u);
    l.misc[M_REP + wave] = (uint32_t)rep;
  }
  kasw::sync();
  const bool fits = kasw::load_shared_u32(flag) == 0u && !(a.spec.max_moves != 0 && open_n + g > a.spec.max_moves);
  if (fits) {                                                   // (the same for every lane: one word, read between two barriers)
    if (wave == 0) {
      if (s.n == 0) { s.first = base; s.topic = l.qtp[2 * head]; s.part = l.qtp[2 * head + 1]; }
      s.n += g;
      for (int w = 0; w < WAVES; ++w) s.rep += (int32_t)l.misc[M_REP + w];
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (in_n[k] != NONE) kasw::lds_sub_u32(l.ctr + in_n[k], 1u);
    if (out_n[k] != NONE) kasw::lds_sub_u32(l.ctr + N + out_n[k], 1u);
  }
  kasw::sync();
  if (wave == 0) replay<W>(a, j, N, l, s, head, g, base);
  kasw::sync();
}

// One tile: rows [row_lo, row_hi) of segment g.  Appends the tile's REPLICAS moves to the queue behind its `qcount` entries,
// in row order; returns how many.  Every lane of the workgroup calls it.
template <int W, bool C16>
KAS_DEV int32_t load_tile(const KasBatchesLaunch& a, const KasMovesSeg& g, int32_t topic_rel, int32_t row_lo, int32_t row_hi,
                          const kasi::Lookup& L, const Lds<W>& l, int32_t qcount) {
  const int32_t tid = kasw::tid(), wave = kasw::wave_id();
  const int32_t cw = g.cur_width < W ? g.cur_width : W, ow = g.out_width < W ? g.out_width : W;
  const int32_t* lens = g.cur_len_off >= 0 ? a.aux + g.cur_len_off : nullptr;
  const int32_t* part = g.part_id_off >= 0 ? a.aux + g.part_id_off : nullptr;
  const int32_t* cur = reinterpret_cast<const int32_t*>(a.cur);
  const int32_t* out = reinterpret_cast<const int32_t*>(a.out);
  uint32_t packed[U][W];                    // In node k | Out node k << 16
  bool mv[U];
  int32_t rank[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int32_t p = row_lo + u * KAS_BATCH_BLOCK + tid;
    const bool live = p < row_hi;
    int32_t c[W], o[W];
    const int32_t cl = live ? (lens ? lens[p] : cw) : 0;
    const int32_t clen = cl < 0 ? 0 : (cl > cw ? cw : cl);
    const int64_t crow = g.cur_off + (int64_t)p * g.cur_width, orow = g.out_off + (int64_t)p * g.out_width;
#pragma unroll
    for (int k = 0; k < W; ++k) c[k] = (live && k < cw) ? kasi::cell<C16>(cur, crow + k) : -1;
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = (live && k < ow) ? kasi::cell<C16>(out, orow + k) : -1;
    int32_t olen = 0;
    bool open = true;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      open = open && k < ow && o[k] != -1;                      // (the pad: -1, KAS_CELL16_NONE)
      olen += open ? 1 : 0;
    }
    // gained / lost cells as the moves pass counts them (the flag), In / Out as sets of NODES: a cell that repeats an
    // earlier one of its list adds nothing
    bool gained[W], lost[W], any = false;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      bool in_c = false, in_o = false, dup_o = false, dup_c = false;
#pragma unroll
      for (int q = 0; q < W; ++q) {
        in_c = in_c || (q < clen && c[q] == o[k]);
        in_o = in_o || (q < olen && o[q] == c[k]);
        dup_o = dup_o || (q < k && o[q] == o[k]);
        dup_c = dup_c || (q < k && c[q] == c[k]);
      }
      any = any || (k < olen && !in_c) || (k < clen && !in_o);
      gained[k] = k < olen && !in_c && !dup_o;
      lost[k] = k < clen && !in_o && !dup_c;
    }
    mv[u] = olen > 0 && any;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      uint32_t ni = NONE, no = NONE;
      if (mv[u] && gained[k]) { const int32_t n = kasi::node_of<C16>(L, o[k]); ni = n >= 0 ? (uint32_t)n : NONE; }
      if (mv[u] && lost[k]) { const int32_t n = kasi::node_of<C16>(L, c[k]); no = n >= 0 ? (uint32_t)n : NONE; }
      packed[u][k] = ni | (no << 16);
    }
    const uint64_t m = kasw::ballot(mv[u]);
    rank[u] = kasw::count_below(m);
    if (kasw::lane() == 0) l.misc[M_SUB + u * WAVES + wave] = (uint32_t)kasw::popc(m);
  }
  kasw::sync();
  int32_t total = 0;                        // moves of the (u, wavefront) groups so far: before this lane's, then of the tile
#pragma unroll
  for (int u = 0; u < U; ++u) {
    for (int w = 0; w < WAVES; ++w) {
      const int32_t cnt = (int32_t)l.misc[M_SUB + u * WAVES + w];
      if (w == wave && mv[u]) {
        const int32_t e = qcount + total + rank[u];
        const int32_t p = row_lo + u * KAS_BATCH_BLOCK + tid;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          l.qn[e * 2 * W + k] = (uint16_t)(packed[u][k] & 0xffffu);
          l.qn[e * 2 * W + W + k] = (uint16_t)(packed[u][k] >> 16);
        }
        l.qtp[2 * e] = topic_rel;
        l.qtp[2 * e + 1] = part ? part[p] : p;
      }
      total += cnt;
    }
  }
  kasw::sync();
  return total;
}

// Kernel body: workgroup j = listed scenario j.
template <int W, bool C16>
KAS_DEV void batches_scenario(const KasBatchesLaunch& a, int32_t j, unsigned char* lds) {
  const int32_t tid = kasw::tid(), wave = kasw::wave_id();
  const int32_t sidx = a.select[j];
  if (sidx < 0 || sidx >= a.S) {                                // an empty slot: zeros (the same for every lane)
    if (tid == 0) { kas_scenario_batches r = {0, 0, 0, 0, 0, 0, 0, 0}; a.scenarios[j] = r; }
    return;
  }
  const KasMovesScen z = a.scen[sidx];
  const kas_scenario_desc sd = a.sdesc[sidx];
  const int32_t N = sd.n_nodes > 0 ? (sd.n_nodes < a.n_cap ? sd.n_nodes : a.n_cap) : 0;
  Lds<W> l;
  l.ctr = reinterpret_cast<uint32_t*>(lds);
  l.misc = reinterpret_cast<uint32_t*>(lds + a.lds.off_misc);
  l.qn = reinterpret_cast<uint16_t*>(lds + a.lds.off_qn);
  l.qtp = reinterpret_cast<int32_t*>(lds + a.lds.off_qtp);
  for (int32_t i = tid; i < 2 * N; i += KAS_BATCH_BLOCK) l.ctr[i] = 0u;
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
        for (int32_t i = tid; i < (int32_t)range; i += KAS_BATCH_BLOCK) map[i] = -1;
        kasw::sync();
        for (int32_t i = tid; i < N; i += KAS_BATCH_BLOCK) {
          const int64_t d = (int64_t)g_id[i] - lo_id;
          if (d >= 0 && d < range) map[d] = (int16_t)i;
        }
        L.min_id = (int32_t)lo_id; L.range = (uint32_t)range;
      } else {
        int32_t* ids = reinterpret_cast<int32_t*>(lds + a.lds.off_look);
        for (int32_t i = tid; i < N; i += KAS_BATCH_BLOCK) ids[i] = g_id[i];
      }
    }
  }
  kasw::sync();
  State s;
  s.first = 0; s.n = 0; s.rep = 0; s.topic = 0; s.part = 0;
  s.nb = 0; s.moves = 0; s.reps = 0; s.max_moves = 0; s.max_reps = 0;
  s.by_moves = 0; s.by_in = 0; s.by_out = 0;
  int32_t qcount = 0, consumed = 0, parity = 0;
  for (int32_t t = 0; t < z.seg_count; ++t) {
    const KasMovesSeg g = a.segs[z.seg_begin + t];
    if (a.topic_results[g.topic].status != KAS_OK) continue;    // (uniform: one word every lane reads)
    for (int32_t row_lo = 0; row_lo < g.rows; row_lo += KAS_MOVES_ITEM_ROWS) {
      const int32_t row_hi = g.rows - row_lo > KAS_MOVES_ITEM_ROWS ? row_lo + KAS_MOVES_ITEM_ROWS : g.rows;
      qcount += load_tile<W, C16>(a, g, t, row_lo, row_hi, L, l, qcount);
      int32_t head = 0;
      while (qcount - head >= KAS_BATCH_GROUP) {
        consume<W>(a, j, N, l, s, head, KAS_BATCH_GROUP, consumed, parity);
        head += KAS_BATCH_GROUP; consumed += KAS_BATCH_GROUP; parity ^= 1;
      }
      if (head > 0) {                                           // what is left (fewer than a group) moves to the front
        const int32_t left = qcount - head;
        uint16_t n16[2 * W];
        int32_t tp0 = 0, tp1 = 0;
        kasw::sync();
        if (tid < left) {
#pragma unroll
          for (int k = 0; k < 2 * W; ++k) n16[k] = l.qn[(head + tid) * 2 * W + k];
          tp0 = l.qtp[2 * (head + tid)]; tp1 = l.qtp[2 * (head + tid) + 1];
        }
        kasw::sync();
        if (tid < left) {
#pragma unroll
          for (int k = 0; k < 2 * W; ++k) l.qn[tid * 2 * W + k] = n16[k];
          l.qtp[2 * tid] = tp0; l.qtp[2 * tid + 1] = tp1;
        }
        kasw::sync();
        qcount = left;
      }
    }
  }
  if (qcount > 0) { consume<W>(a, j, N, l, s, 0, qcount, consumed, parity); consumed += qcount; }
  kasw::sync();
  if (wave == 0) {
    if (s.n > 0) close_batch(a, j, N, l.ctr, l.misc, s, KAS_BATCH_END_OF_LIST);
    if (tid == 0) {
      kas_scenario_batches r;
      r.n_batches = s.nb; r.n_moves = s.moves; r.replicas = s.reps;
      r.max_batch_moves = s.max_moves; r.max_batch_replicas = s.max_reps;
      r.closed_by_max_moves = s.by_moves; r.closed_by_inbound = s.by_in;
      r.closed_by_outbound = s.by_out;
      a.scenarios[j] = r;
    }
  }
}

}  // namespace kasb
