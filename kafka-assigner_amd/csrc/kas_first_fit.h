// kas_first_fit.h — first fit, P4 (KAS:56, 162-186): the windows over the orphan lists, the per-topic driver around them and
// kas_p4_kernel's scenario.  Included by kas_solver_body.h (after the row helpers, before fill_topic).
//
// Three workgroups run first fit: the fill workgroup (fill_topic), kas_p4_kernel / the second wavefront of kas_p4_order_kernel
// (p4_scenario, below) and kas_spread_p4_kernel (spread_p4).  Each brings loads, racks and the chunks' orphan counts into its LDS in
// its own way; the live list, the windows with the failed row and the verdict are written once here.  first_fit_topic is the three
// in a row: p4_scenario and spread_p4 call it, fill_topic puts them together itself around the general fill's P3 + P4.
#pragma once

namespace kas {

// node positions per hand-over step of the parallel P4.  The step is the chain (window w + 1 takes a
// position group when window w has published it) and its cost grows with the group: lists 5 wide test
// five holder racks per position and at configs[4] nearly every orphan lands on the first or second
// node of the group, so 2 positions (fill 3.4 ms) beat 4 (4.3) and 8 (5.2); at the headline shape
// (lists 3 wide, rack-conflict stragglers walking a list of few nodes) 4 is best (365k against 360k
// scenarios/s at 2 or 8).
#ifndef KAS_P4_U
#define KAS_P4_U 4
#endif
#ifndef KAS_P4_U_WIDE
#define KAS_P4_U_WIDE 1
#endif
// ---------------------------------------------------------------------------------------------
// P4 of the rack-diverse fill (KAS:162-186) on ALL wavefronts of the workgroup.  The orphan rows
// were listed per chunk by pass B; windows of 64 orphans (lane = orphan, ascending row order,
// position-major first fit as in p4_window) go to the waves round-robin.  Window w + 1 may look
// at live-list positions [j, j + U) as soon as window w is done with them (cell (orphan, node
// position) of the reference's double loop depends only on earlier orphans at that position and
// on earlier positions of that orphan), so consecutive windows run one step apart.
// prog[wave] = window << 32 | positions done (monotone; a finished window counts as the start of
// the next one).  A window waits for EVERY earlier window that may still be running (the latest
// window of each other wave; earlier windows of its own wave are finished), not only for its
// predecessor: that one can finish early while an older window still walks the list.  The earliest window that cannot place an orphan decides the failure
// (KAS:183-184): everything before it completed exactly as in the sequential order; later
// windows stop when they see it.  LDS words other waves write are read through a ballot or a
// broadcast, so a wave always acts on one answer.
// ---------------------------------------------------------------------------------------------
// (NC: chunk lists the orphans come in — the fill's wavefronts — where that is not the number of wavefronts running the
// windows: kas_p4_kernel)
// (fin != nullptr — first fit in the order kernel's workgroup, kas_p4_order_kernel, NW == 1: behind every finished window the word
//  gets fin_hi | rows of the topic that are FINAL — every row below the next window's first orphan; the order wavefront of the
//  same workgroup follows it)
template <int W, int NW, int NC = NW>
KAS_DEV void p4_lists_parallel(const LdsView& L, const TopicView& T, int32_t live_count, int32_t wave,
                               int64_t (&st)[8], int32_t& fail_win, int32_t& fail_row, uint64_t* fin = nullptr, uint64_t fin_hi = 0ull) {
  const int lane = kasw::lane();
  uint64_t* prog = (uint64_t*)&L.ctl[KAS_CTL_PROG];
  int32_t oc[NC], total = 0;
#pragma unroll
  for (int w = 0; w < NC; ++w) { oc[w] = L.ctl[KAS_CTL_OC + w]; total += oc[w]; }
  // row index of the g-th orphan of the topic (chunk lists concatenated), or -1 past the end
  auto orphan_row = [&](int32_t g) -> int32_t {
    int32_t w = 0, base = 0;
#pragma unroll
    for (int k = 0; k < NC - 1; ++k) {
      const bool next = w == k && g >= base + oc[k];
      base += next ? oc[k] : 0;
      w += next ? 1 : 0;
    }
    return g < total ? T.orph[((int64_t)chunk_begin<NC>(T.nt, w) << 6) + (g - base)] : -1;
  };
  auto row_cells = [&](int32_t p) -> MidRaw<W> {
    return mid_load_raw<W>(T.mid, T.ow, p >= 0 ? p : 0, p >= 0, T.m32);
  };
  const int32_t n_win = (total + 63) >> 6;
  // Window w may touch live-list positions [j, j + U) once EVERY earlier window is done with them.
  // Waiting for window w - 1 alone is not enough: it may finish early (its orphans all placed on the
  // first nodes) while window w - 2 still walks the list with an orphan whose racks were taken, and
  // window w would then overtake that orphan and take a slot that is not its turn (round 2: one
  // scenario solve in ~70,000 of the bench mix ended with a broker one over its cap).  Windows
  // w - NW and earlier ran on this wave and are finished; lane d (1 <= d < NW) watches the wave that
  // has window w - d.
  const int32_t dw = (lane >= 1 && lane < NW) ? lane : 1;
  const int32_t xw = (wave + NW - dw) % NW;
  const int32_t cap = T.cap, mw = mid_width(T.ow);
  constexpr int U = W >= 4 ? KAS_P4_U_WIDE : KAS_P4_U;      // node positions fetched per LDS round trip
  int32_t p_nxt = orphan_row(64 * wave + lane);
  MidRaw<W> c_nxt = row_cells(p_nxt);
  for (int32_t w = wave; w < n_win; w += NW) {
    const int32_t p = p_nxt;
    int32_t c_cur[W];
    mid_unpack<W>(c_nxt, T.ow, c_cur, T.m32);
    p_nxt = orphan_row(64 * (w + NW) + lane);              // my next window's rows: read ahead
    c_nxt = row_cells(p_nxt);
    kasw::repoll();
    if (kasw::ballot(L.ctl[KAS_CTL_FAILWIN] < w) != 0) break;   // an earlier window failed: so has the topic
    int32_t hc = 0, hr[W];                                  // holders are a prefix of the row
#pragma unroll
    for (int k = 0; k < W; ++k) {
      hr[k] = (p >= 0 && c_cur[k] >= 0) ? (int32_t)lds_rack(L, c_cur[k]) : -1;
      hc += (p >= 0 && c_cur[k] >= 0) ? 1 : 0;
    }
    int32_t need = p >= 0 ? T.rf - hc : 0;
    int32_t j = kasw::shfl(L.ctl[KAS_CTL_HEAD], 0);
    if (lane == 0) prog[wave] = ((uint64_t)(uint32_t)w << 32) | (uint32_t)j;
    KAS_COUNT(st[4]);
    bool stop = false;
    bool placed = false;                                    // (dword mid rows) my row took a broker in this window
    for (;;) {
      uint64_t pend = kasw::ballot(need > 0);
      if (pend == 0) break;
      if (j >= live_count) {                                // KAS:183-184: this orphan cannot be placed
        if (lane == 0) kasw::lds_atomic_min(&L.ctl[KAS_CTL_FAILWIN], w);
        stop = true;
        break;
      }
      // (the nodes of the position group and their racks do not change: read before the wait, so that what
      // follows it — the chain from window to window — is one LDS round trip for the loads)
      int32_t n[U], slots[U], rk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) n[u] = (int32_t)L.live[j + u < live_count ? j + u : j];
#pragma unroll
      for (int u = 0; u < U; ++u) rk[u] = (int32_t)lds_rack(L, n[u]);
      if (w > 0 && NW > 1) {                                // until every earlier window is done with [j, j + U)
        const int32_t upto = j + U < live_count ? j + U : live_count;
        const bool watch = lane >= 1 && lane < NW && w - dw >= 0;
        const uint64_t want = ((uint64_t)(uint32_t)(w - dw) << 32) + (uint32_t)upto;
        bool abandoned = false;
        int32_t idle = 0;
        for (;;) {
          kasw::repoll();
          if (kasw::ballot(watch && prog[xw] < want) == 0) break;
          if (kasw::ballot(L.ctl[KAS_CTL_FAILWIN] < w) != 0) { abandoned = true; break; }
          if (watchdog_poll((uint32_t*)&L.ctl[KAS_CTL_WATCHDOG], false, idle)) {
            if (lane == 0) kasw::lds_atomic_min(&L.ctl[KAS_CTL_FAILWIN], -1);   // every later window stops
            abandoned = true;
            break;
          }
          // (no s_sleep between polls: the hand-over from window to window is the chain of P4, and the
          // poll is one LDS read; in flight 362.4k against 358.2k scenarios/s with the pause in round 3, 634k against
          // 653k in round 5)
        }
        if (abandoned) { stop = true; break; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) slots[u] = cap - lds_load(L, n[u]);
      int32_t taken[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        taken[u] = 0;
        if (j + u < live_count && pend != 0) {             // wave-uniform
          KAS_COUNT(st[5]);
          if (slots[u] > 0) {
            bool want = need > 0;
#pragma unroll
            for (int k = 0; k < W; ++k) want = want && !(k < hc && hr[k] == rk[u]);
            const uint64_t wm = kasw::ballot(want);
            if (wm != 0) {
              const int32_t rank = kasw::count_below(wm);
              if (want && rank < slots[u]) {               // accept (KAS:178-181)
                if (W == 3 && T.m32) {                       // (dword mid rows: the row is stored again, sorted, when its window is through)
                  put<W>(c_cur, hc, n[u]);
                  placed = true;
                } else {
                  T.mid[(int64_t)p * mw + hc] = (uint16_t)n[u];
                }
                put<W>(hr, hc, rk[u]);
                hc += 1;
                need -= 1;
              }
              const int32_t takers = kasw::popc(wm);
              taken[u] = takers < slots[u] ? takers : slots[u];
              pend = kasw::ballot(need > 0);
            }
          }
        }
      }
      if (lane == 0) {
#pragma unroll
        // (only this wave touches these nodes now: the new load follows from the slots read above, no re-read)
        for (int u = 0; u < U; ++u) if (taken[u] > 0) lds_load(L, n[u]) = cap - slots[u] + taken[u];
      }
      kasw::lockstep();
      j += U;
      if (lane == 0) prog[wave] = ((uint64_t)(uint32_t)w << 32) | (uint32_t)(j < live_count ? j : live_count);
    }
    if constexpr (W == 3) {
      if (T.m32 && placed) reinterpret_cast<uint32_t*>(T.mid)[p] = mid32_pack(c_cur[0], c_cur[1], c_cur[2]);
    }
    if (stop) {
      // failed or abandoned: whoever waits on this window must not hang
      if (j >= live_count) {
        const uint64_t left = kasw::ballot(need > 0);
        fail_win = w;
        fail_row = kasw::shfl(p, left != 0 ? kasw::first_lane(left) : 0);
      }
      if (lane == 0) prog[wave] = (uint64_t)(uint32_t)(w + 1) << 32;
      break;
    }
    // done: full nodes at the front of the live list need not be looked at again
    if (lane == 0) {
      int32_t head = L.ctl[KAS_CTL_HEAD];
      while (head < live_count && lds_load(L, (int32_t)L.live[head]) >= cap) ++head;
      kasw::lds_atomic_max(&L.ctl[KAS_CTL_HEAD], head);
      prog[wave] = (uint64_t)(uint32_t)(w + 1) << 32;
    }
    if (fin != nullptr) {                                    // (wave-uniform) this window's mid-row cells are out: publish
      const int32_t nxt0 = kasw::shfl(p_nxt, 0);             // the next window's first orphan (ascending rows), or none
      kasw::wave_sync();                                     // (release: the stores above before the word)
      if (lane == 0) kasw::store_shared_u64_lds(fin, fin_hi | (uint64_t)(uint32_t)(nxt0 >= 0 ? nxt0 : T.P));
    }
  }
}

// ---- the per-topic driver and its pieces ----
// the control words of a topic (every thread of the workgroup calls; a barrier before anything reads them)
KAS_DEV void first_fit_reset_ctl(const LdsView& L, int32_t tid) {
  if (tid < KAS_CTL_INTS) L.ctl[tid] = tid == KAS_CTL_FAILROW ? -1 : (tid == KAS_CTL_FAILWIN ? 0x7fffffff : 0);
}

// KAS:168, 188-200: the non-full nodes in the topic's processing order -> L.live, their number -> KAS_CTL_LIVE and returned (a
// full node can never accept again).  One wavefront; idxN = java_abs_mod(T.hash, T.N), and that it is >= 0 is the caller's check.
KAS_DEV int32_t first_fit_live_list(const LdsView& L, const TopicView& T, int32_t idxN) {
  const int lane = kasw::lane();
  const int32_t N = T.N, cap = T.cap;
  const int32_t start = (N - idxN) % N;        // order[j] = sorted[(j + start) % N]
  int32_t live_count = 0;
  for (int32_t base = 0; base < N; base += 64) {
    const int32_t j = base + lane;
    int32_t n = j + start; if (n >= N) n -= N;
    const bool is_live = j < N && lds_load(L, n) < cap;
    const uint64_t m = kasw::ballot(is_live);
    if (is_live) L.live[live_count + kasw::count_below(m)] = (int16_t)n;
    live_count += kasw::popc(m);
  }
  kasw::lockstep();
  if (lane == 0) L.ctl[KAS_CTL_LIVE] = live_count;
  return live_count;
}

// a wait between the windows ran out (workgroup-uniform; behind a barrier that follows the windows)
KAS_DEV bool first_fit_hung(const LdsView& L) { return KAS_SPIN_BOUND > 0 && L.ctl[KAS_CTL_WATCHDOG] != 0; }

// the verdict (workgroup-uniform; behind a barrier that follows the last write of KAS_CTL_FAILROW): KAS_OK, the watchdog, or the
// first partition that could not be placed (KAS:183-184) under the id the caller of the library knows it by
KAS_DEV TopicOutcome first_fit_outcome(const LdsView& L, const TopicView& T, bool hung) {
  TopicOutcome o;
  o.status = KAS_OK; o.fail_partition = -1; o.moved_replicas = 0; o.moved_partitions = 0;
  const int32_t row = hung ? -1 : L.ctl[KAS_CTL_FAILROW];
  if (hung) o.status = KAS_FAIL_WATCHDOG;
  else if (row >= 0) {
    o.status = KAS_FAIL_UNASSIGNABLE;
    o.fail_partition = T.pid_arr ? T.pid_arr[row] : row;
  }
  return o;
}

// The windows of one topic on the NW wavefronts of the workgroup, and the row of the earliest window that failed into
// KAS_CTL_FAILROW (every thread calls, behind a barrier that follows the live list; a barrier before the verdict is read).
// FS (first fit as ONE wavefront beside the order wavefront, kas_p4_order_kernel: NW == 1, whatever the wavefront's index in its
// workgroup): the barriers are wavefront barriers, and `fin` starts with fin_hi | rows below the topic's first orphan — those are
// final before any window runs — and goes on as p4_lists_parallel says.
template <int W, int NW, int NC = NW, bool FS = false>
KAS_DEV void first_fit_windows(const LdsView& L, const TopicView& T, int32_t wave, int64_t (&st)[8], uint64_t* fin = nullptr, uint64_t fin_hi = 0ull) {
  const int lane = kasw::lane();
  if constexpr (FS) {
    int32_t total_o = 0;
#pragma unroll
    for (int w = 0; w < NC; ++w) total_o += L.ctl[KAS_CTL_OC + w];
    int32_t first = T.P;
    if (total_o > 0) {
      int32_t w0 = 0;
      while (w0 < NC - 1 && L.ctl[KAS_CTL_OC + w0] == 0) ++w0;
      first = T.orph[(int64_t)chunk_begin<NC>(T.nt, w0) << 6];
    }
    if (lane == 0) kasw::store_shared_u64_lds(fin, fin_hi | (uint64_t)(uint32_t)first);
  }
  int32_t fail_win = -1, fail_row = -1;
  p4_lists_parallel<W, NW, NC>(L, T, L.ctl[KAS_CTL_LIVE], wave, st, fail_win, fail_row, fin, fin_hi);
  if constexpr (FS) kasw::wave_sync(); else kasw::sync();    // KAS_CTL_FAILWIN is final: its wave reports the row
  if (fail_win >= 0 && fail_win == L.ctl[KAS_CTL_FAILWIN] && lane == 0) L.ctl[KAS_CTL_FAILROW] = fail_row;
}

// First fit of one topic (every thread calls): live list, windows, verdict.  In the LDS on entry: load[] and rack[] of the nodes, the
// control words reset, the NC chunks' orphan counts in KAS_CTL_OC (the first barrier is in here).  Movement counts are the caller's.
template <int W, int NW, int NC = NW, bool FS = false>
KAS_DEV TopicOutcome first_fit_topic(const LdsView& L, const TopicView& T, int64_t (&st)[8], uint64_t* fin = nullptr, uint64_t fin_hi = 0ull) {
  static_assert(!FS || NW == 1, "first fit inside the order kernel's workgroup is one wavefront");
  const int32_t wave = FS ? 0 : kasw::wave_id();
  auto barrier = [&]() { if constexpr (FS) kasw::wave_sync(); else kasw::sync(); };
  if (wave == 0) first_fit_live_list(L, T, java_abs_mod(T.hash, T.N));
  barrier();
  first_fit_windows<W, NW, NC, FS>(L, T, wave, st, fin, fin_hi);
  barrier();
  return first_fit_outcome(L, T, first_fit_hung(L));
}

// ---------------------------------------------------------------------------------------------
// kas_p4_kernel, one scenario (KAS_FLAG_SPLIT_P4): first fit of the topics the fill kernel handed over (KasLaunch::p4s), in order, on
// PW wavefronts.  A partition that cannot be placed fails its topic (KAS:183-184), the topics behind it are skipped (KAG:173-184
// aborted) and emit nothing, and the scenario's record says so — what fill_scenario does when first fit runs inside it.
// ---------------------------------------------------------------------------------------------
// FS (kas_p4_order_kernel: first fit as ONE wavefront of the order kernel's workgroup, whatever its index there): the workgroup
// barriers become wavefront barriers, and fs[] carries what the order wavefront follows —
//   fs[0]  topic << 32 | rows of that topic that are final (first fit done with them; a topic that needs none: all its rows)
//   fs[1]  the topic first fit failed at (KAS:183-184), or 0x7fffffff;  fs[2]  the order wavefront's answer: it has stopped writing
// — and a failed topic's padding waits for that answer (the order wavefront may have emitted rows of it already).
// (M32C: the mid-row layout as a compile-time constant, as in fill_topic — 1: dword mid rows, 0: 16-bit rows, -1: the launch's flags)
template <int W, int PW, bool FS = false, int M32C = -1>
KAS_DEV void p4_scenario(const KasLaunch& a, int32_t s, unsigned char* lds_raw, uint64_t* fs = nullptr) {
  constexpr int NW = PW, NT = 64 * NW, NC = KAS_P4_WAVES;    // PW wavefronts run the windows over the fill's NC chunk lists
  const int lane = kasw::lane();
  const int tid = FS ? lane : kasw::tid();
  auto barrier = [&]() { if constexpr (FS) kasw::wave_sync(); else kasw::sync(); };
  const kas_scenario_desc sd = a.scen[s];
  const int32_t N = sd.n_nodes;
  // (a scenario the fill kernel failed at topic k2 still has its rack-diverse topics before k2 waiting for their first fit)
  const KasP4Lds lay = kas_p4_lds_layout(a.n_max);
  LdsView L;
  L.x = nullptr; L.qrs = nullptr; L.idmap = nullptr; L.ids = nullptr; L.ring_p = nullptr; L.ring_meta = nullptr; L.ring_rack = nullptr;
  L.load = (int32_t*)(lds_raw + lay.off_load);
  L.rack = (int16_t*)(lds_raw + lay.off_rack);
  L.live = (int16_t*)(lds_raw + lay.off_live);
  L.ctl = (int32_t*)(lds_raw + lay.off_ctl);
  L.ns = 1; L.rs = 1;
  const int32_t* g_node_rack = a.node_rack + sd.node_off;
  const int64_t t_begin = kasw::clock_ticks();
  int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t* orph = a.orph + a.orph_off[s];
  bool failed = false;
  int32_t moved_r = 0, moved_p = 0;                          // (over the topics before a failure)
  for (int32_t k = 0; k < sd.topic_count; ++k) {
    const int32_t ti = sd.topic_begin + k;
    const kas_topic_desc td = a.topics[ti];
    int32_t* const orph_topic = orph;
    orph += (int64_t)((td.n_partitions > 0 ? td.n_partitions : 0) + 63) / 64 * 64;
    if (failed) {                                            // KAG:173-184 aborted: nothing is returned for this topic
      // (FS: the order wavefront skips every topic behind fs[1] and never writes there)
      out_pad(topic_out(a, td), (int64_t)td.n_partitions * td.out_width, tid, NT);
      TopicOutcome o;
      o.status = KAS_SKIPPED; o.fail_partition = -1; o.moved_replicas = 0; o.moved_partitions = 0;
      if (tid == 0) put_topic_result(a, ti, o);
      continue;
    }
    const kas_topic_result tr0 = a.topic_results[ti];
    moved_r += tr0.moved_replicas; moved_p += tr0.moved_partitions;
    const int32_t* p4s = a.p4s + (int64_t)ti * (KAS_P4S_HEAD + a.n_max);
    if (tr0.status != KAS_OK || p4s[0] == 0) {               // (workgroup-uniform: nothing handed over)
      if constexpr (FS) {                                    // every row of the topic is final as the fill kernel left it
        if (lane == 0) kasw::store_shared_u64_lds(&fs[0], ((uint64_t)(uint32_t)k << 32) | (uint64_t)(uint32_t)(td.n_partitions > 0 ? td.n_partitions : 0));
      }
      continue;
    }
    TopicView T = topic_view(a, td, N, M32C);                // (cur / len_arr / inp_arr come along unused: first fit reads mid rows)
    T.orph = orph_topic;
    T.cap = p4s[1];
    barrier();                                            // (the previous topic's node state has been read)
    for (int32_t i = tid; i < N; i += NT) { L.load[i] = p4s[KAS_P4S_HEAD + i]; L.rack[i] = (int16_t)g_node_rack[i]; }
    first_fit_reset_ctl(L, tid);
    barrier();
    if (tid < NC) L.ctl[KAS_CTL_OC + tid] = p4s[2 + tid];
    // (the rotation of KAS:190 is valid: the fill kernel checked)
    TopicOutcome o = first_fit_topic<W, NW, NC, FS>(L, T, st, FS ? &fs[0] : nullptr, (uint64_t)(uint32_t)k << 32);
    if (o.status != KAS_OK) {                                // (workgroup-uniform)
      failed = true;
      moved_r -= tr0.moved_replicas; moved_p -= tr0.moved_partitions;
      if constexpr (FS) {
        // the order wavefront may have emitted rows of this topic: it stops when it sees fs[1], says so in fs[2], and only
        // then is the topic padded (bounded like every wait between wavefronts: kas_solver_body.h, "Hang containment")
        if (lane == 0) kasw::store_shared_u64_lds(&fs[1], (uint64_t)(uint32_t)k);
        int32_t idle = 0;
        for (;;) {
          kasw::repoll();
          if (kasw::ballot(kasw::load_shared_u64_lds(&fs[2]) != 0ull) != 0ull) break;
          if (watchdog_poll(reinterpret_cast<uint32_t*>(&fs[3]), false, idle)) break;
        }
      }
      out_pad(topic_out(a, td), (int64_t)td.n_partitions * td.out_width, tid, NT);   // nothing is returned for a failed topic
      if (tid == 0) {
        put_topic_result(a, ti, o);
        put_scenario_result(a, s, o.status, k, o.fail_partition, moved_r, moved_p);
      }
    }
  }
  if constexpr (FS) {
    kasw::wave_sync();                                       // (the records above before the word)
    if (lane == 0) kasw::store_shared_u64_lds(&fs[0], (uint64_t)(uint32_t)sd.topic_count << 32);
  }
  if (tid == 0 && a.stats) a.stats[(int64_t)s * KAS_STATS_PER_SCENARIO + 3] += kasw::clock_ticks() - t_begin;
}

}  // namespace kas
