// kas_front_body.h — device code of the mark and front rank kernels (launch arguments: kas_front.h).
//
// Written against the kasw:: primitives (kas_wave.h), so that tests/emu/front_driver.cpp steps the same source on CPU fibers.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_choose_body.h"
#include "kas_front.h"
#include "kas_wave.h"

#ifndef KAS_FRONT_MARK_UNROLL
#define KAS_FRONT_MARK_UNROLL 4        // entries of the tile a lane tests per trip of the mark loop (the trips are independent)
#endif

namespace kasf {

// ---- mark ---------------------------------------------------------------------------------------------------------------
// A scenario as the domination test reads it: the criteria in spec order, each biased so that unsigned order is int32 order,
// unused criteria 0 (equal everywhere: they change nothing); the index is the entry's place in the tile.
struct Entry {
  uint32_t c[KAS_CHOOSE_MAX_KEYS];
  int32_t ok;                   // status == KAS_OK
  int32_t eligible;             // ... and every bound holds
  int32_t reserved[2];
};
static_assert(sizeof(Entry) == 32, "an LDS tile entry is two 16-byte reads");

template <class Src>
KAS_DEV Entry entry_of(const KasFrontLaunch& a, int32_t s, const Src& src) {
  const kas_scenario_result r = a.c.sr[s];
  const kas_scenario_impact m = a.c.si[s];
  Entry e;
#pragma unroll
  for (int i = 0; i < KAS_CHOOSE_MAX_KEYS; ++i)
    e.c[i] = i < a.c.n_keys ? (uint32_t)kasc::criterion_of(src, r, m, s, a.c.key[i]) ^ 0x80000000u : 0u;
  e.ok = r.status == KAS_OK ? 1 : 0;
  int32_t within = 1;
#pragma unroll
  for (int i = 0; i < KAS_CHOOSE_MAX_KEYS; ++i)
    if (i < a.n_limits && kasc::criterion_of(src, r, m, s, a.limit_key[i]) > a.limit[i]) within = 0;
  e.eligible = e.ok & within;
  e.reserved[0] = 0; e.reserved[1] = 0;
  return e;
}

// Workgroup `block` of the mark kernel.  tile: KAS_CHOOSE_TILE entries of LDS.  Lane g < S is scenario g.  Src: where the criteria
// come from (kas_choose_body.h).
template <class Src = kasc::Records>
KAS_DEV void mark_block(const KasFrontLaunch& a, int32_t block, Entry* tile, const Src& src = Src()) {
  const int32_t S = a.c.S;
  const int32_t tid = kasw::tid();
  const int32_t g = block * KAS_CHOOSE_BLOCK + tid;
  const bool live = g < S;
  Entry mine;
  mine.c[0] = 0; mine.c[1] = 0; mine.c[2] = 0; mine.c[3] = 0; mine.ok = 0; mine.eligible = 0;
  if (live) mine = entry_of(a, g, src);
  int32_t beaten = 0, n_ok = 0, n_eligible = 0;
  for (int32_t base = 0; base < S; base += KAS_CHOOSE_TILE) {
    const int32_t n = S - base < KAS_CHOOSE_TILE ? S - base : KAS_CHOOSE_TILE;
    kasw::sync();                                               // (every lane has left the tile before)
    for (int32_t i = tid; i < n; i += KAS_CHOOSE_BLOCK) tile[i] = entry_of(a, base + i, src);
    kasw::sync();
#pragma unroll KAS_FRONT_MARK_UNROLL
    for (int32_t i = 0; i < n; ++i) {                           // (every lane reads the same entry: an LDS broadcast)
      const Entry e = tile[i];
      const bool le = e.c[0] <= mine.c[0] && e.c[1] <= mine.c[1] && e.c[2] <= mine.c[2] && e.c[3] <= mine.c[3];
      const bool lt = e.c[0] < mine.c[0] || e.c[1] < mine.c[1] || e.c[2] < mine.c[2] || e.c[3] < mine.c[3];
      beaten |= (e.eligible != 0 && le && (lt || base + i < g)) ? 1 : 0;
      n_ok += e.ok;
      n_eligible += e.eligible;
    }
  }
  if (live) a.cls[g] = !mine.ok ? KAS_FRONT_NOT_OK : !mine.eligible ? KAS_FRONT_OVER_LIMIT : beaten ? KAS_FRONT_DOMINATED : 0;
  if (g == 0) { a.c.n_ok[0] = n_ok; a.counts[0] = n_ok; a.counts[1] = n_eligible; }
}

// ---- front rank ---------------------------------------------------------------------------------------------------------
// The members of the front take part; everybody else keeps its class code as its rank.
struct ByClass {
  const int32_t* cls;
  int32_t* counts;
};
KAS_DEV int32_t takes_part(const ByClass& p, const KasChooseLaunch&, int32_t s, const kas_scenario_result&) { return p.cls[s] == 0 ? 1 : 0; }
KAS_DEV int32_t outside(const ByClass& p, const KasChooseLaunch&, int32_t s) { return p.cls[s]; }
KAS_DEV void count(const ByClass& p, const KasChooseLaunch&, int32_t n) { p.counts[2] = n; p.counts[3] = 0; }

// Workgroup `block` of the front rank kernel: kasc::rank_block's grid and tile.
template <class Src = kasc::Records>
KAS_DEV void rank_block(const KasFrontLaunch& a, int32_t block, kasc::Entry* tile, const Src& src = Src()) {
  kasc::rank_block(a.c, block, tile, ByClass{a.cls, a.counts}, src);
}

}  // namespace kasf
