// kas_choose.h — choosing the best scenarios on the device (include/kas_abi.h: kas_choose_spec / kas_choice): launch arguments,
// the host-built size and segment tables and the launchers the kernels' translation unit (kas_choose.hip) exports to kas_hip.hip.
//
// Pure C++ (no HIP calls), so that the same tables are built in the library and in the CPU emulation under tests/emu/.
//
// Two kernels behind a solve and its impact pass (the rank kernel in three instances: the second also reads the scenario rack
// records of a rack pass, for the rack criteria of KAS_KEY_RACK_BASE, the third those and the scenario topic records of a topic
// pass, for the topic criteria of KAS_KEY_TOPIC_BASE):
//   rank    one lane per scenario, KAS_CHOOSE_BLOCK lanes a workgroup.  Every workgroup streams all S keys through the LDS in
//           tiles of KAS_CHOOSE_TILE entries, built from the 64 bytes of records per scenario; a lane counts the entries whose
//           key is smaller than its own — its rank — and in the same loop sums their packed cells and node counts: the offsets
//           of its rows and of its node block in the packed outputs.  Exact, no atomics, nothing between workgroups.
//   gather  one workgroup per (chosen j, chunk of KAS_CHOOSE_CHUNK bytes of scenario chosen[j]'s packed rows, then of its node
//           block): it walks the scenario's segments (one per topic) and copies bytes with the widest aligned accesses source
//           and destination allow.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "kas_abi.h"

#define KAS_CHOOSE_BLOCK 256           // lanes of a workgroup of either kernel
#define KAS_CHOOSE_TILE 1024           // key entries of an LDS tile (32 bytes each)
#define KAS_CHOOSE_CHUNK 16384         // bytes of packed output a gather workgroup copies

// per scenario: what the rank kernel sums and where the gather kernel finds the scenario's pieces
struct KasChooseSize {
  int64_t cells;                // its topics' out rows, packed: sum of P x out_width
  int64_t node_base;            // first record of its block in the impact pass's node table
  int32_t n_nodes;
  int32_t seg_begin, seg_count; // its segments in the segment table: one per topic, in descriptor order
  int32_t reserved;
};

// one topic's rows
struct KasChooseSeg {
  int64_t out_off;              // cells into the out pool, as the device sees it (the descriptor's offset)
  int64_t cells;
  int64_t packed_at;            // cells of the scenario's earlier topics
  int64_t reserved;
};

// Kernel arguments of both kernels: device pointers (host pointers in the emulator).
struct KasChooseLaunch {
  const kas_scenario_result* sr;        // [S]
  const kas_scenario_impact* si;        // [S]
  const KasChooseSize* sizes;           // [S]; NULL: rank only (no offsets)
  const KasChooseSeg* segs;
  int32_t S, n_keys, key[KAS_CHOOSE_MAX_KEYS], k;
  int32_t* rank;                        // [S]
  int32_t* chosen;                      // [k]
  int64_t* row_off;                     // [k + 1] (with sizes)
  int64_t* node_off;                    // [k + 1] (with sizes)
  int32_t* n_ok;
  // gather
  const void* out;                      // the out pool the solve wrote
  const kas_node_impact* src_nodes;     // the impact pass's node table
  void* rows;                           // packed rows of the chosen
  kas_node_impact* nodes;               // packed node blocks of the chosen
  int32_t src_cell, dst_cell;           // bytes of a cell: 4 / 4, 2 / 2, or 4 / 2 (an int32 solve of a 16-bit call: narrowed on the way)
  int32_t chunks;                       // gather workgroups per chosen scenario
};

#if defined(__HIPCC__)
#define KAS_CHOOSE_FN static inline __host__ __device__   // (also called by the gather kernel)
#else
#define KAS_CHOOSE_FN static inline
#endif
KAS_CHOOSE_FN int64_t kas_choose_chunks_of(int64_t bytes) { return (bytes + KAS_CHOOSE_CHUNK - 1) / KAS_CHOOSE_CHUNK; }

// The size and segment tables of a batch, and what a choice of k scenarios may need at most.
struct KasChoosePlan {
  std::vector<KasChooseSize> sizes;     // [S]
  std::vector<KasChooseSeg> segs;
  int64_t max_cells = 0;                // the largest scenario's packed rows
  int32_t max_nodes = 0;
};

static inline void kas_choose_plan_build(const kas_batch_desc* b, KasChoosePlan* cp) {
  const int32_t S = b->n_scenarios > 0 ? b->n_scenarios : 0;
  cp->sizes.assign((size_t)S, KasChooseSize{});
  cp->segs.clear();
  cp->max_cells = 0; cp->max_nodes = 0;
  int64_t node_base = 0;
  for (int32_t s = 0; s < S; ++s) {
    const kas_scenario_desc& sd = b->scenarios[s];
    KasChooseSize& z = cp->sizes[(size_t)s];
    z.node_base = node_base;
    z.n_nodes = sd.n_nodes > 0 ? sd.n_nodes : 0;
    node_base += z.n_nodes;
    z.seg_begin = (int32_t)cp->segs.size();
    for (int32_t t = 0; t < sd.topic_count; ++t) {
      const kas_topic_desc& td = b->topics[sd.topic_begin + t];
      const int64_t cells = (int64_t)(td.n_partitions > 0 ? td.n_partitions : 0) * (td.out_width > 0 ? td.out_width : 0);
      cp->segs.push_back(KasChooseSeg{td.out_off, cells, z.cells, 0});
      z.cells += cells;
    }
    z.seg_count = (int32_t)cp->segs.size() - z.seg_begin;
    if (z.cells > cp->max_cells) cp->max_cells = z.cells;
    if (z.n_nodes > cp->max_nodes) cp->max_nodes = z.n_nodes;
  }
}

// What the k largest scenarios need: the capacity a caller must offer for a choice of k (any k scenarios may win).
static inline void kas_choose_k_largest(const KasChoosePlan& cp, int32_t k, int64_t* cells, int64_t* nodes) {
  std::vector<int64_t> c, n;
  for (const KasChooseSize& z : cp.sizes) { c.push_back(z.cells); n.push_back(z.n_nodes); }
  const size_t kk = (size_t)(k < 0 ? 0 : k) < c.size() ? (size_t)(k < 0 ? 0 : k) : c.size();
  std::partial_sort(c.begin(), c.begin() + (ptrdiff_t)kk, c.end(), std::greater<int64_t>());
  std::partial_sort(n.begin(), n.begin() + (ptrdiff_t)kk, n.end(), std::greater<int64_t>());
  *cells = 0; *nodes = 0;
  for (size_t i = 0; i < kk; ++i) { *cells += c[i]; *nodes += n[i]; }
}

// gather workgroups per chosen scenario: enough for the largest rows and the largest node block
static inline int64_t kas_choose_chunks(const KasChoosePlan& cp, int32_t dst_cell) {
  return kas_choose_chunks_of(cp.max_cells * dst_cell) + kas_choose_chunks_of((int64_t)cp.max_nodes * (int64_t)sizeof(kas_node_impact));
}

// Rack criteria (KAS_KEY_RACK_BASE .. KAS_KEY_RACK_END - 1) are known to the *_racks entries only: `racks` widens the key set.
static inline bool kas_key_is_rack(int32_t key) { return key >= KAS_KEY_RACK_BASE && key < KAS_KEY_RACK_END; }
// Topic criteria (KAS_KEY_TOPIC_BASE .. KAS_KEY_TOPIC_END - 1) are known to the *_topics entries only: `topics` widens it again.
static inline bool kas_key_is_topic(int32_t key) { return key >= KAS_KEY_TOPIC_BASE && key < KAS_KEY_TOPIC_END; }
static inline bool kas_key_known(int32_t key, bool racks, bool topics = false) {
  return (key >= 0 && key < KAS_KEY_COUNT) || (racks && kas_key_is_rack(key)) || (topics && kas_key_is_topic(key));
}

// "" or what is wrong with a spec for S scenarios (the text of the KAS_E_INVALID_ARG)
static inline const char* kas_choose_spec_error_keys(const kas_choose_spec* spec, int64_t S, bool racks, bool topics = false) {
  if (!spec) return "kas_choose_spec == NULL";
  if (spec->n_keys < 1 || spec->n_keys > KAS_CHOOSE_MAX_KEYS) return "kas_choose_spec: n_keys outside 1..4";
  for (int32_t i = 0; i < spec->n_keys; ++i)
    if (!kas_key_known(spec->key[i], racks, topics)) return "kas_choose_spec: unknown criterion";
  if (spec->k < 0 || spec->k > S) return "kas_choose_spec: k outside 0..n_scenarios";
  return "";
}
static inline const char* kas_choose_spec_error(const kas_choose_spec* spec, int64_t S) { return kas_choose_spec_error_keys(spec, S, false); }

// does a (valid) spec name a rack criterion: what the *_racks entries need rack records for
static inline bool kas_choose_spec_uses_racks(const kas_choose_spec* spec) {
  for (int32_t i = 0; i < spec->n_keys; ++i)
    if (kas_key_is_rack(spec->key[i])) return true;
  return false;
}
#define KAS_NO_RACK_RECORDS "rack criterion without rack records"   // the refusal of a rack criterion with NULL records

// ... and a topic criterion: what the *_topics entries need topic records for
static inline bool kas_choose_spec_uses_topics(const kas_choose_spec* spec) {
  for (int32_t i = 0; i < spec->n_keys; ++i)
    if (kas_key_is_topic(spec->key[i])) return true;
  return false;
}
#define KAS_NO_TOPIC_RECORDS "topic criterion without topic records"

// the spec's words of the launch arguments
static inline void kas_choose_fill_spec(KasChooseLaunch* a, const kas_choose_spec* spec, int32_t S) {
  a->S = S; a->n_keys = spec->n_keys; a->k = spec->k;
  for (int i = 0; i < KAS_CHOOSE_MAX_KEYS; ++i) a->key[i] = i < spec->n_keys ? spec->key[i] : 0;
}

// Kernel arguments of the rank kernel's instance that also reads scenario rack records (a struct of its own: the arguments of
// the instances above stay as they are).  srk: [S], never NULL here.
struct KasRackChooseLaunch {
  KasChooseLaunch c;
  const kas_scenario_rack_impact* srk;
};

// ... and of the instance that reads scenario rack records and scenario topic records.  stp: [S], never NULL here; srk: [S], or
// NULL when the spec names no rack criterion (it is then never dereferenced).
struct KasTopicChooseLaunch {
  KasChooseLaunch c;
  const kas_scenario_rack_impact* srk;
  const kas_scenario_topic_impact* stp;
};

// kas_choose.hip.  All return a hipError_t (0 = hipSuccess).  kas_gather_launch needs a.chunks * a.k below 2^31.
int kas_rank_launch(const KasChooseLaunch* a, void* hip_stream);
int kas_gather_launch(const KasChooseLaunch* a, void* hip_stream);
int kas_rank_racks_launch(const KasRackChooseLaunch* a, void* hip_stream);
int kas_rank_topics_launch(const KasTopicChooseLaunch* a, void* hip_stream);
