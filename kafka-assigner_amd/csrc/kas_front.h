// kas_front.h — the Pareto front of a solve's scenarios on the device (include/kas_abi.h: kas_front_spec): launch arguments of the
// two kernels and the launchers their translation unit (kas_choose.hip) exports to kas_hip.hip.  Device code: kas_front_body.h.
//
// Pure C++ (no HIP calls), as kas_choose.h, whose tables and gather kernel a front uses as they are.
//
// Two kernels in front of the gather kernel (and of the moves pass), which take the chosen[] and the offsets they leave:
//   mark        one lane per scenario, KAS_CHOOSE_BLOCK lanes a workgroup.  Every workgroup streams all S scenarios through the
//               LDS in tiles of KAS_CHOOSE_TILE entries: the four biased criteria, the OK flag and the eligible flag (OK, and
//               every bound holds).  A lane tests every entry against its own scenario — componentwise <=, any <, the index on
//               full equality — and writes its class: 0 for a member of the front, or KAS_FRONT_*.
//   front rank  kasc::rank_block (kas_choose_body.h) with "takes part" read from the classes instead of the status.
// Exact, no atomics, nothing between workgroups: the same inputs give the same bytes.
#pragma once
#include <stdint.h>

#include "kas_abi.h"
#include "kas_choose.h"

// Kernel arguments of both kernels: the choose arguments (of which the mark kernel reads sr, si, S, n_keys, key and n_ok), the bounds,
// the classes and the counts.
struct KasFrontLaunch {
  KasChooseLaunch c;
  int32_t n_limits, limit_key[KAS_CHOOSE_MAX_KEYS], limit[KAS_CHOOSE_MAX_KEYS];
  int32_t* cls;                         // [S] 0 for a member, or KAS_FRONT_*: written by mark, read by front rank
  int32_t* counts;                      // [4] n_ok, n_eligible (mark), n_front, 0 (front rank)
};

// "" or what is wrong with a spec for S scenarios (the text of the KAS_E_INVALID_ARG); racks: rack criteria are known (the
// *_racks entries)
static inline const char* kas_front_spec_error_keys(const kas_front_spec* spec, int64_t S, bool racks, bool topics = false) {
  if (!spec) return "kas_front_spec == NULL";
  if (spec->n_keys < 1 || spec->n_keys > KAS_CHOOSE_MAX_KEYS) return "kas_front_spec: n_keys outside 1..4";
  for (int32_t i = 0; i < spec->n_keys; ++i)
    if (!kas_key_known(spec->key[i], racks, topics)) return "kas_front_spec: unknown criterion";
  if (spec->n_limits < 0 || spec->n_limits > KAS_CHOOSE_MAX_KEYS) return "kas_front_spec: n_limits outside 0..4";
  for (int32_t i = 0; i < spec->n_limits; ++i)
    if (!kas_key_known(spec->limit_key[i], racks, topics)) return "kas_front_spec: unknown limit criterion";
  for (int32_t i = 0; i < spec->n_limits; ++i)
    if (spec->limit[i] < 0) return "kas_front_spec: negative limit";
  if (spec->k < 0 || spec->k > S) return "kas_front_spec: k outside 0..n_scenarios";
  return "";
}
static inline const char* kas_front_spec_error(const kas_front_spec* spec, int64_t S) { return kas_front_spec_error_keys(spec, S, false); }

// does a (valid) spec name a rack criterion, among its keys or its bounds
static inline bool kas_front_spec_uses_racks(const kas_front_spec* spec) {
  for (int32_t i = 0; i < spec->n_keys; ++i)
    if (kas_key_is_rack(spec->key[i])) return true;
  for (int32_t i = 0; i < spec->n_limits; ++i)
    if (kas_key_is_rack(spec->limit_key[i])) return true;
  return false;
}

// ... or a topic criterion
static inline bool kas_front_spec_uses_topics(const kas_front_spec* spec) {
  for (int32_t i = 0; i < spec->n_keys; ++i)
    if (kas_key_is_topic(spec->key[i])) return true;
  for (int32_t i = 0; i < spec->n_limits; ++i)
    if (kas_key_is_topic(spec->limit_key[i])) return true;
  return false;
}

// the part of a (valid) front spec that orders the members and sizes the outputs: what every choose decision reads
static inline kas_choose_spec kas_front_choose_spec(const kas_front_spec* spec) {
  kas_choose_spec cs;
  cs.n_keys = spec->n_keys; cs.k = spec->k;
  for (int i = 0; i < KAS_CHOOSE_MAX_KEYS; ++i) cs.key[i] = i < spec->n_keys ? spec->key[i] : 0;
  return cs;
}

// the spec's words of the launch arguments
static inline void kas_front_fill_spec(KasFrontLaunch* a, const kas_front_spec* spec, int32_t S) {
  const kas_choose_spec cs = kas_front_choose_spec(spec);
  kas_choose_fill_spec(&a->c, &cs, S);
  a->n_limits = spec->n_limits;
  for (int i = 0; i < KAS_CHOOSE_MAX_KEYS; ++i) {
    a->limit_key[i] = i < spec->n_limits ? spec->limit_key[i] : 0;
    a->limit[i] = i < spec->n_limits ? spec->limit[i] : 0;
  }
}

// workgroups of the mark kernel: one lane per scenario, and one workgroup at least (its first lane writes the counts)
static inline int64_t kas_front_mark_grid(int32_t S) {
  const int64_t g = ((int64_t)S + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK;
  return g < 1 ? 1 : g;
}

// Kernel arguments of the two kernels' instances that also read scenario rack records (as KasRackChooseLaunch).
struct KasRackFrontLaunch {
  KasFrontLaunch f;
  const kas_scenario_rack_impact* srk;  // [S], never NULL here
};

// ... and of the instances that read scenario rack records and scenario topic records (as KasTopicChooseLaunch).
struct KasTopicFrontLaunch {
  KasFrontLaunch f;
  const kas_scenario_rack_impact* srk;  // [S], or NULL when the spec names no rack criterion
  const kas_scenario_topic_impact* stp; // [S], never NULL here
};

// kas_choose.hip.  All return a hipError_t (0 = hipSuccess).
int kas_front_mark_launch(const KasFrontLaunch* a, void* hip_stream);
int kas_front_rank_launch(const KasFrontLaunch* a, void* hip_stream);
int kas_front_mark_racks_launch(const KasRackFrontLaunch* a, void* hip_stream);
int kas_front_rank_racks_launch(const KasRackFrontLaunch* a, void* hip_stream);
int kas_front_mark_topics_launch(const KasTopicFrontLaunch* a, void* hip_stream);
int kas_front_rank_topics_launch(const KasTopicFrontLaunch* a, void* hip_stream);
