// tests/emu/topic_driver.cpp — runs the topic pass's device code (csrc/kas_topics_body.h) on CPU fibers.
// TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp, which provides the fiber scheduler.
// kas_emu_topics() takes a batch and the tables a solve left, builds the product's work list (kas_topics.h) and runs every
// item's workgroup, then every merge workgroup, then every scenario's summary workgroup, as kas_topic_launch does on the GPU.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_topics_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

namespace {

struct Args { const KasTopicLaunch* a; int32_t i; unsigned char* lds; };

template <int W, bool C16> void run_item(void* p) {
  Args* r = (Args*)p;
  kast::topic_item<W, C16>(*r->a, r->i, r->lds);
}
void run_merge(void* p) {
  Args* r = (Args*)p;
  kast::topic_merge(*r->a, r->i, (int32_t*)r->lds);
}
void run_summary(void* p) {
  Args* r = (Args*)p;
  kast::topic_summary(*r->a, r->i, (int32_t*)r->lds);
}
typedef void (*run_fn)(void*);
template <bool C16> run_fn item_for(int32_t wc) {   // (the instances kas_topic_launch picks)
  return wc <= 3 ? run_item<3, C16> : (wc <= 5 ? run_item<5, C16> : run_item<8, C16>);
}

uint32_t g_lds_fill = 0xCDCDCDCDu;

}  // namespace

// The word every workgroup finds all over its LDS when it starts (default 0xCDCDCDCD).  LDS is uninitialised on hardware: it holds
// what the workgroup before left there, an id table for instance, and a test may want exactly that behind this launch's tables.
extern "C" __attribute__((visibility("default")))
void kas_emu_topics_lds_fill(uint32_t word) { g_lds_fill = word; }

// t->cur / t->out: int32 pools, or uint16 pools (cells16; b->node_id is then not read).  node_cap_limit >= 0: topics of
// scenarios above that many nodes count in global scratch; rows_per_item > 0: rows of an item instead of the product's rule.
// topics [T], scenarios [S]: the pass's records.  items (may be NULL): the work list, six int32 per item as KasImpactItem, at
// most items_cap of them.  info (may be NULL) <- items, merge workgroups, FLUSH items, GLOBAL items, node_cap, and region_ints
// as two int32 (low, high).  Returns 0, -100 on divergence / deadlock or an LDS write beyond a launch's allocation, or a KAS_E_*
// code (the scratch limit: KAS_E_UNSUPPORTED, before anything runs).
extern "C" __attribute__((visibility("default")))
int kas_emu_topics(const kas_batch_desc* b, const kas_tables* t, int cells16, int node_cap_limit, int64_t rows_per_item,
                   kas_topic_impact* topics, kas_scenario_topic_impact* scenarios, int32_t* items, int32_t items_cap, int32_t* info,
                   char* errbuf, int errlen) {
  auto say = [&](const std::string& m) { if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", m.c_str()); };
  KasShape sh;
  std::string err;
  std::vector<int32_t> ident;
  kas_batch_desc bb = *b;
  if (cells16) {                                       // (the plan's node table: node i has id i)
    ident.assign((size_t)(b->node_pool_len > 0 ? b->node_pool_len : 1), 0);
    for (int32_t s = 0; s < b->n_scenarios; ++s)
      for (int32_t i = 0; i < b->scenarios[s].n_nodes; ++i) ident[(size_t)(b->scenarios[s].node_off + i)] = i;
    bb.node_id = ident.data();
  }
  const int rc = kas_shape_batch(&bb, &sh, &err, 0, 0);
  if (rc != KAS_E_OK) { say(err); return rc; }
  KasTopicPlan tp;
  kas_topic_plan_build(&bb, sh.n_max, sh.idmap_entries, sh.need_bsearch, cells16, node_cap_limit,
                       rows_per_item > 0 ? rows_per_item : kas_impact_rows_per_item(&bb), &tp);
  if (!kas_topic_scratch_ok(tp)) { say(KAS_TOPIC_SCRATCH_TEXT); return KAS_E_UNSUPPORTED; }
  std::vector<int32_t> region((size_t)tp.region_ints + 1, 0);
  KasTopicLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = bb.scenarios; a.topics = bb.topics; a.node_id = bb.node_id;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.items = tp.items.data(); a.merge = tp.merge.data();
  a.region_off = tp.region_off.data(); a.region = region.data();
  a.topic_out = topics; a.scenarios = scenarios;
  a.n_items = (int32_t)tp.items.size(); a.n_merge = (int32_t)tp.merge.size(); a.n_scenarios = bb.n_scenarios;
  a.idmap_entries = sh.idmap_entries;
  a.off_look = tp.off_look; a.off_red = tp.off_red; a.lds_bytes = tp.lds_bytes; a.cells16 = cells16;
  auto bad = [&](const char* what, int32_t i) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %d", what, i);
    return -100;
  };
  // exactly the LDS the product launches each kernel with (uninitialised on hardware: the fill word here), and a guard behind it
  auto run = [&](run_fn fn, int32_t n, size_t bytes, const char* name) {
    std::vector<unsigned char> lds(bytes + 4096);
    for (int32_t i = 0; i < n; ++i) {
      for (size_t k = 0; k + 4 <= bytes; k += 4) memcpy(lds.data() + k, &g_lds_fill, 4);
      memset(lds.data() + bytes, 0xA5, 4096);
      Args r{&a, i, lds.data()};
      if (kasw::run_block(fn, &r, KAS_TOPIC_BLOCK / 64) != 0) return bad(name, i);
      for (size_t k = 0; k < 4096; ++k)
        if (lds[bytes + k] != 0xA5) return bad("topic pass: LDS written beyond the launch's bytes", i);
    }
    return 0;
  };
  int e;
  if ((e = run(cells16 ? item_for<true>(sh.Wc) : item_for<false>(sh.Wc), a.n_items, (size_t)tp.lds_bytes, "topic item: divergence / deadlock")) != 0) return e;
  if ((e = run(run_merge, a.n_merge, 4 * KAS_TOPIC_RED * (KAS_TOPIC_BLOCK / 64), "topic merge: divergence / deadlock")) != 0) return e;
  if ((e = run(run_summary, a.n_scenarios, 4 * KAS_TOPIC_WORDS * (KAS_TOPIC_BLOCK / 64), "topic summary: divergence / deadlock")) != 0) return e;
  int32_t flush = 0, global = 0;
  for (size_t i = 0; i < tp.items.size(); ++i) {
    flush += tp.items[i].mode == KAS_TOPIC_FLUSH ? 1 : 0;
    global += tp.items[i].mode == KAS_TOPIC_GLOBAL ? 1 : 0;
    if (items && (int32_t)i < items_cap) memcpy(items + 6 * i, &tp.items[i], sizeof(KasImpactItem));
  }
  if (info) {
    info[0] = a.n_items; info[1] = a.n_merge; info[2] = flush; info[3] = global; info[4] = tp.node_cap;
    info[5] = (int32_t)(tp.region_ints & 0xffffffff); info[6] = (int32_t)(tp.region_ints >> 32);
  }
  return KAS_E_OK;
}

// kas_plan_host_call for a kas_solve_host_topic_impact call (topics != 0) or a kas_solve_host_impact call (topics == 0), without
// running anything.  lens[4]: cur_len, out_len, aux_len, ctx_len; n_select < 0: every row; impact: host_impact is there, and
// have_nodes: host_impact->nodes too; missing: bit 0 host_topics itself, 1 its topics, 2 its scenarios.  bytes [KAS_HB_EVERY] in
// KasHostBuf's order; region_ints <- the global counters of the call's work list.  Returns the planner's code; its text in errbuf.
extern "C" __attribute__((visibility("default")))
int kas_emu_topic_host_call(const kas_batch_desc* b, const int64_t* lens, int32_t n_select, int cells16, int topics, int impact,
                            int have_nodes, unsigned missing, int64_t* bytes, int64_t* region_ints, char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.cur_len = lens[0]; in.out_len = lens[1]; in.aux_len = lens[2]; in.ctx_len = lens[3];
  in.have_cur = in.have_out = in.have_aux = in.have_ctx = in.have_topic_results = in.have_scenario_results = true;
  in.n_select = n_select;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  in.impact = impact != 0; in.have_imp_nodes = impact && have_nodes; in.have_imp_scenarios = impact != 0;
  if (topics) {
    in.topics = true;
    in.have_tp_tables = !(missing & 1u); in.have_tp_topics = !(missing & 3u); in.have_tp_scenarios = !(missing & 5u);
  }
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  for (int i = 0; i < KAS_HB_EVERY; ++i) bytes[i] = (int64_t)hc.bytes[i];
  *region_ints = hc.tp_region_ints;
  return rc;
}
extern "C" __attribute__((visibility("default")))
int kas_emu_topic_buffers(int which) { return which == 0 ? KAS_HB_EVERY : KAS_HB_LAST; }
