// tests/emu/impact_driver.cpp — runs the impact pass's device code (csrc/kas_impact_body.h) on CPU fibers.
// TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp, which provides the fiber scheduler.
// kas_emu_impact() takes a batch and the tables a solve left, builds the product's work list (kas_impact.h) and runs every
// item's workgroup, then every merge workgroup, as kas_impact_launch does on the GPU.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_impact_body.h"
#include "kas_plan_math.h"

namespace {

struct ItemArgs { const KasImpactLaunch* a; int32_t i; unsigned char* lds; };

template <int W, bool C16> void run_item(void* p) {
  ItemArgs* r = (ItemArgs*)p;
  kasi::impact_item<W, C16>(*r->a, r->i, r->lds);
}
void run_merge(void* p) {
  ItemArgs* r = (ItemArgs*)p;
  kasi::impact_merge(*r->a, r->i, (int32_t*)r->lds);
}
typedef void (*run_fn)(void*);
template <bool C16> run_fn item_for(int32_t wc) {   // (the instances kas_impact_launch picks)
  return wc <= 3 ? run_item<3, C16> : (wc <= 5 ? run_item<5, C16> : run_item<8, C16>);
}

uint32_t g_lds_fill = 0xCDCDCDCDu;

}  // namespace

// The word every workgroup finds all over its LDS when it starts (default 0xCDCDCDCD).  LDS is uninitialised on hardware: it holds
// what the workgroup before left there, an id table for instance, and a test may want exactly that behind this launch's tables.
extern "C" __attribute__((visibility("default")))
void kas_emu_impact_lds_fill(uint32_t word) { g_lds_fill = word; }

// t->cur / t->out: int32 pools, or uint16 pools (cells16; b->node_id is then not read).  node_cap_limit >= 0: count scenarios
// above that many nodes in global scratch; rows_per_item > 0: rows of an item instead of the product's rule.
// info (may be NULL) <- items, merge workgroups, items counting in global scratch, node_cap.  Returns 0, -100 on divergence /
// deadlock or an LDS write beyond the launch's allocation, or a KAS_E_* code.
extern "C" __attribute__((visibility("default")))
int kas_emu_impact(const kas_batch_desc* b, const kas_tables* t, int cells16, int node_cap_limit, int64_t rows_per_item,
                   kas_node_impact* nodes, kas_scenario_impact* scenarios, int32_t* info, char* errbuf, int errlen) {
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
  if (rc != KAS_E_OK) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", err.c_str());
    return rc;
  }
  KasImpactPlan ip;
  kas_impact_plan_build(&bb, sh.n_max, sh.idmap_entries, sh.need_bsearch, cells16, node_cap_limit,
                        rows_per_item > 0 ? rows_per_item : kas_impact_rows_per_item(&bb), &ip);
  std::vector<int32_t> region((size_t)ip.region_ints + 1, 0);
  KasImpactLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = bb.scenarios; a.topics = bb.topics; a.node_id = bb.node_id;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.items = ip.items.data(); a.merge_scen = ip.merge_scen.data();
  a.node_base = ip.node_base.data(); a.region_off = ip.region_off.data(); a.region = region.data();
  a.nodes = nodes; a.scenarios = scenarios;
  a.n_items = (int32_t)ip.items.size(); a.n_merge = (int32_t)ip.merge_scen.size();
  a.node_cap = ip.node_cap; a.idmap_entries = sh.idmap_entries;
  a.off_look = ip.off_look; a.off_red = ip.off_red; a.lds_bytes = ip.lds_bytes; a.cells16 = cells16;
  auto bad = [&](const char* what, int32_t i) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %d", what, i);
    return -100;
  };
  // exactly the LDS the product launches the item kernel with, and a guard behind it
  const size_t bytes = (size_t)ip.lds_bytes;
  std::vector<unsigned char> lds(bytes + 4096);
  const run_fn item = cells16 ? item_for<true>(sh.Wc) : item_for<false>(sh.Wc);
  int32_t global_items = 0;
  for (int32_t i = 0; i < a.n_items; ++i) {
    global_items += ip.items[(size_t)i].mode == KAS_IMPACT_GLOBAL ? 1 : 0;
    for (size_t k = 0; k + 4 <= bytes; k += 4) memcpy(lds.data() + k, &g_lds_fill, 4);   // LDS is uninitialised on hardware too
    memset(lds.data() + bytes, 0xA5, 4096);
    ItemArgs r{&a, i, lds.data()};
    if (kasw::run_block(item, &r, KAS_IMPACT_BLOCK / 64) != 0) return bad("impact item: divergence / deadlock", i);
    for (size_t k = 0; k < 4096; ++k)
      if (lds[bytes + k] != 0xA5) return bad("impact item: LDS written beyond lds_bytes", i);
  }
  std::vector<int32_t> red(KAS_IMPACT_FIELDS * (KAS_IMPACT_BLOCK / 64), (int32_t)0xCDCDCDCD);
  for (int32_t m = 0; m < a.n_merge; ++m) {
    ItemArgs r{&a, m, (unsigned char*)red.data()};
    if (kasw::run_block(run_merge, &r, KAS_IMPACT_BLOCK / 64) != 0) return bad("impact merge: divergence / deadlock", m);
  }
  if (info) { info[0] = a.n_items; info[1] = a.n_merge; info[2] = global_items; info[3] = ip.node_cap; }
  return KAS_E_OK;
}
