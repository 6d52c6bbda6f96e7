// tests/emu/rack_driver.cpp — runs the rack pass's device code (csrc/kas_racks_body.h) on CPU fibers.
// TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp (the fiber scheduler) and impact_driver.cpp (the
// impact pass, whose node records the reduce kernel folds).
// kas_emu_racks() takes a batch and the tables a solve left, runs the impact pass (kas_emu_impact), builds the product's rack
// tables (kas_racks.h) and runs every item's workgroup of the row kernel, then every scenario's workgroup of the reduce kernel,
// as kas_rack_launch does on the GPU.  It keeps one KasRackPlan between calls, as a kas_plan does, and decides with the
// product's kas_rack_plan_serves whether a call rebuilds it.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_racks_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

extern "C" int kas_emu_impact(const kas_batch_desc* b, const kas_tables* t, int cells16, int node_cap_limit, int64_t rows_per_item,
                              kas_node_impact* nodes, kas_scenario_impact* scenarios, int32_t* info, char* errbuf, int errlen);

namespace {

struct Args { const KasRackLaunch* a; int32_t i; unsigned char* lds; };

template <int W, bool C16> void run_rows(void* p) {
  Args* r = (Args*)p;
  kasr::rack_item<W, C16>(*r->a, r->i, r->lds);
}
void run_reduce(void* p) {
  Args* r = (Args*)p;
  kasr::rack_reduce(*r->a, r->i, r->lds);
}
typedef void (*run_fn)(void*);
template <bool C16> run_fn rows_for(int32_t wc) {     // (the instances kas_rack_launch picks)
  return wc <= 3 ? run_rows<3, C16> : (wc <= 5 ? run_rows<5, C16> : run_rows<8, C16>);
}

KasRackPlan g_plan;            // the "plan's" rack tables, kept between calls
int g_ready = 0;

}  // namespace

// Forget the kept rack tables (a plan rebuilt for another batch).
extern "C" __attribute__((visibility("default")))
void kas_emu_racks_reset(void) { g_ready = 0; }

// t->cur / t->out: int32 pools, or uint16 pools (cells16).  report_rack: node_pool_len entries or NULL.  rows_per_item > 0:
// rows of an item instead of the product's rule; rack_cap_limit >= 0: the racks from global memory when the largest scenario
// has more nodes.  nodes / scenarios: the impact pass's records (written here); racks [racks_cap], rack_scenarios [S],
// rack_off [S + 1]: the rack pass's.  info (may be NULL) <- 1 when the rack tables were (re)built, racks in the LDS, items,
// the largest R_s.  Returns 0, -100 on divergence / deadlock or an LDS write beyond a launch's allocation, or a KAS_E_* code.
extern "C" __attribute__((visibility("default")))
int kas_emu_racks(const kas_batch_desc* b, const kas_tables* t, int cells16, int64_t rows_per_item, int rack_cap_limit,
                  const int32_t* report_rack, kas_node_impact* nodes, kas_scenario_impact* scenarios, kas_rack_impact* racks,
                  int64_t racks_cap, kas_scenario_rack_impact* rack_scenarios, int64_t* rack_off, int32_t* info, char* errbuf, int errlen) {
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
  int rc = kas_shape_batch(&bb, &sh, &err, 0, 0);
  if (rc != KAS_E_OK) { say(err); return rc; }
  // the refusals, in the library's order (kas_rack_impl): the table, then the capacity
  if (report_rack && bb.node_pool_len <= 0) { say("report_rack: a table for a batch without nodes"); return KAS_E_INVALID_ARG; }
  const int32_t* table = report_rack ? report_rack : bb.node_rack;
  const bool same = g_ready && kas_rack_plan_serves(g_plan, table, bb.node_pool_len);
  if (!same) {
    KasRackPlan fresh;
    rc = kas_rack_plan_build(&bb, table, sh.n_max, sh.idmap_entries, sh.need_bsearch, cells16, rack_cap_limit, &fresh, &err);
    if (rc != KAS_E_OK) { say(err); return rc; }
    g_plan = fresh;
    g_ready = 1;
  }
  const KasRackPlan& rp = g_plan;
  const int32_t S = bb.n_scenarios;
  if (racks_cap < rp.rack_off[(size_t)S]) { say("kas_rack_tables: racks_cap below the sum of the scenarios' rack counts"); return KAS_E_INVALID_ARG; }
  memcpy(rack_off, rp.rack_off.data(), sizeof(int64_t) * ((size_t)S + 1));
  // the impact pass, then the work list it ran (the same call builds the same list)
  rc = kas_emu_impact(b, t, cells16, -1, rows_per_item, nodes, scenarios, nullptr, errbuf, errlen);
  if (rc != KAS_E_OK) return rc;
  KasImpactPlan ip;
  kas_impact_plan_build(&bb, sh.n_max, sh.idmap_entries, sh.need_bsearch, cells16, -1,
                        rows_per_item > 0 ? rows_per_item : kas_impact_rows_per_item(&bb), &ip);
  std::vector<int32_t> sums((size_t)KAS_RACK_SUMS * (size_t)(S + 1), 0);
  KasRackLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = bb.scenarios; a.topics = bb.topics; a.node_id = bb.node_id;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.items = ip.items.data(); a.rr = rp.rr.data();
  a.node_base = ip.node_base.data(); a.rack_off = rp.rack_off.data(); a.sums = sums.data();
  a.nodes = nodes; a.racks = racks; a.scenarios = rack_scenarios;
  a.n_items = (int32_t)ip.items.size(); a.n_scenarios = S;
  a.idmap_entries = sh.idmap_entries;
  a.off_rack = rp.off_rack; a.racks_in_lds = rp.racks_in_lds; a.lds_bytes = rp.lds_bytes; a.reduce_lds_bytes = rp.reduce_lds_bytes;
  a.cells16 = cells16;
  auto bad = [&](const char* what, int32_t i) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %d", what, i);
    return -100;
  };
  // exactly the LDS the product launches each kernel with (uninitialised on hardware: 0xCD here), and a guard behind it
  auto run = [&](run_fn fn, int32_t n, size_t bytes, const char* name) {
    std::vector<unsigned char> lds(bytes + 4096);
    for (int32_t i = 0; i < n; ++i) {
      memset(lds.data(), 0xCD, bytes);
      memset(lds.data() + bytes, 0xA5, 4096);
      Args r{&a, i, lds.data()};
      if (kasw::run_block(fn, &r, KAS_RACK_BLOCK / 64) != 0) return bad(name, i);
      for (size_t k = 0; k < 4096; ++k)
        if (lds[bytes + k] != 0xA5) return bad("rack pass: LDS written beyond the launch's bytes", i);
    }
    return 0;
  };
  if ((rc = run(cells16 ? rows_for<true>(sh.Wc) : rows_for<false>(sh.Wc), a.n_items, (size_t)rp.lds_bytes, "rack rows: divergence / deadlock")) != 0) return rc;
  if ((rc = run(run_reduce, S, (size_t)rp.reduce_lds_bytes, "rack reduce: divergence / deadlock")) != 0) return rc;
  if (info) { info[0] = same ? 0 : 1; info[1] = rp.racks_in_lds; info[2] = a.n_items; info[3] = rp.r_max; }
  return KAS_E_OK;
}

// kas_plan_host_call for a kas_solve_host_rack_impact call (racks != 0) or a kas_solve_host_impact call (racks == 0), without
// running anything.  lens[4]: cur_len, out_len, aux_len, ctx_len; n_select < 0: every row; have_nodes: host_impact->nodes is
// there; missing: bit 0 racks, 1 scenarios, 2 rack_off of kas_rack_tables.  bytes [KAS_HB_LAST] in KasHostBuf's order;
// rack_off [S + 1] when racks.  Returns the planner's code; its text in errbuf.
extern "C" __attribute__((visibility("default")))
int kas_emu_rack_host_call(const kas_batch_desc* b, const int64_t* lens, int32_t n_select, int cells16, int racks, int have_nodes,
                           const int32_t* report_rack, int64_t racks_cap, unsigned missing, int64_t* bytes, int64_t* rack_off,
                           char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.cur_len = lens[0]; in.out_len = lens[1]; in.aux_len = lens[2]; in.ctx_len = lens[3];
  in.have_cur = in.have_out = in.have_aux = in.have_ctx = in.have_topic_results = in.have_scenario_results = true;
  in.n_select = n_select;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  in.impact = true; in.have_imp_nodes = have_nodes != 0; in.have_imp_scenarios = true;
  if (racks) {
    in.racks = true; in.report_rack = report_rack; in.racks_cap = racks_cap;
    in.have_rk_racks = !(missing & 1u); in.have_rk_scenarios = !(missing & 2u); in.have_rk_off = !(missing & 4u);
  }
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  for (int i = 0; i < KAS_HB_LAST; ++i) bytes[i] = (int64_t)hc.bytes[i];
  for (size_t i = 0; i < hc.rack.rack_off.size(); ++i) rack_off[i] = hc.rack.rack_off[i];
  return rc;
}
extern "C" __attribute__((visibility("default")))
int kas_emu_rack_buffers(int which) { return which == 0 ? KAS_HB_LAST : KAS_HB_END; }
