// tests/emu/topic_choose_driver.cpp — runs the instances of the rank, mark and front rank kernels' device code that read the
// scenario topic records (csrc/kas_choose_body.h, kas_front_body.h with kasc::TopicRecords) and the gather kernel's on CPU fibers,
// and exports the host call planner with the arguments of the *_topics host entries.  TEST INFRASTRUCTURE: see tests/emu/kas_wave.h;
// linked with emu_driver.cpp, which provides the fiber scheduler.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_front_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

namespace {

// which instance is stepped: the one that was always there, the one that reads srk, the one that reads srk and stp
enum Src { SRC_RECORDS = 0, SRC_RACKS = 1, SRC_TOPICS = 2 };

struct BlockArgs {
  const KasFrontLaunch* a; const kas_scenario_rack_impact* srk; const kas_scenario_topic_impact* stp; int src; bool front; int64_t i;
  unsigned char* lds;
};

void run_mark(void* p) {
  BlockArgs* r = (BlockArgs*)p;
  if (r->src == SRC_TOPICS) kasf::mark_block(*r->a, (int32_t)r->i, (kasf::Entry*)r->lds, kasc::TopicRecords{r->srk, r->stp});
  else if (r->src == SRC_RACKS) kasf::mark_block(*r->a, (int32_t)r->i, (kasf::Entry*)r->lds, kasc::RackRecords{r->srk});
  else kasf::mark_block(*r->a, (int32_t)r->i, (kasf::Entry*)r->lds);
}
void run_rank(void* p) {
  BlockArgs* r = (BlockArgs*)p;
  if (r->front) {
    if (r->src == SRC_TOPICS) kasf::rank_block(*r->a, (int32_t)r->i, (kasc::Entry*)r->lds, kasc::TopicRecords{r->srk, r->stp});
    else if (r->src == SRC_RACKS) kasf::rank_block(*r->a, (int32_t)r->i, (kasc::Entry*)r->lds, kasc::RackRecords{r->srk});
    else kasf::rank_block(*r->a, (int32_t)r->i, (kasc::Entry*)r->lds);
  } else {
    if (r->src == SRC_TOPICS) kasc::rank_block(r->a->c, (int32_t)r->i, (kasc::Entry*)r->lds, kasc::ByStatus(), kasc::TopicRecords{r->srk, r->stp});
    else if (r->src == SRC_RACKS) kasc::rank_block(r->a->c, (int32_t)r->i, (kasc::Entry*)r->lds, kasc::ByStatus(), kasc::RackRecords{r->srk});
    else kasc::rank_block(r->a->c, (int32_t)r->i, (kasc::Entry*)r->lds);
  }
}
void run_gather(void* p) {
  BlockArgs* r = (BlockArgs*)p;
  kasc::gather_item(r->a->c, r->i);
}

int bad(char* errbuf, int errlen, const char* what, int64_t i) {
  if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %lld", what, (long long)i);
  return -100;
}

// every workgroup of a kernel with an LDS tile: the tile full of `lds_fill`, a guard behind it
int tiled_all(void (*fn)(void*), BlockArgs r, int64_t grid, uint32_t lds_fill, const char* name, char* errbuf, int errlen) {
  static_assert(sizeof(kasf::Entry) == sizeof(kasc::Entry), "one tile size");
  const size_t bytes = sizeof(kasc::Entry) * KAS_CHOOSE_TILE;
  std::vector<unsigned char> lds(bytes + 4096);
  for (int64_t i = 0; i < grid; ++i) {
    for (size_t k = 0; k + 4 <= bytes; k += 4) memcpy(lds.data() + k, &lds_fill, 4);   // LDS is uninitialised on hardware too
    memset(lds.data() + bytes, 0xA5, 4096);
    r.i = i; r.lds = lds.data();
    if (kasw::run_block(fn, &r, KAS_CHOOSE_BLOCK / 64) != 0) return bad(errbuf, errlen, name, i);
    for (size_t k = 0; k < 4096; ++k)
      if (lds[bytes + k] != 0xA5) return bad(errbuf, errlen, "LDS written beyond the tile", i);
  }
  return 0;
}

// rank, or mark and front rank, as the launchers' grids; cls: S entries and a guard behind them
int rank_all(KasFrontLaunch& a, const kas_scenario_rack_impact* srk, const kas_scenario_topic_impact* stp, int src, bool front,
             uint32_t lds_fill, char* errbuf, int errlen) {
  const int32_t S = a.c.S;
  std::vector<int32_t> cls((size_t)S + 1, 0x7B7B7B7B);
  a.cls = cls.data();
  BlockArgs r{&a, srk, stp, src, front, 0, nullptr};
  int rc = 0;
  if (front) rc = tiled_all(run_mark, r, kas_front_mark_grid(S), lds_fill, "mark kernel: divergence / deadlock", errbuf, errlen);
  if (rc == 0)
    rc = tiled_all(run_rank, r, ((int64_t)S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK, lds_fill, "rank kernel: divergence / deadlock", errbuf, errlen);
  if (rc == 0 && cls[(size_t)S] != 0x7B7B7B7B) rc = bad(errbuf, errlen, "the classes were written beyond S", -1);
  a.cls = nullptr;
  return rc;
}

// The refusals of the *_topics entries that need no plan: the spec with the key set widened twice, then the missing rack records,
// then the missing topic records.  *src <- the instance the library launches for the spec.
int refuse(const kas_front_spec* front, const kas_choose_spec* spec, int64_t S, bool have_srk, bool have_stp, int* src, char* errbuf,
           int errlen) {
  const char* refusal = front ? kas_front_spec_error_keys(front, S, true, true) : kas_choose_spec_error_keys(spec, S, true, true);
  if (!refusal[0]) {
    const bool racks = front ? kas_front_spec_uses_racks(front) : kas_choose_spec_uses_racks(spec);
    const bool topics = front ? kas_front_spec_uses_topics(front) : kas_choose_spec_uses_topics(spec);
    *src = topics ? SRC_TOPICS : racks ? SRC_RACKS : SRC_RECORDS;
    if (racks && !have_srk) refusal = KAS_NO_RACK_RECORDS;
    else if (topics && !have_stp) refusal = KAS_NO_TOPIC_RECORDS;
  }
  if (!refusal[0]) return 0;
  if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", refusal);
  return KAS_E_INVALID_ARG;
}

void fill(KasFrontLaunch* a, const kas_front_spec* front, const kas_choose_spec* spec, int32_t S) {
  if (front) kas_front_fill_spec(a, front, S);
  else kas_choose_fill_spec(&a->c, spec, S);
}

}  // namespace

// Rank (spec) or mark and front rank (front; exactly one of the two) over S records, as kas_rank_device_topics /
// kas_front_rank_device_topics.  srk / stp may be NULL when no criterion of their set is named.  path: 0 = the instances the
// library launches (the topic instances iff the spec names a topic criterion, else the rack instances iff it names a rack
// criterion, else the oldest), 1 = the rack instances (srk != NULL, no topic criterion), 2 = the topic instances whatever the spec
// names (stp != NULL; srk may be NULL without a rack criterion).
// cells / n_nodes ([S], both or neither): the size table's columns — with them row_off and node_off ([k + 1]) are written.
// counts: [4], a front's.  Returns 0, -100 on divergence / deadlock / a write beyond the tile or the classes, or KAS_E_INVALID_ARG
// with the refusal's text.
extern "C" __attribute__((visibility("default")))
int kas_emu_topic_rank(const kas_scenario_result* sr, const kas_scenario_impact* si, const kas_scenario_rack_impact* srk,
                       const kas_scenario_topic_impact* stp, int32_t S, const kas_front_spec* front, const kas_choose_spec* spec, int path,
                       const int64_t* cells, const int32_t* n_nodes, int32_t* rank, int32_t* chosen, int64_t* row_off, int64_t* node_off,
                       int32_t* n_ok, int32_t* counts, uint32_t lds_fill, char* errbuf, int errlen) {
  int src = SRC_RECORDS;
  if (refuse(front, spec, S, srk != nullptr, stp != nullptr, &src, errbuf, errlen)) return KAS_E_INVALID_ARG;
  if (path == 1) src = SRC_RACKS;
  if (path == 2) src = SRC_TOPICS;
  std::vector<KasChooseSize> sizes;
  if (cells && n_nodes) {
    sizes.assign((size_t)S + 1, KasChooseSize{});
    for (int32_t s = 0; s < S; ++s) { sizes[(size_t)s].cells = cells[s]; sizes[(size_t)s].n_nodes = n_nodes[s]; }
  }
  KasFrontLaunch a;
  memset(&a, 0, sizeof(a));
  a.c.sr = sr; a.c.si = si;
  a.c.sizes = sizes.empty() ? nullptr : sizes.data();
  fill(&a, front, spec, S);
  a.c.rank = rank; a.c.chosen = chosen; a.c.row_off = row_off; a.c.node_off = node_off; a.c.n_ok = n_ok;
  a.counts = counts;
  return rank_all(a, srk, stp, src, front != nullptr, lds_fill, errbuf, errlen);
}

// Rank (or mark and front rank) and gather over the tables a solve, its impact pass, its rack pass and its topic pass left, as
// kas_choose_device_topics / kas_front_device_topics do.  cells: 0 = int32 cells, 1 = 16-bit cells, 2 = int32 cells in `out`
// gathered into 16-bit rows (the widened 16-bit host call).
extern "C" __attribute__((visibility("default")))
int kas_emu_topic_choose(const kas_batch_desc* b, const kas_tables* t, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                         const kas_scenario_topic_impact* stp, int cells, const kas_front_spec* front, const kas_choose_spec* spec,
                         const kas_choice* ch, int32_t* counts, uint32_t lds_fill, char* errbuf, int errlen) {
  int src = SRC_RECORDS;
  if (refuse(front, spec, b->n_scenarios, srk != nullptr, stp != nullptr, &src, errbuf, errlen)) return KAS_E_INVALID_ARG;
  KasChoosePlan cp;
  kas_choose_plan_build(b, &cp);
  const int64_t chunks = kas_choose_chunks(cp, cells == 0 ? 4 : 2);
  cp.sizes.push_back(KasChooseSize{});                 // (one spare entry each: data() of an empty batch's tables is not NULL)
  cp.segs.push_back(KasChooseSeg{});
  KasFrontLaunch a;
  memset(&a, 0, sizeof(a));
  a.c.sr = t->scenario_results; a.c.si = imp->scenarios;
  a.c.sizes = cp.sizes.data(); a.c.segs = cp.segs.data();
  fill(&a, front, spec, b->n_scenarios);
  a.c.rank = ch->rank; a.c.chosen = ch->chosen; a.c.row_off = ch->row_off; a.c.node_off = ch->node_off; a.c.n_ok = ch->n_ok;
  a.c.out = t->out; a.c.src_nodes = imp->nodes; a.c.rows = ch->rows; a.c.nodes = ch->nodes;
  a.c.src_cell = cells == 1 ? 2 : 4; a.c.dst_cell = cells == 0 ? 4 : 2;
  a.c.chunks = (int32_t)chunks;
  a.counts = counts;
  int rc = rank_all(a, srk, stp, src, front != nullptr, lds_fill, errbuf, errlen);
  const int64_t grid = (int64_t)a.c.k * a.c.chunks;
  for (int64_t i = 0; i < grid && rc == 0; ++i) {
    BlockArgs r{&a, nullptr, nullptr, SRC_RECORDS, false, i, nullptr};
    if (kasw::run_block(run_gather, &r, KAS_CHOOSE_BLOCK / 64) != 0) rc = bad(errbuf, errlen, "gather kernel: divergence / deadlock", i);
  }
  return rc;
}

// kas_plan_host_call for a kas_solve_host_choose_topics / 16 call (spec) or a kas_solve_host_front_topics / 16 call (front); mv may
// be NULL.  rack_keys / topic_keys 0 plan the call of the same arguments that knows no criterion of that set (both 0: the oldest
// entries), racks 0 a call without a rack pass (host_racks == NULL), topics 0 one without a topic pass (host_topics == NULL).
// With neither front nor spec: a kas_solve_host_topic_impact call (topics) or a kas_solve_host_impact call, n_select as given.
// lens: cur, aux, ctx lengths, rows_cap, nodes_cap, racks_cap, out_len (read without a choice only).  missing: bits of what is
// NULL — 1 cur, 4 aux, 8 ctx, 16 topic_results, 32 scenario_results, 64 impact nodes (without a choice; a choice never has them),
// 128 impact scenarios, then the kas_choice arrays: 256 rank, 512 chosen, 1024 row_off, 2048 node_off, 4096 n_ok, 8192 rows, 16384
// nodes, 32768 counts, then the kas_rack_tables arrays: 65536 racks, 131072 scenarios, 262144 rack_off, then the
// kas_topic_impact_tables arrays: 524288 topics, 1048576 scenarios.
// head [11] <- rows needed, node records needed, gather workgroups per chosen, header bytes, rows gathered, K, native16, listed,
// rack records, the largest R_s, the topic pass's global counters; bytes [kas_emu_topic_choose_buffers()]
extern "C" __attribute__((visibility("default")))
int kas_emu_topic_choose_host_call(const kas_batch_desc* b, const int64_t* lens, unsigned missing, int cells16, const kas_front_spec* front,
                                   const kas_choose_spec* spec, const kas_moves* mv, int racks, int rack_keys, int topics, int topic_keys,
                                   const int32_t* report_rack, int32_t n_select, int64_t* head, int64_t* bytes, char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  const bool choice = front || spec;
  KasHostCallIn in;
  in.batch = b;
  in.cur_len = lens[0]; in.out_len = choice ? 0 : lens[6]; in.aux_len = lens[1]; in.ctx_len = lens[2];
  in.have_cur = !(missing & 1u); in.have_out = !choice; in.have_aux = !(missing & 4u); in.have_ctx = !(missing & 8u);
  in.have_topic_results = !(missing & 16u); in.have_scenario_results = !(missing & 32u);
  in.select = nullptr; in.n_select = choice ? 0 : n_select;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  in.impact = true; in.have_imp_nodes = !choice && !(missing & 64u); in.have_imp_scenarios = !(missing & 128u);
  if (choice) {
    in.choose = spec; in.rows_cap = lens[3]; in.nodes_cap = lens[4];
    in.have_ch_rank = !(missing & 256u); in.have_ch_chosen = !(missing & 512u); in.have_ch_row_off = !(missing & 1024u);
    in.have_ch_node_off = !(missing & 2048u); in.have_ch_n_ok = !(missing & 4096u);
    in.have_ch_rows = !(missing & 8192u); in.have_ch_nodes = !(missing & 16384u);
  }
  if (front) { in.choose = nullptr; in.front = front; in.have_fr_counts = !(missing & 32768u); in.ch_rows_optional = true; }
  if (mv) { in.moves = mv; in.ch_rows_optional = true; }
  in.rack_keys = rack_keys != 0;
  if (in.rack_keys) in.ch_rows_optional = true;
  if (racks) {
    in.racks = true; in.report_rack = report_rack; in.racks_cap = lens[5];
    in.have_rk_racks = !(missing & 65536u); in.have_rk_scenarios = !(missing & 131072u); in.have_rk_off = !(missing & 262144u);
  }
  in.topic_keys = topic_keys != 0;
  if (topics) {
    in.topics = true; in.have_tp_tables = true;
    in.have_tp_topics = !(missing & 524288u); in.have_tp_scenarios = !(missing & 1048576u);
  }
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  const int64_t S = hc.batch.n_scenarios;
  const int64_t h[11] = {hc.ch_rows_need, hc.ch_nodes_need, hc.ch_chunks, (int64_t)hc.ch_head.bytes, hc.ch_gather_rows, hc.K, hc.native16, hc.mv_n,
                         racks ? hc.rack.rack_off[(size_t)S] : 0, racks ? hc.rack.r_max : 0, hc.tp_region_ints};
  memcpy(head, h, sizeof(h));
  for (int i = 0; i < KAS_HB_EVERY; ++i) bytes[i] = (int64_t)hc.bytes[i];
  return rc;
}

// every buffer of a host call
extern "C" __attribute__((visibility("default")))
int kas_emu_topic_choose_buffers(void) { return KAS_HB_EVERY; }
