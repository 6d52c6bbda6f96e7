// tests/emu/choose_driver.cpp — runs the rank and gather kernels' device code (csrc/kas_choose_body.h) on CPU fibers, and exports
// the host call planner with the choose arguments.  TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp,
// which provides the fiber scheduler.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_choose_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

namespace {

struct BlockArgs { const KasChooseLaunch* a; int64_t i; unsigned char* lds; };

void run_rank(void* p) {
  BlockArgs* r = (BlockArgs*)p;
  kasc::rank_block(*r->a, (int32_t)r->i, (kasc::Entry*)r->lds);
}
void run_gather(void* p) {
  BlockArgs* r = (BlockArgs*)p;
  kasc::gather_item(*r->a, r->i);
}

int bad(char* errbuf, int errlen, const char* what, int64_t i) {
  if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %lld", what, (long long)i);
  return -100;
}

// every workgroup of the rank kernel, as kas_rank_launch's grid: the LDS tile full of `lds_fill`, a guard behind it
int rank_all(const KasChooseLaunch& a, uint32_t lds_fill, char* errbuf, int errlen) {
  const size_t bytes = sizeof(kasc::Entry) * KAS_CHOOSE_TILE;
  std::vector<unsigned char> lds(bytes + 4096);
  const int64_t grid = ((int64_t)a.S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK;
  for (int64_t i = 0; i < grid; ++i) {
    for (size_t k = 0; k + 4 <= bytes; k += 4) memcpy(lds.data() + k, &lds_fill, 4);   // LDS is uninitialised on hardware too
    memset(lds.data() + bytes, 0xA5, 4096);
    BlockArgs r{&a, i, lds.data()};
    if (kasw::run_block(run_rank, &r, KAS_CHOOSE_BLOCK / 64) != 0) return bad(errbuf, errlen, "rank kernel: divergence / deadlock", i);
    for (size_t k = 0; k < 4096; ++k)
      if (lds[bytes + k] != 0xA5) return bad(errbuf, errlen, "rank kernel: LDS written beyond the tile", i);
  }
  return 0;
}

int gather_all(const KasChooseLaunch& a, char* errbuf, int errlen) {
  const int64_t grid = (int64_t)a.k * a.chunks;
  for (int64_t i = 0; i < grid; ++i) {
    BlockArgs r{&a, i, nullptr};
    if (kasw::run_block(run_gather, &r, KAS_CHOOSE_BLOCK / 64) != 0) return bad(errbuf, errlen, "gather kernel: divergence / deadlock", i);
  }
  return 0;
}

}  // namespace

// The rank kernel over S records.  cells / n_nodes ([S], both or neither): the size table's columns — with them row_off and
// node_off ([k + 1]) are written, without them only rank, chosen and n_ok (kas_rank_device).  Returns 0, -100 on divergence /
// deadlock / an LDS write beyond the tile, or KAS_E_INVALID_ARG with the spec's refusal.
extern "C" __attribute__((visibility("default")))
int kas_emu_rank(const kas_scenario_result* sr, const kas_scenario_impact* si, int32_t S, const kas_choose_spec* spec, const int64_t* cells,
                 const int32_t* n_nodes, int32_t* rank, int32_t* chosen, int64_t* row_off, int64_t* node_off, int32_t* n_ok,
                 uint32_t lds_fill, char* errbuf, int errlen) {
  const char* refusal = kas_choose_spec_error(spec, S);
  if (refusal[0]) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", refusal);
    return KAS_E_INVALID_ARG;
  }
  std::vector<KasChooseSize> sizes;
  if (cells && n_nodes) {
    sizes.assign((size_t)S + 1, KasChooseSize{});
    for (int32_t s = 0; s < S; ++s) { sizes[(size_t)s].cells = cells[s]; sizes[(size_t)s].n_nodes = n_nodes[s]; }
  }
  KasChooseLaunch a;
  memset(&a, 0, sizeof(a));
  a.sr = sr; a.si = si;
  a.sizes = sizes.empty() ? nullptr : sizes.data();
  kas_choose_fill_spec(&a, spec, S);
  a.rank = rank; a.chosen = chosen; a.row_off = row_off; a.node_off = node_off; a.n_ok = n_ok;
  return rank_all(a, lds_fill, errbuf, errlen);
}

// Rank and gather over the tables a solve and its impact pass left, as kas_choose_device does: t->out and t->scenario_results,
// imp->nodes and imp->scenarios, into ch.  cells: 0 = int32 cells, 1 = 16-bit cells, 2 = int32 cells in `out` gathered into
// 16-bit rows (the widened 16-bit host call).
extern "C" __attribute__((visibility("default")))
int kas_emu_choose(const kas_batch_desc* b, const kas_tables* t, const kas_impact_tables* imp, int cells, const kas_choose_spec* spec,
                   const kas_choice* ch, uint32_t lds_fill, char* errbuf, int errlen) {
  const char* refusal = kas_choose_spec_error(spec, b->n_scenarios);
  if (refusal[0]) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", refusal);
    return KAS_E_INVALID_ARG;
  }
  KasChoosePlan cp;
  kas_choose_plan_build(b, &cp);
  const int64_t chunks = kas_choose_chunks(cp, cells == 0 ? 4 : 2);
  cp.sizes.push_back(KasChooseSize{});                 // (one spare entry each: data() of an empty batch's tables is not NULL)
  cp.segs.push_back(KasChooseSeg{});
  KasChooseLaunch a;
  memset(&a, 0, sizeof(a));
  a.sr = t->scenario_results; a.si = imp->scenarios;
  a.sizes = cp.sizes.data(); a.segs = cp.segs.data();
  kas_choose_fill_spec(&a, spec, b->n_scenarios);
  a.rank = ch->rank; a.chosen = ch->chosen; a.row_off = ch->row_off; a.node_off = ch->node_off; a.n_ok = ch->n_ok;
  a.out = t->out; a.src_nodes = imp->nodes; a.rows = ch->rows; a.nodes = ch->nodes;
  a.src_cell = cells == 1 ? 2 : 4; a.dst_cell = cells == 0 ? 4 : 2;
  a.chunks = (int32_t)chunks;
  int rc = rank_all(a, lds_fill, errbuf, errlen);
  if (rc == 0) rc = gather_all(a, errbuf, errlen);
  return rc;
}

// kas_plan_host_call for a kas_solve_host_choose / 16 call.  lens: cur, aux, ctx lengths, rows_cap, nodes_cap.  missing: bits of
// the tables that are NULL — 1 cur, 4 aux, 8 ctx, 16 topic_results, 32 scenario_results, 128 impact scenarios, then the
// kas_choice arrays: 256 rank, 512 chosen, 1024 row_off, 2048 node_off, 4096 n_ok, 8192 rows, 16384 nodes.
// head [8] <- rows needed, node records needed, gather workgroups per chosen, header bytes, segments, K, native16, S
// bytes [KAS_HB_TOTAL]; sizes [S] x (cells, node_base, n_nodes, seg_begin, seg_count); segs [segments] x (out_off, cells, packed_at)
extern "C" __attribute__((visibility("default")))
int kas_emu_choose_host_call(const kas_batch_desc* b, const int64_t* lens, unsigned missing, int cells16, const kas_choose_spec* spec,
                             int64_t* head, int64_t* bytes, int64_t* sizes, int64_t* segs, int64_t segs_cap, char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.cur_len = lens[0]; in.out_len = 0; in.aux_len = lens[1]; in.ctx_len = lens[2];
  in.have_cur = !(missing & 1u); in.have_out = false; in.have_aux = !(missing & 4u); in.have_ctx = !(missing & 8u);
  in.have_topic_results = !(missing & 16u); in.have_scenario_results = !(missing & 32u);
  in.select = nullptr; in.n_select = 0;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  in.impact = true; in.have_imp_nodes = false; in.have_imp_scenarios = !(missing & 128u);
  in.choose = spec; in.rows_cap = lens[3]; in.nodes_cap = lens[4];
  in.have_ch_rank = !(missing & 256u); in.have_ch_chosen = !(missing & 512u); in.have_ch_row_off = !(missing & 1024u);
  in.have_ch_node_off = !(missing & 2048u); in.have_ch_n_ok = !(missing & 4096u);
  in.have_ch_rows = !(missing & 8192u); in.have_ch_nodes = !(missing & 16384u);
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  const int64_t h[8] = {hc.ch_rows_need, hc.ch_nodes_need, hc.ch_chunks, (int64_t)hc.ch_head.bytes, (int64_t)hc.choose.segs.size(),
                        hc.K, hc.native16, b->n_scenarios};
  memcpy(head, h, sizeof(h));
  for (int i = 0; i < KAS_HB_TOTAL; ++i) bytes[i] = (int64_t)hc.bytes[i];
  for (size_t s = 0; s < hc.choose.sizes.size(); ++s) {
    const KasChooseSize& z = hc.choose.sizes[s];
    const int64_t row[5] = {z.cells, z.node_base, z.n_nodes, z.seg_begin, z.seg_count};
    memcpy(sizes + 5 * s, row, sizeof(row));
  }
  for (size_t g = 0; g < hc.choose.segs.size() && (int64_t)g < segs_cap; ++g) {
    const KasChooseSeg& sg = hc.choose.segs[g];
    const int64_t row[3] = {sg.out_off, sg.cells, sg.packed_at};
    memcpy(segs + 3 * g, row, sizeof(row));
  }
  return rc;
}

extern "C" __attribute__((visibility("default")))
int kas_emu_choose_buffers(void) { return KAS_HB_TOTAL; }
