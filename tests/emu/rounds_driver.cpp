// tests/emu/rounds_driver.cpp — runs the kernel body of the rounds pass (csrc/kas_rounds_body.h) on CPU fibers, and exports the
// host call planner with the rounds arguments.  TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp,
// which provides the fiber scheduler.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_rounds_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

namespace {

struct BlockArgs { const KasRoundsLaunch* a; int32_t block; int32_t wc; unsigned char* lds; };

template <bool C16>
void run_w(const BlockArgs& r) {
  if (r.wc <= 3) kasr::rounds_scenario<3, C16>(*r.a, r.block, r.lds);
  else if (r.wc <= 5) kasr::rounds_scenario<5, C16>(*r.a, r.block, r.lds);
  else kasr::rounds_scenario<8, C16>(*r.a, r.block, r.lds);
}
void run_block_fn(void* p) { const BlockArgs& r = *(BlockArgs*)p; if (r.a->src16) run_w<true>(r); else run_w<false>(r); }

int bad(char* errbuf, int errlen, const char* what, int64_t i) {
  if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %lld", what, (long long)i);
  return -100;
}

constexpr int GUARD = 1024;   // bytes behind the kernel's LDS

}  // namespace

// The rounds pass over the tables a solve left, as kas_solve_host_rounds runs it: one workgroup per listed scenario, each with
// exactly the LDS the product launches the kernel with, full of `lds_fill` (LDS is uninitialised on hardware) and a guard behind
// it.  cells16: cur / out are uint16 node indices (b->node_id is then not read).  select: n_select entries, or NULL with
// n_select < 0: every scenario.  out: host arrays.  info (may be NULL) <- LDS bytes, n_cap, the width class, the wave collectives
// the workgroups ran through (a walk of a scenario's tables takes the same number whatever the caps: how often it was walked).
// Returns 0, -100 on divergence / deadlock / a write beyond the LDS, or the refusal's code with its text.
extern "C" __attribute__((visibility("default")))
int kas_emu_rounds(const kas_batch_desc* b, const kas_tables* t, int cells16, const int32_t* select, int32_t n_select,
                   const kas_round_spec* spec, const kas_rounds* out, uint32_t lds_fill, int32_t* info, char* errbuf, int errlen) {
  auto refuse = [&](int code, const char* text) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", text);
    return code;
  };
  const int64_t n = n_select < 0 ? b->n_scenarios : n_select;
  int code = KAS_E_OK;
  int32_t n_cap = 0;
  KasMovesPlan mp;
  kas_moves_plan_build(b, &mp);
  const char* refusal = kas_rounds_list_error(b, n_select < 0 ? nullptr : select, n, spec, out, &code, &n_cap, &mp);
  if (refusal[0]) return refuse(code, refusal);
  int32_t wc = 1;
  for (int32_t i = 0; i < b->n_topics; ++i) {
    if (b->topics[i].cur_width > wc) wc = b->topics[i].cur_width;
    if (b->topics[i].out_width > wc) wc = b->topics[i].out_width;
  }
  const int32_t W = wc <= 3 ? 3 : (wc <= 5 ? 5 : 8);
  mp.scen.push_back(KasMovesScen{});                   // (one spare entry each: data() of an empty batch's tables is not NULL)
  mp.segs.push_back(KasMovesSeg{});
  std::vector<int32_t> sel;
  for (int64_t j = 0; j < n; ++j) sel.push_back(n_select < 0 ? (int32_t)j : select[j]);
  sel.push_back(0);
  KasRoundsLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = mp.scen.data(); a.segs = mp.segs.data(); a.sdesc = b->scenarios; a.node_id = b->node_id;
  a.select = sel.data();
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.scenarios = out->scenarios; a.rounds = out->rounds; a.round_of = out->round_of;
  a.round_stride = out->round_stride; a.move_stride = out->move_stride; a.spec = *spec;
  a.n = (int32_t)n; a.S = b->n_scenarios; a.n_cap = n_cap; a.src16 = cells16 ? 1 : 0;
  a.lds = kas_rounds_lds(n_cap, W, a.src16);
  if (info) { info[0] = a.lds.total; info[1] = n_cap; info[2] = W; info[3] = 0; }
  const long collectives0 = kasw::g_emu.collectives;
  if (a.lds.total > KAS_ROUND_LDS_LIMIT) return bad(errbuf, errlen, "the layout exceeds the LDS", -1);
  const size_t bytes = (size_t)a.lds.total;
  std::vector<unsigned char> lds(bytes + GUARD);
  for (int64_t j = 0; j < n; ++j) {
    for (size_t k = 0; k + 4 <= bytes; k += 4) memcpy(lds.data() + k, &lds_fill, 4);
    memset(lds.data() + bytes, 0xA5, GUARD);
    BlockArgs r{&a, (int32_t)j, wc, lds.data()};
    if (kasw::run_block(run_block_fn, &r, KAS_ROUND_BLOCK / 64) != 0) return bad(errbuf, errlen, "rounds kernel: divergence / deadlock", j);
    for (int k = 0; k < GUARD; ++k)
      if (lds[bytes + (size_t)k] != 0xA5) return bad(errbuf, errlen, "LDS written beyond the kernel's bytes", j);
  }
  if (info) info[3] = (int32_t)(kasw::g_emu.collectives - collectives0);
  return 0;
}

// kas_plan_host_call for a kas_solve_host_rounds / 16 call (kind 2), a kas_solve_host_batches / 16 call (kind 1: spec / out are a
// kas_batch_spec / kas_batches) or a plain kas_solve_host_select / 16 call (kind 0: select / n_select are then its row
// selection).  lens: cur, out, aux, ctx lengths.  head [4] <- listed, n_cap, K, native16;  bytes [KAS_HB_BUFFERS]
extern "C" __attribute__((visibility("default")))
int kas_emu_rounds_host_call(const kas_batch_desc* b, const int64_t* lens, int cells16, int kind, const int32_t* select, int32_t n_select,
                             const void* spec, const void* out, int ranges_override, int64_t* head, int64_t* bytes, char* errbuf,
                             int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.ranges_override = ranges_override;
  in.cur_len = lens[0]; in.out_len = lens[1]; in.aux_len = lens[2]; in.ctx_len = lens[3];
  in.have_cur = in.have_out = in.have_aux = in.have_ctx = in.have_topic_results = in.have_scenario_results = true;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  if (kind == 2) {
    in.select = nullptr; in.n_select = 0;
    in.rounds = (const kas_round_spec*)spec; in.rd_out = (const kas_rounds*)out; in.rd_select = select; in.rd_n_select = n_select;
  } else if (kind == 1) {
    in.select = nullptr; in.n_select = 0;
    in.batches = (const kas_batch_spec*)spec; in.bt_out = (const kas_batches*)out; in.bt_select = select; in.bt_n_select = n_select;
  } else {
    in.select = select; in.n_select = n_select;
  }
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  head[0] = kind == 2 ? hc.rd_n : hc.bt_n; head[1] = kind == 2 ? hc.rd_n_cap : hc.bt_n_cap; head[2] = hc.K; head[3] = hc.native16;
  for (int i = 0; i < KAS_HB_BUFFERS; ++i) bytes[i] = (int64_t)hc.bytes[i];
  return rc;
}

// [0] KAS_HB_BUFFERS, [1] KAS_HB_FINAL, [2] KAS_ROUND_WINDOW, [3] KAS_MOVES_ITEM_ROWS, [4] KAS_ROUND_NODE_LIMIT, [5] KAS_ROUND_QUEUE,
// [6 .. 8] KAS_HB_RD_SCEN, _ROUNDS, _OF, [9 .. 11] KAS_HB_BT_SDESC, _NODE_ID, _SELECT, [12] KAS_HB_MV_SCEN, [13] KAS_HB_MV_SEGS
extern "C" __attribute__((visibility("default")))
int kas_emu_rounds_const(int which) {
  const int v[] = {KAS_HB_BUFFERS, KAS_HB_FINAL, KAS_ROUND_WINDOW, KAS_MOVES_ITEM_ROWS, KAS_ROUND_NODE_LIMIT, KAS_ROUND_QUEUE,
                   KAS_HB_RD_SCEN, KAS_HB_RD_ROUNDS, KAS_HB_RD_OF, KAS_HB_BT_SDESC, KAS_HB_BT_NODE_ID, KAS_HB_BT_SELECT,
                   KAS_HB_MV_SCEN, KAS_HB_MV_SEGS};
  return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}

// the LDS layout (kas_rounds.h): out[6] <- off_look, off_misc, off_qn, off_qtp, off_win, total
extern "C" __attribute__((visibility("default")))
void kas_emu_rounds_lds(int32_t n_cap, int32_t W, int32_t cells16, int32_t* out) {
  const KasRoundsLds L = kas_rounds_lds(n_cap, W, cells16);
  out[0] = L.off_look; out[1] = L.off_misc; out[2] = L.off_qn; out[3] = L.off_qtp; out[4] = L.off_win; out[5] = L.total;
}
