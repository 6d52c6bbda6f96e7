// tests/emu/batches_driver.cpp — runs the kernel body of the batches pass (csrc/kas_batches_body.h) on CPU fibers, and exports the
// host call planner with the batches arguments.  TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp,
// which provides the fiber scheduler.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_batches_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

namespace {

struct BlockArgs { const KasBatchesLaunch* a; int32_t block; int32_t wc; unsigned char* lds; };

template <bool C16>
void run_w(const BlockArgs& r) {
  if (r.wc <= 3) kasb::batches_scenario<3, C16>(*r.a, r.block, r.lds);
  else if (r.wc <= 5) kasb::batches_scenario<5, C16>(*r.a, r.block, r.lds);
  else kasb::batches_scenario<8, C16>(*r.a, r.block, r.lds);
}
void run_block_fn(void* p) { const BlockArgs& r = *(BlockArgs*)p; if (r.a->src16) run_w<true>(r); else run_w<false>(r); }

int bad(char* errbuf, int errlen, const char* what, int64_t i) {
  if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %lld", what, (long long)i);
  return -100;
}

constexpr int GUARD = 1024;   // bytes behind the kernel's LDS

}  // namespace

// The batches pass over the tables a solve left, as kas_solve_host_batches runs it: one workgroup per listed scenario, each with
// exactly the LDS the product launches the kernel with, full of `lds_fill` (LDS is uninitialised on hardware: it holds what the
// workgroup before left there) and a guard behind it.  cells16: cur / out are uint16 node indices (b->node_id is then not read).
// select: n_select entries, or NULL with n_select < 0: every scenario.  out: host arrays.  info (may be NULL) <- LDS bytes,
// n_cap, the width class, the wave collectives the workgroups ran through (a replayed group adds its moves' ballots: whether a
// group was replayed, which the records do not show).  Returns 0, -100 on divergence / deadlock / a write beyond the LDS, or the refusal's code with its text.
extern "C" __attribute__((visibility("default")))
int kas_emu_batches(const kas_batch_desc* b, const kas_tables* t, int cells16, const int32_t* select, int32_t n_select,
                    const kas_batch_spec* spec, const kas_batches* out, uint32_t lds_fill, int32_t* info, char* errbuf, int errlen) {
  auto refuse = [&](int code, const char* text) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", text);
    return code;
  };
  const int64_t n = n_select < 0 ? b->n_scenarios : n_select;
  int code = KAS_E_OK;
  int32_t n_cap = 0;
  const char* refusal = kas_batches_list_error(b, n_select < 0 ? nullptr : select, n, spec, out, &code, &n_cap);
  if (refusal[0]) return refuse(code, refusal);
  KasMovesPlan mp;
  kas_moves_plan_build(b, &mp);
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
  KasBatchesLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = mp.scen.data(); a.segs = mp.segs.data(); a.sdesc = b->scenarios; a.node_id = b->node_id;
  a.select = sel.data();
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.scenarios = out->scenarios; a.batches = out->batches; a.stride = out->stride; a.spec = *spec;
  a.n = (int32_t)n; a.S = b->n_scenarios; a.n_cap = n_cap; a.src16 = cells16 ? 1 : 0;
  a.lds = kas_batches_lds(n_cap, W, a.src16);
  if (info) { info[0] = a.lds.total; info[1] = n_cap; info[2] = W; info[3] = 0; }
  const long collectives0 = kasw::g_emu.collectives;
  if (a.lds.total > KAS_BATCH_LDS_LIMIT) return bad(errbuf, errlen, "the layout exceeds the LDS", -1);
  const size_t bytes = (size_t)a.lds.total;
  std::vector<unsigned char> lds(bytes + GUARD);
  for (int64_t j = 0; j < n; ++j) {
    for (size_t k = 0; k + 4 <= bytes; k += 4) memcpy(lds.data() + k, &lds_fill, 4);
    memset(lds.data() + bytes, 0xA5, GUARD);
    BlockArgs r{&a, (int32_t)j, wc, lds.data()};
    if (kasw::run_block(run_block_fn, &r, KAS_BATCH_BLOCK / 64) != 0) return bad(errbuf, errlen, "batches kernel: divergence / deadlock", j);
    for (int k = 0; k < GUARD; ++k)
      if (lds[bytes + (size_t)k] != 0xA5) return bad(errbuf, errlen, "LDS written beyond the kernel's bytes", j);
  }
  if (info) info[3] = (int32_t)(kasw::g_emu.collectives - collectives0);
  return 0;
}

// kas_plan_host_call for a kas_solve_host_batches / 16 call (spec != NULL) or a plain kas_solve_host_select / 16 call (spec ==
// NULL: select / n_select are then its row selection).  lens: cur, out, aux, ctx lengths.
// head [4] <- listed, n_cap, K, native16;  bytes [KAS_HB_FINAL]
extern "C" __attribute__((visibility("default")))
int kas_emu_batches_host_call(const kas_batch_desc* b, const int64_t* lens, int cells16, const int32_t* select, int32_t n_select,
                              const kas_batch_spec* spec, const kas_batches* out, int ranges_override, int64_t* head, int64_t* bytes,
                              char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.ranges_override = ranges_override;
  in.cur_len = lens[0]; in.out_len = lens[1]; in.aux_len = lens[2]; in.ctx_len = lens[3];
  in.have_cur = in.have_out = in.have_aux = in.have_ctx = in.have_topic_results = in.have_scenario_results = true;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  if (spec || out) {
    in.select = nullptr; in.n_select = 0;
    in.batches = spec; in.bt_out = out; in.bt_select = select; in.bt_n_select = n_select;
  } else {
    in.select = select; in.n_select = n_select;
  }
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  head[0] = hc.bt_n; head[1] = hc.bt_n_cap; head[2] = hc.K; head[3] = hc.native16;
  for (int i = 0; i < KAS_HB_FINAL; ++i) bytes[i] = (int64_t)hc.bytes[i];
  return rc;
}

// [0] KAS_HB_FINAL, [1] KAS_HB_EVERY, [2] KAS_BATCH_GROUP, [3] KAS_MOVES_ITEM_ROWS, [4] KAS_BATCH_NODE_LIMIT, [5] KAS_BATCH_QUEUE,
// [6 .. 10] KAS_HB_BT_SDESC, _NODE_ID, _SELECT, _SCEN, _BATCHES, [11] KAS_HB_MV_SCEN, [12] KAS_HB_MV_SEGS
extern "C" __attribute__((visibility("default")))
int kas_emu_batches_const(int which) {
  const int v[] = {KAS_HB_FINAL, KAS_HB_EVERY, KAS_BATCH_GROUP, KAS_MOVES_ITEM_ROWS, KAS_BATCH_NODE_LIMIT, KAS_BATCH_QUEUE,
                   KAS_HB_BT_SDESC, KAS_HB_BT_NODE_ID, KAS_HB_BT_SELECT, KAS_HB_BT_SCEN, KAS_HB_BT_BATCHES, KAS_HB_MV_SCEN, KAS_HB_MV_SEGS};
  return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}

// the LDS layout (kas_batches.h): out[5] <- off_look, off_misc, off_qn, off_qtp, total
extern "C" __attribute__((visibility("default")))
void kas_emu_batches_lds(int32_t n_cap, int32_t W, int32_t cells16, int32_t* out) {
  const KasBatchesLds L = kas_batches_lds(n_cap, W, cells16);
  out[0] = L.off_look; out[1] = L.off_misc; out[2] = L.off_qn; out[3] = L.off_qtp; out[4] = L.total;
}
