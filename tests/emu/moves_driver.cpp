// tests/emu/moves_driver.cpp — runs the three kernel bodies of the moves pass (csrc/kas_moves_body.h) on CPU fibers, and exports
// the host call planner with the moves arguments.  TEST INFRASTRUCTURE: see tests/emu/kas_wave.h; linked with emu_driver.cpp,
// which provides the fiber scheduler.
#include <string.h>

#include <string>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_moves_body.h"
#include "kas_solver_body.h"
#include "kas_host_call.h"

namespace {

struct BlockArgs { const KasMovesLaunch* a; int32_t block; int32_t wc; int32_t* lds; };

template <bool C16>
void count_w(const BlockArgs& r) {
  if (r.wc <= 3) kasm::count_item<3, C16>(*r.a, r.block, r.lds);
  else if (r.wc <= 5) kasm::count_item<5, C16>(*r.a, r.block, r.lds);
  else kasm::count_item<8, C16>(*r.a, r.block, r.lds);
}
template <bool C16>
void emit_w(const BlockArgs& r) {
  if (r.wc <= 3) kasm::emit_item<3, C16>(*r.a, r.block, r.lds);
  else if (r.wc <= 5) kasm::emit_item<5, C16>(*r.a, r.block, r.lds);
  else kasm::emit_item<8, C16>(*r.a, r.block, r.lds);
}
void run_count(void* p) { const BlockArgs& r = *(BlockArgs*)p; if (r.a->src16) count_w<true>(r); else count_w<false>(r); }
void run_emit(void* p) { const BlockArgs& r = *(BlockArgs*)p; if (r.a->src16) emit_w<true>(r); else emit_w<false>(r); }
void run_scan(void* p) { const BlockArgs& r = *(BlockArgs*)p; kasm::scan_all(*r.a, r.lds); }

int bad(char* errbuf, int errlen, const char* what, int64_t i) {
  if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s, workgroup %lld", what, (long long)i);
  return -100;
}

constexpr int GUARD = 256;   // int32 words behind a kernel's LDS

// one workgroup with `words` int32 of LDS full of `lds_fill` (LDS is uninitialised on hardware too) and a guard behind them
int run_one(void (*fn)(void*), const KasMovesLaunch& a, int32_t block, int32_t wc, int words, uint32_t lds_fill, const char* what,
            char* errbuf, int errlen) {
  std::vector<int32_t> lds((size_t)words + GUARD);
  for (int k = 0; k < words; ++k) lds[(size_t)k] = (int32_t)lds_fill;
  for (int k = 0; k < GUARD; ++k) lds[(size_t)words + k] = (int32_t)0xA5A5A5A5;
  BlockArgs r{&a, block, wc, lds.data()};
  if (kasw::run_block(fn, &r, KAS_MOVES_BLOCK / 64) != 0) return bad(errbuf, errlen, what, block);
  for (int k = 0; k < GUARD; ++k)
    if (lds[(size_t)words + k] != (int32_t)0xA5A5A5A5) return bad(errbuf, errlen, "LDS written beyond the kernel's words", block);
  return 0;
}

}  // namespace

// The moves pass over the tables a solve left, as kas_moves_device runs it: count, scan, emit.  cells: 0 = int32 cells, 1 = 16-bit
// cells, 2 = int32 cells in cur / out written as 16-bit list cells (the widened 16-bit host call).  select: n_select entries.
// The scratch table is pre-filled with a pattern and has a guard entry behind it.  Returns 0, -100 on divergence / deadlock / a
// write beyond the LDS or the scratch, or KAS_E_INVALID_ARG / KAS_E_UNSUPPORTED with the refusal's text.
extern "C" __attribute__((visibility("default")))
int kas_emu_moves(const kas_batch_desc* b, const kas_tables* t, int cells, const int32_t* select, int32_t n_select, const kas_moves* mv,
                  uint32_t lds_fill, char* errbuf, int errlen) {
  auto refuse = [&](int code, const char* text) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "%s", text);
    return code;
  };
  const char* refusal = kas_moves_args_error(mv, cells == 0 ? 4 : 2);
  if (refusal[0]) return refuse(KAS_E_INVALID_ARG, refusal);
  KasMovesPlan mp;
  kas_moves_plan_build(b, &mp);
  refusal = kas_moves_shape_error(mp, n_select);
  if (refusal[0]) return refuse(KAS_E_UNSUPPORTED, refusal);
  int32_t wc = 1;
  for (int32_t i = 0; i < b->n_topics; ++i) {
    if (b->topics[i].cur_width > wc) wc = b->topics[i].cur_width;
    if (b->topics[i].out_width > wc) wc = b->topics[i].out_width;
  }
  mp.scen.push_back(KasMovesScen{});                   // (one spare entry each: data() of an empty batch's tables is not NULL)
  mp.segs.push_back(KasMovesSeg{});
  const size_t entries = (size_t)n_select * (size_t)mp.max_items;
  std::vector<KasMovesCount> scratch(entries + 1);
  memset(scratch.data(), 0x7B, sizeof(KasMovesCount) * (entries + 1));
  std::vector<int32_t> sel(select, select + n_select);
  sel.push_back(0);
  KasMovesLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = mp.scen.data(); a.segs = mp.segs.data(); a.select = sel.data();
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.scratch = scratch.data();
  a.move_off = mv->move_off; a.cell_off = mv->cell_off; a.moves = mv->moves; a.cells = mv->cells;
  a.moves_cap = mv->moves_cap; a.cells_cap = mv->cells_cap;
  a.n = n_select; a.stride = mp.max_items; a.S = b->n_scenarios; a.mask = mv->mask;
  a.src16 = cells == 1; a.dst16 = cells != 0;
  const int64_t grid = (int64_t)a.n * a.stride;
  int rc = 0;
  for (int64_t i = 0; i < grid && rc == 0; ++i)
    rc = run_one(run_count, a, (int32_t)i, wc, 2 * kasm::WAVES, lds_fill, "count kernel: divergence / deadlock", errbuf, errlen);
  if (rc == 0) rc = run_one(run_scan, a, 0, wc, 2 * kasm::WAVES, lds_fill, "scan kernel: divergence / deadlock", errbuf, errlen);
  for (int64_t i = 0; i < grid && rc == 0 && (a.moves_cap > 0 || a.cells_cap > 0); ++i)
    rc = run_one(run_emit, a, (int32_t)i, wc, 2 * kasm::GROUPS, lds_fill, "emit kernel: divergence / deadlock", errbuf, errlen);
  if (rc != 0) return rc;
  const unsigned char* g = (const unsigned char*)&scratch[entries];
  for (size_t k = 0; k < sizeof(KasMovesCount); ++k)
    if (g[k] != 0x7B) return bad(errbuf, errlen, "the scratch table was written beyond n x stride", -1);
  return 0;
}

// the room helpers (kas_moves.h): out[0..1] <- rows, cells of the list (select == NULL: every scenario); out[2..3] <- of the k largest
extern "C" __attribute__((visibility("default")))
void kas_emu_moves_room(const kas_batch_desc* b, const int32_t* select, int32_t n_select, int32_t k, int64_t* out) {
  KasMovesPlan mp;
  kas_moves_plan_build(b, &mp);
  kas_moves_room(mp, select, n_select, &out[0], &out[1]);
  kas_moves_k_largest(mp, k, &out[2], &out[3]);
  out[4] = mp.max_items;
}

// kas_plan_host_call for a kas_solve_host_moves / 16 call (spec == NULL: the list is select / n_select, < 0 every scenario) or a
// kas_solve_host_choose_moves / 16 call (spec: its list is the choice's).  lens: cur, aux, ctx lengths, rows_cap, nodes_cap.
// missing: bits of what is NULL — 1 cur, 4 aux, 8 ctx, 16 topic_results, 32 scenario_results, 128 impact scenarios, 8192 the choice's
// rows (its other arrays are there); the kas_moves arrays are mv's own.
// head [12] <- listed, room moves, room cells, device moves cap, device cells cap, K, launch stride, rows gathered, rows needed,
//              scenarios of the moves table, segments of it, native16;  bytes [KAS_HB_ALL]
// ranges_override: what the library reads from KAS_HOST_RANGES and passes in (0: not set)
extern "C" __attribute__((visibility("default")))
int kas_emu_moves_host_call(const kas_batch_desc* b, const int64_t* lens, unsigned missing, int cells16, const kas_choose_spec* spec,
                            const int32_t* select, int32_t n_select, const kas_moves* mv, int ranges_override, int64_t* head,
                            int64_t* bytes, char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.ranges_override = ranges_override;
  in.cur_len = lens[0]; in.out_len = 0; in.aux_len = lens[1]; in.ctx_len = lens[2];
  in.have_cur = !(missing & 1u); in.have_out = false; in.have_aux = !(missing & 4u); in.have_ctx = !(missing & 8u);
  in.have_topic_results = !(missing & 16u); in.have_scenario_results = !(missing & 32u);
  in.select = nullptr; in.n_select = 0;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  if (spec) {
    in.impact = true; in.have_imp_nodes = false; in.have_imp_scenarios = !(missing & 128u);
    in.choose = spec; in.rows_cap = lens[3]; in.nodes_cap = lens[4];
    in.have_ch_rank = in.have_ch_chosen = in.have_ch_row_off = in.have_ch_node_off = in.have_ch_n_ok = in.have_ch_nodes = true;
    in.have_ch_rows = !(missing & 8192u);
    in.ch_rows_optional = true;
  } else {
    in.mv_select = select; in.mv_n_select = n_select;
  }
  in.moves = mv;
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  const int64_t h[12] = {hc.mv_n, hc.mv_room_moves, hc.mv_room_cells, hc.mv_moves_cap, hc.mv_cells_cap, hc.K, hc.moves.max_items,
                         hc.ch_gather_rows, hc.ch_rows_need, (int64_t)hc.moves.scen.size(), (int64_t)hc.moves.segs.size(), hc.native16};
  memcpy(head, h, sizeof(h));
  for (int i = 0; i < KAS_HB_ALL; ++i) bytes[i] = (int64_t)hc.bytes[i];
  return rc;
}

extern "C" __attribute__((visibility("default")))
int kas_emu_moves_buffers(void) { return KAS_HB_ALL; }

extern "C" __attribute__((visibility("default")))
int kas_emu_moves_item_rows(void) { return KAS_MOVES_ITEM_ROWS; }
