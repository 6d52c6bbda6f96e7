// tests/emu/emu_driver.cpp — runs the solver body (csrc/kas_solver_body.h) on CPU fibers.
// TEST INFRASTRUCTURE: see tests/emu/kas_wave.h.  Exposes kas_emu_solve_batch() with the
// semantics of kas_solve_host(), including the product's own planning code (kas_plan_math.h).
#include <string.h>

#include <string>
#include <cstdlib>
#include <vector>

#include "emu/kas_wave.h"     // defines KAS_WAVE_H_ first, so the body's own #include "kas_wave.h" is a no-op
#include "kas_solver_body.h"
#include "kas_launch_plan.h"   // the launch resolver the product shares: which kernels, grids, LDS and launch words
#include "kas_host_call.h"     // what a host call does, decided on the CPU: the planner the product's host path executes

namespace kasw {

Emu g_emu;
static const size_t STACK_BYTES = 192 * 1024;
static char* g_stacks = nullptr;

struct Tramp { void (*fn)(void*); void* arg; };
static Tramp g_tramp;

static void lane_entry() {
  g_tramp.fn(g_tramp.arg);
  g_emu.state[g_emu.cur] = S_DONE;
  kas_emu_switch(&g_emu.lane_ctx[g_emu.cur], &g_emu.main_ctx);
  abort();                                                   // a finished fiber is never resumed
}

#if KAS_EMU_FAST_SWITCH
// kas_emu_switch(from, to): push the callee-saved registers, park the stack pointer in *from, take
// *to's, pop, return into the other fiber.  (MXCSR / x87 control words are the process defaults in
// every fiber and nothing here changes them.)
asm(".text\n"
    ".globl kas_emu_switch\n"
    ".hidden kas_emu_switch\n"
    ".type kas_emu_switch,@function\n"
    "kas_emu_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n"
    "  movq (%rsi), %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n"
    "  ret\n"
    ".size kas_emu_switch, .-kas_emu_switch\n");

// a fresh fiber: six zeroed registers, then lane_entry as the address the first switch returns to,
// entered with the stack the ABI promises a function (rsp + 8 a multiple of 16)
static void make_fiber(Ctx* c, char* stack, size_t bytes) {
  uintptr_t top = ((uintptr_t)stack + bytes) & ~(uintptr_t)15;
  void** sp = (void**)(top - 64);
  for (int i = 0; i < 6; ++i) sp[i] = nullptr;
  sp[6] = (void*)&lane_entry;
  sp[7] = nullptr;
  c->sp = sp;
}
#else
static void make_fiber(Ctx* c, char* stack, size_t bytes) {
  getcontext(&c->uc);
  c->uc.uc_stack.ss_sp = stack;
  c->uc.uc_stack.ss_size = bytes;
  c->uc.uc_link = &g_emu.main_ctx.uc;
  makecontext(&c->uc, lane_entry, 0);
}
#endif

// KAS_EMU_CHAOS=<seed>: waves no longer advance in step.  Each round a wave whose lanes have all
// arrived at a collective is released only with probability 1/2 (never none of them), and now and
// then one wave is held back for a long stretch — relative wave speeds on hardware are arbitrary,
// and the protocols between waves (ring tags, P4 progress words) must not depend on them.
static uint64_t g_chaos = 0;
static uint32_t chaos_next() {
  g_chaos ^= g_chaos << 13; g_chaos ^= g_chaos >> 7; g_chaos ^= g_chaos << 17;
  return (uint32_t)(g_chaos >> 32);
}

long g_last_block_rounds = 0;   // scheduling rounds of the last run_block (KAS_EMU_STATS)

int run_block(void (*fn)(void*), void* arg, int n_waves) {
  Emu& e = g_emu;
  static int chaos_init = 0;
  if (!chaos_init) {
    chaos_init = 1;
    const char* c = getenv("KAS_EMU_CHAOS");
    if (c && *c) g_chaos = 0x9E3779B97F4A7C15ull * (uint64_t)(strtoull(c, nullptr, 10) + 1);
  }
  // KAS_EMU_WAVE_DIV="w:k[,w:k...]": wave w is released only every k-th scheduling round — a crude way
  // of making one wavefront the slow one (on hardware the class-1 solver of the wide order kernel is the
  // bottleneck and always has a full hand; with every wave at the same speed it is starved instead)
  static int wave_div[KAS_EMU_MAX_LANES / 64];
  static int div_init = 0;
  if (!div_init) {
    div_init = 1;
    for (int w = 0; w < KAS_EMU_MAX_LANES / 64; ++w) wave_div[w] = 1;
    const char* c = getenv("KAS_EMU_WAVE_DIV");
    while (c && *c) {
      char* end = nullptr;
      const long w = strtol(c, &end, 10);
      if (!end || *end != ':') break;
      const long k = strtol(end + 1, &end, 10);
      if (w >= 0 && w < KAS_EMU_MAX_LANES / 64 && k >= 1) wave_div[w] = (int)k;
      c = (*end == ',') ? end + 1 : nullptr;
    }
  }
  int held_wave = -1;
  long held_rounds = 0, rounds = 0;
  const int n = 64 * n_waves;
  if (n > KAS_EMU_MAX_LANES) return -1;
  if (!g_stacks) g_stacks = (char*)malloc((size_t)KAS_EMU_MAX_LANES * STACK_BYTES);
  g_tramp.fn = fn; g_tramp.arg = arg;
  e.n_lanes = n;
  for (int i = 0; i < n; ++i) {
    e.state[i] = S_RUNNABLE; e.kind[i] = K_NONE;
    make_fiber(&e.lane_ctx[i], g_stacks + (size_t)i * STACK_BYTES, STACK_BYTES);
  }
  for (;;) {
    // 1. run every runnable fiber until it parks at a collective or finishes
    int ran = 0, done = 0;
    for (int i = 0; i < n; ++i) {
      if (e.state[i] == S_DONE) { ++done; continue; }
      if (e.state[i] != S_RUNNABLE) continue;
      e.cur = i;
      kas_emu_switch(&e.main_ctx, &e.lane_ctx[i]);
      ++ran;
      if (e.state[i] == S_DONE) ++done;
    }
    if (done == n) { g_last_block_rounds = rounds; return 0; }
    // 2. release every wave whose 64 fibers all wait at the same wave collective; a workgroup
    //    barrier releases when every fiber of the block waits at it
    int released = 0, at_sync = 0, n_ready = 0;
    int ready_waves[KAS_EMU_MAX_LANES / 64];
    for (int w = 0; w < n_waves; ++w) {
      int parked = 0, finished = 0, k = -1;
      bool mixed = false;
      for (int i = 64 * w; i < 64 * w + 64; ++i) {
        if (e.state[i] == S_DONE) { ++finished; continue; }
        if (e.state[i] == S_PARKED) {
          ++parked;
          if (k < 0) k = e.kind[i]; else if (e.kind[i] != k) mixed = true;
        }
      }
      if (finished == 64) continue;
      if (parked + finished < 64) continue;                // cannot happen after step 1
      if (finished > 0) { fprintf(stderr, "emu: wave %d: %d lanes exited while others wait at a collective\n", w, finished); return -1; }
      if (mixed) {
        fprintf(stderr, "emu: wave %d: divergence, lanes wait at different collectives:", w);
        for (int i = 64 * w; i < 64 * w + 64; ++i) fprintf(stderr, " %d", e.kind[i]);
        fprintf(stderr, "\n");
        return -1;
      }
      if (k == K_SYNC) { at_sync += 64; continue; }
      ready_waves[n_ready++] = w;
    }
    if (n_ready > 0) {
      int first_released = -1;
      if (g_chaos != 0 && n_waves > 1) {
        if (held_rounds > 0) --held_rounds; else held_wave = -1;
        if (held_wave < 0 && (chaos_next() & 1023u) == 0) { held_wave = (int)(chaos_next() % (uint32_t)n_waves); held_rounds = 50 + (long)(chaos_next() % 2000u); }
      }
      for (int r = 0; r < n_ready; ++r) {
        const int w = ready_waves[r];
        bool go = true;
        if (g_chaos != 0 && n_waves > 1) go = w != held_wave && (chaos_next() & 1u) != 0;
        if (wave_div[w] > 1 && n_waves > 1 && (rounds % wave_div[w]) != 0) go = false;
        if (!go) continue;
        for (int i = 64 * w; i < 64 * w + 64; ++i) e.state[i] = S_RUNNABLE;
        ++released; e.collectives++;
        if (first_released < 0) first_released = w;
      }
      if (released == 0) {                                 // never stall everybody
        int w = ready_waves[chaos_next() % (uint32_t)n_ready];
        if (w == held_wave && n_ready > 1) w = ready_waves[(w == ready_waves[0]) ? 1 : 0];
        for (int i = 64 * w; i < 64 * w + 64; ++i) e.state[i] = S_RUNNABLE;
        ++released; e.collectives++;
      }
    }
    if (++rounds > 400000000L) { fprintf(stderr, "emu: no end in sight after %ld rounds (livelock?)\n", rounds); return -1; }
    if (at_sync == n) {
      for (int i = 0; i < n; ++i) e.state[i] = S_RUNNABLE;
      ++released;
    } else if (at_sync > 0 && at_sync == n - done && done > 0) {
      fprintf(stderr, "emu: some waves exited while others wait at the workgroup barrier\n");
      return -1;
    }
    if (released == 0 && ran == 0) { fprintf(stderr, "emu: deadlock (nothing runnable, nothing released)\n"); return -1; }
    if (released == 0) {
      // every live fiber is parked and no group is complete
      bool any_runnable = false;
      for (int i = 0; i < n; ++i) any_runnable = any_runnable || e.state[i] == S_RUNNABLE;
      if (!any_runnable) { fprintf(stderr, "emu: deadlock at a collective\n"); return -1; }
    }
  }
}

}  // namespace kasw

namespace {

struct RunArgs { const KasLaunch* a; int32_t s; unsigned char* lds; };

template <int W, int M32C = 0> void run_fill_slim(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::fill_scenario<W, 4, true, M32C>(*r->a, r->s, r->lds);
}
template <int W, int NW> void run_fill(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::fill_scenario<W, NW>(*r->a, r->s, r->lds);
}
template <int W, int M32C = 0> void run_p4(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::p4_scenario<W, 1, false, M32C>(*r->a, r->s, r->lds);   // (one wavefront, as kas_p4_kernel is launched; its instance per mid-row layout)
}
template <int W, int G, bool PK> void run_order_tickets(void* p) {
  RunArgs* r = (RunArgs*)p;
  if constexpr (W <= 3) kas::order_tickets<W, G, PK>(*r->a, r->s, r->lds);
}
void run_permutation(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::order_permutation(*r->a, r->lds);
}
template <int W> void run_order_relax_wide(void* p) {
  RunArgs* r = (RunArgs*)p;
  if constexpr (W == 4 || W == 5) kas::order_relax_wide<W>(*r->a, r->s, r->lds);
}
template <int W> void run_order_wide(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::order_tickets_wide<W>(*r->a, r->s, r->lds);
}
template <int W, bool DUAL, bool CTX, bool VERIFY = false, bool C16 = false, bool IDL = false> void run_order_relax(void* p) {
  RunArgs* r = (RunArgs*)p;
  if constexpr (W <= 3) kas::order_relax<W, DUAL, CTX, VERIFY, C16, IDL>(*r->a, r->s, r->lds);
}
template <int W, bool DUAL, bool C16, bool IDL, bool M32 = false, bool QUAD = false> void run_p4_order(void* p) {
  RunArgs* r = (RunArgs*)p;
  if constexpr (W <= 3) kas::p4_order_scenario<W, DUAL, C16, IDL, M32, QUAD>(*r->a, r->s, r->lds);
}
// the instances for dword mid rows (KAS_FLAG_MID32)
template <bool DUAL, bool QUAD = false> void run_order_relax_m32(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::order_relax<3, DUAL, false, false, false, true, false, true, QUAD>(*r->a, r->s, r->lds);
}
template <int W> void run_order_rounds(void* p) {
  RunArgs* r = (RunArgs*)p;
  kas::order_scenario_rounds<W>(*r->a, r->s, r->lds);
}

struct SpreadArgs { const KasLaunch* a; int32_t s, c; unsigned char* lds; };
template <int W> void run_spread_a(void* p) { SpreadArgs* r = (SpreadArgs*)p; kas::spread_pass_a<W>(*r->a, r->s, r->c, r->lds); }
template <int W> void run_spread_b(void* p) { SpreadArgs* r = (SpreadArgs*)p; kas::spread_pass_b<W>(*r->a, r->s, r->c, r->lds); }
template <int W> void run_spread_p4(void* p) { SpreadArgs* r = (SpreadArgs*)p; kas::spread_p4<W, KAS_SPREAD_P4_WAVES>(*r->a, r->s, r->lds); }
template <int W> void run_spread_quota(void* p) {
  const KasLaunch& a = *((SpreadArgs*)p)->a;
  for (int32_t s = 0; s < a.n_scenarios; ++s)
    for (int32_t n = 0; n < a.n_max; ++n) kas::spread_quota<W>(a, s, n);
}

// kas_fill_kernel as it is launched: workgroup `block` of `grid` runs kas::fill_block — its loop over the scenarios it takes (by index,
// or by rank among the flagged ones behind the slim kernel / the spread fill / the wide form's check), the LDS NOT cleared between them
struct BlockArgs { const KasLaunch* a; int32_t block, grid; unsigned char* lds; };
template <int W, int NW> void run_fill_block(void* p) {
  BlockArgs* r = (BlockArgs*)p;
  kas::fill_block<W, NW>(*r->a, r->block, r->grid, r->lds);
}
typedef void (*run_fn)(void*);
// relaxation form: the instance for (tiles, Context)
template <int W, bool VERIFY, bool C16, bool IDL> run_fn relax_instance(const KasKernelId& k) {
  if constexpr (W == 3)
    if (k.tiles == 1) return k.ctx ? run_order_relax<3, true, true, VERIFY, C16, IDL> : run_order_relax<3, true, false, VERIFY, C16, IDL>;
  if (k.tiles != 0) return nullptr;
  return k.ctx ? run_order_relax<W, false, true, VERIFY, C16, IDL> : run_order_relax<W, false, false, VERIFY, C16, IDL>;
}
template <int W, bool C16> run_fn p4_order_instance(const KasKernelId& k) {
  if constexpr (W == 3)
    if (k.tiles == 1) return run_p4_order<3, true, C16, !C16>;
  return k.tiles == 0 ? run_p4_order<W, false, C16, !C16> : nullptr;
}
// kernel identity (kas_launch_plan.h) -> the function a fiber runs; the same width classes and instances the product's mapping has
// (+ 8 fill wavefronts per scenario, which exist here only)
template <int W> run_fn emu_kernel_w(const KasKernelId& k) {
  switch (k.family) {
    case KAS_K_FILL:
      return k.NW == 1 ? run_fill_block<W, 1> : k.NW == 2 ? run_fill_block<W, 2> : k.NW == 4 ? run_fill_block<W, 4> : k.NW == 8 ? run_fill_block<W, 8> : nullptr;
    case KAS_K_FILL_SLIM:
      if constexpr (W == 3) if (k.m32) return run_fill_slim<3, 1>;
      if constexpr (W <= 3) if (!k.m32) return run_fill_slim<W>;
      return nullptr;
    case KAS_K_P4:
      if constexpr (W == 3) if (k.m32) return run_p4<3, 1>;
      return k.m32 ? nullptr : run_p4<W>;
    case KAS_K_ORDER_RELAX:
      if constexpr (W == 3)
        if (k.m32) {
          if (!k.idl || k.ctx || k.verify || k.c16) return nullptr;
          return k.tiles == 2 ? run_order_relax_m32<true, true> : k.tiles == 1 ? run_order_relax_m32<true> : run_order_relax_m32<false>;
        }
      if constexpr (W <= 3) {
        if (k.m32 || (k.c16 && k.idl)) return nullptr;
        if (k.c16) return k.verify ? relax_instance<W, true, true, false>(k) : relax_instance<W, false, true, false>(k);
        if (k.idl) return k.verify ? relax_instance<W, true, false, true>(k) : relax_instance<W, false, false, true>(k);
        return k.verify ? nullptr : relax_instance<W, false, false, false>(k);
      }
      return nullptr;
    case KAS_K_P4_ORDER:
      if constexpr (W == 3)
        if (k.m32) {
          if (!k.idl || k.c16) return nullptr;
          return k.tiles == 2 ? run_p4_order<3, true, false, true, true, true> : k.tiles == 1 ? run_p4_order<3, true, false, true, true> : run_p4_order<3, false, false, true, true>;
        }
      if constexpr (W <= 3) {
        if (k.m32 || (k.c16 != 0) == (k.idl != 0)) return nullptr;
        return k.c16 ? p4_order_instance<W, true>(k) : p4_order_instance<W, false>(k);
      }
      return nullptr;
    case KAS_K_ORDER_RELAX_WIDE:
      if constexpr (W == 4 || W == 5) return run_order_relax_wide<W>;
      return nullptr;
    case KAS_K_ORDER_TICKET:
      if constexpr (W <= 3) {
        if (k.G == 1) return k.packed ? run_order_tickets<W, 1, true> : run_order_tickets<W, 1, false>;
        if (k.G == 2) return k.packed ? run_order_tickets<W, 2, true> : run_order_tickets<W, 2, false>;
        if (k.G == 4) return k.packed ? run_order_tickets<W, 4, true> : run_order_tickets<W, 4, false>;
      }
      return nullptr;
    case KAS_K_ORDER_WIDE:
      if constexpr (W == 4 || W == 5) return run_order_wide<W>;
      return nullptr;
    case KAS_K_ORDER_ROUND: return run_order_rounds<W>;
    default:
      if constexpr (W >= 3 && W <= 5) {
        if (k.family == KAS_K_SPREAD_A) return run_spread_a<W>;
        if (k.family == KAS_K_SPREAD_Q) return run_spread_quota<W>;
        if (k.family == KAS_K_SPREAD_B) return run_spread_b<W>;
        if (k.family == KAS_K_SPREAD_P4) return run_spread_p4<W>;
      }
      return nullptr;
  }
}
run_fn emu_kernel_for(const KasKernelId& k) {
  if (k.family == KAS_K_PERMUTATION) return run_permutation;
  switch (k.W) {
    case 2: return emu_kernel_w<2>(k);
    case 3: return emu_kernel_w<3>(k);
    case 4: return emu_kernel_w<4>(k);
    case 5: return emu_kernel_w<5>(k);
    case 8: return emu_kernel_w<8>(k);
    default: return nullptr;
  }
}
// workgroups of an emulated kas_fill_kernel launch: KAS_EMU_FILL_GRID (default 3: most batches of the suites then have workgroups
// that take several scenarios in a row, as a launch on fewer workgroups than scenarios does on the GPU), at most one per scenario
static int32_t emu_fill_grid(int32_t n_scenarios) {
  const char* e = getenv("KAS_EMU_FILL_GRID");
  int32_t g = e ? atoi(e) : 3;
  if (g < 1) g = 1;
  return g < n_scenarios ? g : (n_scenarios > 0 ? n_scenarios : 1);
}
static int g_last_handback = -1;           // what the last by-rank launch left in KasLaunch::handback (-1: there was none)

}  // namespace

// rows the ticket-form solver decided inside queues during the last kas_emu_solve_batch (summed
// over scenarios): lets a CPU test assert that the queue path ran, not only the one-row path
static long g_last_queue_rows = 0;
static int g_last_p4_order = 0;       // the last solve ran first fit inside the order kernel's workgroup (kas_p4_order_kernel)
static int g_last_relax_idl = 0;      // the last relaxation-form launch read its broker ids from the LDS
static long g_last_slim_fill = 0;    // scenarios the slim fill kernel solved itself (not handed back) in the last kas_emu_solve_batch
static long g_last_relax_quad = 0;   // the last kas_emu_solve_batch ran the relaxation form over quad tiles
static long g_last_mid32 = 0;        // the last kas_emu_solve_batch moved its mid rows as one dword each (KAS_FLAG_MID32)
static long g_last_index_rows = 0;   // topics whose fill took the index rows (fill_pass_a_fused<EMIT>) in the last kas_emu_solve_batch
static int g_last_fused = 0;   // the last kas_emu_solve_batch ran the fill with per-chunk histograms
static int g_last_spread = 0;  // scenarios the spread fill solved itself (not handed back) in the last kas_emu_solve_batch
static int g_last_order_form = 0;   // 1: ticket form (lists <= 3 wide), 2: wide ticket form, 3: relaxation form, 0: round form (the last solve's plan)
static int g_last_split_p4 = 0;     // the last solve ran its first fit in kas_p4_kernel (KAS_FLAG_SPLIT_P4)
static long g_last_relax_tiles = 0, g_last_relax_evals = 0, g_last_relax_slow = 0;   // relaxation form: tiles, evaluations, tiles off the straight-line path
static int g_last_flagged = 0; // scenarios a ticket form left to the round form (Context counters too large for its fields)
// flags: low byte = KAS_FLAG_*, bits 8..11 = wavefronts per scenario of the fill kernel, bits
// 12..15 = scenarios per wavefront of the ticket-form order kernel (0 = the planner's choice),
// bit 16 = KAS_FLAG_TICKET_ORDER (the ticket form where the relaxation form would run), bits 17 / 18 = tiles of 64 rows /
// double tiles in the relaxation form whatever the batch size, bit 21 = KAS_FLAG_NO_RTN_QUOTA
static int emu_solve(const kas_batch_desc* b, const kas_tables* t, unsigned flags, char* errbuf, int errlen, bool c16);

extern "C" __attribute__((visibility("default")))
int kas_emu_solve_batch(const kas_batch_desc* b, const kas_tables* t, unsigned flags, char* errbuf, int errlen) {
  return emu_solve(b, t, flags, errbuf, errlen, false);
}

// kas_plan_create16 + kas_solve_device16 (ABI v5): t->cur / t->out point at uint16 node-index cells, b->node_id is not read
extern "C" __attribute__((visibility("default")))
int kas_emu_solve_batch16(const kas_batch_desc* b, const kas_tables* t, unsigned flags, char* errbuf, int errlen) {
  std::vector<int32_t> ids((size_t)(b->node_pool_len > 0 ? b->node_pool_len : 0), 0);
  for (int32_t s = 0; s < b->n_scenarios; ++s)
    for (int32_t i = 0; i < b->scenarios[s].n_nodes; ++i) ids[(size_t)(b->scenarios[s].node_off + i)] = i;
  kas_batch_desc ib = *b;
  ib.node_id = ids.data();
  return emu_solve(&ib, t, flags, errbuf, errlen, true);
}

static int emu_solve(const kas_batch_desc* b, const kas_tables* t, unsigned flags, char* errbuf, int errlen, bool c16) {
  KasShape sh;
  std::string err;
  auto refuse = [&](int code, const char* why) {
    if (errbuf && errlen > 0) { strncpy(errbuf, why, (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
    return code;
  };
  int rc = kas_shape_batch(b, &sh, &err, (int)((flags >> 8) & 0xfu), (int)((flags >> 12) & 0xfu));
  if (rc != KAS_E_OK) return refuse(rc, err.c_str());
  // the plan's state as kas_plan_create(16) + kas_plan_set_flags(flags) leave it, on a context whose self-test passed
  KasLaunchIn in;
  kas_launch_in_shape(&in, &sh);
  in.n_scenarios = b->n_scenarios; in.single_topic = kas_batch_single_topic(b) ? 1 : 0; in.cells16 = c16 ? 1 : 0;
  in.relax_gather = getenv("KAS_EMU_RELAX_GATHER") && getenv("KAS_EMU_RELAX_GATHER")[0] == '1';
  kas_launch_in_user_flags(&in, flags);
  if (c16 && !kas_cells16_ok(sh, in.lane_order_ok, in.built)) return refuse(KAS_E_UNSUPPORTED, "16-bit cells: lists up to 3 wide, relaxation or round form");
  if (const char* why = kas_flags_refusal(sh, c16, flags, in.relax_gather != 0)) return refuse(KAS_E_UNSUPPORTED, why);
  const KasResolvedLaunch L = kas_resolve_launch(in);
  const int32_t S = b->n_scenarios, CH = L.spread_chunks;
  const KasStage* order = L.find(KAS_STAGE_ORDER);
  g_last_order_form = L.order_form;
  g_last_fused = (L.flags & KAS_FLAG_FUSED_HIST) ? 1 : 0;
  g_last_mid32 = (L.flags & KAS_FLAG_MID32) ? 1 : 0;
  g_last_p4_order = order->k.family == KAS_K_P4_ORDER ? 1 : 0;
  g_last_split_p4 = L.find(KAS_STAGE_P4) ? 1 : 0;
  g_last_relax_quad = L.order_form == 3 && order->k.tiles == 2 ? 1 : 0;
  if (L.order_form == 3) g_last_relax_idl = order->k.idl;
  g_last_relax_tiles = 0; g_last_relax_evals = 0; g_last_relax_slow = 0;
  g_last_queue_rows = 0; g_last_flagged = 0; g_last_index_rows = 0; g_last_spread = 0; g_last_slim_fill = 0; g_last_handback = -1;
  // scratch the kernels must write before they read it
  std::vector<uint64_t> accmask((size_t)sh.accmask_words + 1, 0xDEADBEEFDEADBEEFull);
  std::vector<int32_t> orph((size_t)sh.orph_ints + 64, (int32_t)0xDEADBEEF);
  std::vector<int64_t> stats((size_t)KAS_STATS_PER_SCENARIO * (size_t)(S + 1), 0);
  std::vector<int32_t> perm((size_t)S + 1, -1);
  std::vector<int32_t> ord_flag((size_t)S + 1, 0);      // scenarios an order kernel leaves to the round form
  std::vector<int32_t> sp_hist, sp_quota, sp_node, sp_oc, p4s;
  std::vector<int32_t> sp_flag((size_t)S + 1, CH > 0 ? 0 : (int32_t)0xDEADBEEF);   // (the slim kernel writes every scenario's; the spread fill's are cleared)
  KasLaunch a;
  a.scen = b->scenarios; a.topics = b->topics; a.node_id = b->node_id; a.node_rack = b->node_rack;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.ctx = t->ctx;
  a.topic_results = t->topic_results; a.scenario_results = t->scenario_results;
  a.accmask = accmask.data(); a.accmask_off = sh.accmask_off.data();
  a.stats = stats.data();
  a.orph = orph.data(); a.orph_off = sh.orph_off.data();
  a.perm = nullptr; a.ord_flag = ord_flag.data();
  a.n_scenarios = S; a.n_max = sh.n_max; a.idmap_entries = sh.idmap_entries; a.need_bsearch = sh.need_bsearch;
  a.sp_hist = nullptr; a.sp_quota = nullptr; a.sp_node = nullptr; a.sp_flag = nullptr; a.sp_oc = nullptr; a.sp_chunks = 0;
  a.handback = nullptr; a.p4s = nullptr;
  if (CH > 0) {
    const size_t NM = (size_t)sh.n_max;
    sp_hist.assign((size_t)S * (size_t)CH * (size_t)sh.Wc * NM + 1, (int32_t)0xDEADBEEF);
    sp_quota.assign((size_t)S * (size_t)CH * NM + 1, (int32_t)0xDEADBEEF);
    sp_node.assign((size_t)S * 2 * NM + 1, (int32_t)0xDEADBEEF);
    sp_oc.assign((size_t)S * (size_t)(CH + 2) + 1, 0);
  }
  if (L.flags & KAS_FLAG_SPLIT_P4) {
    p4s.assign((size_t)b->n_topics * (size_t)(KAS_P4S_HEAD + (sh.n_max > 0 ? sh.n_max : 1)) + 64, (int32_t)0xDEADBEEF);
    a.p4s = p4s.data();
  }
  auto bad = [&](const std::string& what, int32_t s) {
    if (errbuf && errlen > 0) snprintf(errbuf, (size_t)errlen, "wave divergence / deadlock in %s, workgroup %d", what.c_str(), s);
    return -100;
  };
  const size_t GUARD = 4096;
  for (int32_t i = 0; i < L.n_stages; ++i) {
    const KasStage& sg = L.stages[i];
    const run_fn f = emu_kernel_for(sg.k);
    const std::string name = kas_kernel_name(sg.k);
    if (!f) return refuse(KAS_E_UNSUPPORTED, (name + ": no such instance").c_str());
    KasLaunch la = a;
    la.flags = sg.flags;
    la.perm = sg.perm ? perm.data() : nullptr;
    la.sp_flag = sg.sp_flag == KAS_SP_FLAG_PLAN ? sp_flag.data() : (sg.sp_flag == KAS_SP_FLAG_ORD ? ord_flag.data() : nullptr);
    if (sg.spread) { la.sp_hist = sp_hist.data(); la.sp_quota = sp_quota.data(); la.sp_node = sp_node.data(); la.sp_oc = sp_oc.data(); la.sp_chunks = CH; }
    // the by-rank launch's count (the product asks for it behind the slim kernel; here behind the spread fill too)
    int32_t hb = -1;
    const bool by_rank = sg.role == KAS_STAGE_FILL && sg.sp_flag == KAS_SP_FLAG_PLAN;
    if (by_rank) la.handback = &hb;
    if (sg.role == KAS_STAGE_ROUND_FLAGGED)
      for (int32_t s = 0; s < S; ++s) g_last_flagged += ord_flag[(size_t)s] != 0 ? 1 : 0;
    if (sg.k.family == KAS_K_SPREAD_Q) {                     // (a thread per (scenario, node): no collectives)
      SpreadArgs ra{&la, 0, 0, nullptr};
      f(&ra);
      continue;
    }
    // every workgroup on exactly the LDS the product launches the kernel with, uninitialised as on hardware, and a guard behind it:
    // the hardware drops what a workgroup writes beyond its allocation and reads zeros there — here that must not pass unnoticed
    std::vector<unsigned char> lds((size_t)sg.lds + GUARD);
    const bool per_chunk = sg.k.family == KAS_K_SPREAD_A || sg.k.family == KAS_K_SPREAD_B;
    const bool is_fill = sg.k.family == KAS_K_FILL;
    const int32_t step = sg.k.family == KAS_K_ORDER_TICKET ? sg.k.G : 1;
    const int32_t n_blocks = sg.k.family == KAS_K_PERMUTATION ? 1 : is_fill ? emu_fill_grid(S) : per_chunk ? S * CH : (S + step - 1) / step;
    for (int32_t blk = 0; blk < n_blocks; ++blk) {
      memset(lds.data(), 0xCD, (size_t)sg.lds);
      memset(lds.data() + sg.lds, 0xA5, GUARD);
      int r;
      if (is_fill) {                                          // (fill_block: its loop over the scenarios it takes, the LDS NOT cleared between them)
        BlockArgs ra{&la, blk, n_blocks, lds.data()};
        r = kasw::run_block(f, &ra, (int)sg.block / 64);
      } else if (sg.role == KAS_STAGE_SPREAD) {
        SpreadArgs ra{&la, per_chunk ? blk / CH : blk, per_chunk ? blk % CH : 0, lds.data()};
        r = kasw::run_block(f, &ra, (int)sg.block / 64);
      } else {
        RunArgs ra{&la, blk * step, lds.data()};
        r = kasw::run_block(f, &ra, (int)sg.block / 64);
      }
      if (r != 0) return bad(name, blk);
      for (size_t j = 0; j < GUARD; ++j)
        if (lds[(size_t)sg.lds + j] != 0xA5) return bad(name + ": LDS written beyond the launch's allocation", blk);
    }
    if (by_rank) g_last_handback = hb;
    // what the tests observe, per family
    if (sg.k.family == KAS_K_SPREAD_P4)
      for (int32_t s = 0; s < S; ++s) g_last_spread += sp_flag[(size_t)s] == 0 ? 1 : 0;
    if (sg.role == KAS_STAGE_SLIM)
      for (int32_t s = 0; s < S; ++s) {
        if (sp_flag[(size_t)s] != 0 && sp_flag[(size_t)s] != 1) return bad("slim fill (hand-back flag not written)", s);
        g_last_slim_fill += sp_flag[(size_t)s] == 0 ? 1 : 0;
      }
    if (sg.role == KAS_STAGE_FILL)
      for (int32_t s = 0; s < S; ++s)
        g_last_index_rows += (long)a.stats[(int64_t)s * KAS_STATS_PER_SCENARIO + 6];   // (the fill's own tally, before an order kernel writes there)
    if (sg.role == KAS_STAGE_PERMUTATION) {
      std::vector<char> seen((size_t)S, 0);                  // it must be a permutation, whatever the order
      for (int32_t j = 0; j < S; ++j) {
        const int32_t v = perm[(size_t)j];
        if (v < 0 || v >= S || seen[(size_t)v]) return bad("permutation (not a permutation)", j);
        seen[(size_t)v] = 1;
      }
      int32_t kmax = 0, shift = 0;                           // ... and largest key classes first
      for (int32_t j = 0; j < S; ++j) kmax = a.scenario_results[j].moved_replicas > kmax ? a.scenario_results[j].moved_replicas : kmax;
      while ((kmax >> shift) >= KAS_PERM_BINS) ++shift;
      for (int32_t j = 0; j + 1 < S; ++j)
        if ((a.scenario_results[perm[(size_t)j]].moved_replicas >> shift) < (a.scenario_results[perm[(size_t)j + 1]].moved_replicas >> shift))
          return bad("permutation (not descending by key class)", j);
    }
    if (sg.role != KAS_STAGE_ORDER) continue;
    const bool ticket_form = sg.k.family == KAS_K_ORDER_TICKET || sg.k.family == KAS_K_ORDER_WIDE;
    for (int32_t s = 0; s < S; ++s) {
      const int64_t* st = a.stats + (int64_t)s * KAS_STATS_PER_SCENARIO;
      if (ticket_form) g_last_queue_rows += (long)st[14];
      else if (sg.k.family != KAS_K_ORDER_ROUND) {
        g_last_relax_evals += (long)st[9]; g_last_relax_tiles += (long)st[12];
        if (sg.k.family != KAS_K_ORDER_RELAX_WIDE) g_last_relax_slow += (long)st[13];
      }
      if (!ticket_form || !getenv("KAS_EMU_STATS")) continue;
      fprintf(stderr, "emu stats (%s) s=%d solver_iter=%lld bulk_solver_iter=%lld queue_passes=%lld run_rounds=%lld run_rows=%lld blocked=%lld stager_iter=%lld stager_idle=%lld sched_rounds(last block)=%ld\n",
              name.c_str(), s, (long long)st[9], (long long)st[15], (long long)st[6], (long long)st[10], (long long)st[14], (long long)st[11], (long long)st[12],
              (long long)st[13], kasw::g_last_block_rounds);
      if (sg.k.family == KAS_K_ORDER_WIDE)
        fprintf(stderr, "emu diag (wide, -DKAS_WIDE_DIAG) joint_steps=%lld in_hand=%lld hold_hot=%lld wait_hot_only=%lld eligible=%lld | not eligible: many_ahead_elsewhere=%lld one_ahead_not_in_hand=%lld behind_gap=%lld\n",
                (long long)st[13], (long long)st[3], (long long)st[4], (long long)st[5], (long long)st[7], (long long)st[0], (long long)st[1], (long long)st[2]);
    }
  }
  return KAS_E_OK;
}

// kas_plan_describe for a batch + flag word + cell width, without running anything: the text rendered from the launch the emulator
// would walk (a context whose self-test passed, a plan that has not solved yet).  Returns kas_shape_batch's / the plan's refusal.
extern "C" __attribute__((visibility("default")))
int kas_emu_describe(const kas_batch_desc* b, unsigned flags, int cells16, char* buf, int n) {
  KasShape sh;
  std::string err;
  int rc = kas_shape_batch(b, &sh, &err, (int)((flags >> 8) & 0xfu), (int)((flags >> 12) & 0xfu));
  if (rc == KAS_E_OK && cells16 && !kas_cells16_ok(sh, 1, KAS_BUILT_ALL)) { rc = KAS_E_UNSUPPORTED; err = "16-bit cells: lists up to 3 wide, relaxation or round form"; }
  if (rc == KAS_E_OK)
    if (const char* why = kas_flags_refusal(sh, cells16 != 0, flags, false)) { rc = KAS_E_UNSUPPORTED; err = why; }
  KasLaunchIn in;
  if (rc == KAS_E_OK) {
    kas_launch_in_shape(&in, &sh);
    in.n_scenarios = b->n_scenarios; in.single_topic = kas_batch_single_topic(b) ? 1 : 0; in.cells16 = cells16 ? 1 : 0;
    kas_launch_in_user_flags(&in, flags);
    err = kas_describe_launch(kas_resolve_launch(in));
  }
  if (buf && n > 0) { strncpy(buf, err.c_str(), (size_t)n - 1); buf[n - 1] = 0; }
  return rc;
}

// Is the launch the resolver returns for a batch + flag word + cell width launchable?  Every stage's LDS within 160 KiB, exactly one
// order stage, every kernel identity an instance of the emulator's mapping, and every (identity, LDS) among those the enumeration
// behind kas_plan_set_kernels covers for the plan as kas_plan_create leaves it.  0 and the describe text; 1 and what is wrong; a
// negative KAS_E_* and the refusal when no plan takes the batch / the flags.
extern "C" __attribute__((visibility("default")))
int kas_emu_launch_check(const kas_batch_desc* b, unsigned flags, int cells16, char* buf, int n) {
  const int rc = kas_emu_describe(b, flags, cells16, buf, n);
  if (rc != KAS_E_OK) return rc;
  KasShape sh;                                               // the plan as created (its shape's own waves and groups) ...
  std::string err;
  if (kas_shape_batch(b, &sh, &err, 0, 0) != KAS_E_OK) return 1;
  KasLaunchIn created, in;
  kas_launch_in_shape(&created, &sh);
  created.n_scenarios = b->n_scenarios; created.single_topic = kas_batch_single_topic(b) ? 1 : 0; created.cells16 = cells16 ? 1 : 0;
  in = created;
  KasShape asked = sh;                                       // ... and as kas_plan_set_flags(flags) leaves it
  if (kas_shape_batch(b, &asked, &err, (int)((flags >> 8) & 0xfu), (int)((flags >> 12) & 0xfu)) != KAS_E_OK) return 1;
  kas_launch_in_shape(&in, &asked);
  kas_launch_in_user_flags(&in, flags);
  created.NW = in.NW; created.G = in.G; created.fused = in.fused;   // (kas_plan_set_flags moves these before it opts the kernels in)
  created.lds_total = in.lds_total; created.lds_fused_total = in.lds_fused_total;
  const KasResolvedLaunch L = kas_resolve_launch(in);
  std::string bad;
  int orders = 0;
  for (int32_t i = 0; i < L.n_stages && bad.empty(); ++i) {
    const KasStage& sg = L.stages[i];
    orders += sg.role == KAS_STAGE_ORDER ? 1 : 0;
    bool opted = sg.lds == 0u;
    created.shape = in.shape;
    kas_enumerate_launches(created, [&](const KasStage& e) { opted = opted || (e.k == sg.k && e.lds >= sg.lds); });
    if (sg.lds > (uint32_t)KAS_LDS_LIMIT) bad = kas_kernel_name(sg.k) + ": LDS beyond 160 KiB";
    else if (!emu_kernel_for(sg.k)) bad = kas_kernel_name(sg.k) + ": not an instance of the emulator";
    else if (!opted) bad = kas_kernel_name(sg.k) + ": not among the launches kas_plan_set_kernels enumerates";
  }
  if (bad.empty() && orders != 1) bad = "not exactly one order stage";
  if (bad.empty()) return 0;
  if (buf && n > 0) { strncpy(buf, bad.c_str(), (size_t)n - 1); buf[n - 1] = 0; }
  return 1;
}

// The product's planning decision for a batch shape, without running anything (plan-math tests):
// out[0..9] = tickets_ok, wide_ok, round_fits, G, NW, with_x, packed_ok, fused_ok, wide_checked, relax_ok.  Returns kas_shape_batch's code.
extern "C" __attribute__((visibility("default")))
int kas_emu_shape(const kas_batch_desc* b, int32_t* out, char* errbuf, int errlen) {
  KasShape sh;
  std::string err;
  const int rc = kas_shape_batch(b, &sh, &err, 0, 0);
  if (rc != KAS_E_OK) {
    if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
    return rc;
  }
  out[0] = sh.tickets_ok; out[1] = sh.wide_ok; out[2] = sh.round_fits; out[3] = sh.G; out[4] = sh.NW;
  out[5] = sh.with_x; out[6] = sh.packed_ok; out[7] = sh.fused_ok; out[8] = sh.wide_checked; out[9] = sh.relax_ok;
  return rc;
}

// spread fill planning: chunks per scenario for a batch of n_scenarios single-topic scenarios of this shape
// (0: the one-workgroup fill kernel), and the LDS of its scan kernels (pass A, pass B, the one-workgroup layout)
extern "C" __attribute__((visibility("default")))
int kas_emu_spread_plan(const kas_batch_desc* b, int32_t* out) {
  KasShape sh;
  std::string err;
  const int rc = kas_shape_batch(b, &sh, &err, 0, 0);
  if (rc != KAS_E_OK) return rc;
  out[0] = kas_spread_chunks(sh, b->n_scenarios, kas_batch_single_topic(b), false);
  out[1] = kas_spread_scan_lds(sh.n_max, sh.Wc, sh.idmap_entries, sh.need_bsearch, 1).total;
  out[2] = kas_spread_scan_lds(sh.n_max, sh.Wc, sh.idmap_entries, sh.need_bsearch, 2).total;
  out[3] = kas_fill_lds_layout(sh.n_max, sh.Wc, 1, sh.idmap_entries, sh.need_bsearch, 1).total;
  out[4] = (int32_t)(((int64_t)sh.max_partitions + 63) / 64);
  return rc;
}

// kas_plan_host_call for a batch + the kas_tables lengths + a selection, without running anything (tests/test_host_call.py).
//   lens[4]     cur_len, out_len, aux_len, ctx_len
//   missing     tables that are NULL: bit 0 cur, 1 out, 2 aux, 3 ctx, 4 topic_results, 5 scenario_results, 6 impact nodes, 7 impact scenarios
//   head[12]    K, native16, need32, entries of sel_off, entries of imp_base, then the batch's cur / out / aux extents [lo, need) and ctx_lo
//   ranges      [K][10] scenarios, topics, cur, out, ctx: lo and hi of each
//   scen        the ranges' rebased scenario descriptors, one range after the other ([n_scenarios])
//   bytes       [KAS_HB_COUNT] in KasHostBuf's order;  sel_off [n_select + 1];  imp_base [n_scenarios + 1] when `impact`
// Returns the planner's code; its text in errbuf.
extern "C" __attribute__((visibility("default")))
int kas_emu_host_call(const kas_batch_desc* b, const int64_t* lens, unsigned missing, const int32_t* select, int32_t n_select, int cells16,
                      int impact, int lane_order_ok, unsigned built, int ranges_override, int64_t* head, int64_t* ranges,
                      kas_scenario_desc* scen, int64_t* bytes, int64_t* sel_off, int64_t* imp_base, char* errbuf, int errlen) {
  std::vector<int32_t> ident_ids;
  uint64_t ident_stamp = 0;
  KasHostCallIn in;
  in.batch = b;
  in.cur_len = lens[0]; in.out_len = lens[1]; in.aux_len = lens[2]; in.ctx_len = lens[3];
  in.have_cur = !(missing & 1u); in.have_out = !(missing & 2u); in.have_aux = !(missing & 4u); in.have_ctx = !(missing & 8u);
  in.have_topic_results = !(missing & 16u); in.have_scenario_results = !(missing & 32u);
  in.select = select; in.n_select = n_select;
  in.cells16 = cells16 != 0; in.ident_ids = &ident_ids; in.ident_stamp = &ident_stamp;
  in.impact = impact != 0; in.have_imp_nodes = !(missing & 64u); in.have_imp_scenarios = !(missing & 128u);
  in.lane_order_ok = lane_order_ok;
  for (uint32_t& m : in.built16) m = built;
  in.ranges_override = ranges_override;
  KasHostCall hc;
  std::string err;
  const int rc = kas_plan_host_call(in, &hc, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  if (rc != KAS_E_OK) return rc;
  const KasShape& f = hc.full;
  const int64_t h[12] = {hc.K, hc.native16, hc.need32, (int64_t)hc.sel_off.size(), (int64_t)hc.imp_base.size(),
                         f.cur_lo, f.cur_need, f.out_lo, f.out_need, f.aux_lo, f.aux_need, f.ctx_lo};
  memcpy(head, h, sizeof(h));
  for (const KasHostRange& r : hc.ranges) {
    *ranges++ = r.lo; *ranges++ = r.hi;
    for (const KasExtent& e : r.own) { *ranges++ = e.lo; *ranges++ = e.hi; }
    for (int64_t i = 0; i < r.hi - r.lo; ++i) *scen++ = r.scen[(size_t)i];
  }
  for (int i = 0; i < KAS_HB_COUNT; ++i) bytes[i] = (int64_t)hc.bytes[i];
  for (size_t i = 0; i < hc.sel_off.size(); ++i) sel_off[i] = hc.sel_off[i];
  for (size_t i = 0; i < hc.imp_base.size(); ++i) imp_base[i] = hc.imp_base[i];
  return rc;
}

// kas_cache_choose over a table of n entries of {occupied, key, sig, last_use, call}: the lowest candidate hit (confirmed by the
// byte compare in the library) in *hit, or -1; the victim of a miss in *victim, or -1 (the library's KAS_E_NOMEM)
extern "C" __attribute__((visibility("default")))
void kas_emu_cache_choose(const uint64_t* entries, int32_t n, uint64_t key, uint64_t sig, uint64_t this_call, int32_t* hit, int32_t* victim) {
  std::vector<KasCacheEntry> e((size_t)n);
  for (int32_t i = 0; i < n; ++i) e[(size_t)i] = KasCacheEntry{(int32_t)entries[5 * i], entries[5 * i + 1], entries[5 * i + 2], entries[5 * i + 3], entries[5 * i + 4]};
  const KasCacheChoice c = kas_cache_choose(e.data(), n, key, sig, this_call);
  *hit = c.hits ? __builtin_ctz(c.hits) : -1;
  *victim = c.victim;
}

// the slicing arithmetic behind the library's kas_shard_range / kas_batch_slice and the cache's key and signature of a batch
extern "C" __attribute__((visibility("default")))
void kas_emu_shard_range(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi) { kas_range_of(total, rank, world, lo, hi); }
extern "C" __attribute__((visibility("default")))
int kas_emu_batch_slice(const kas_batch_desc* b, int64_t lo, int64_t hi, kas_scenario_desc* scratch, kas_batch_desc* out, const kas_tables* tables,
                        kas_tables* tables_out, char* errbuf, int errlen) {
  std::string err;
  const int rc = kas_slice_batch(b, lo, hi, scratch, out, tables, tables_out, &err);
  if (errbuf && errlen > 0) { strncpy(errbuf, err.c_str(), (size_t)errlen - 1); errbuf[errlen - 1] = 0; }
  return rc;
}
extern "C" __attribute__((visibility("default")))
void kas_emu_batch_ident(const kas_batch_desc* b, int cells16, uint64_t* key_sig) {
  const KasBatchIdent id(b, cells16);
  key_sig[0] = id.key; key_sig[1] = id.sig;
}

extern "C" __attribute__((visibility("default")))
long kas_emu_collectives(void) { return kasw::g_emu.collectives; }

extern "C" __attribute__((visibility("default")))
long kas_emu_last_queue_rows(void) { return g_last_queue_rows; }

extern "C" __attribute__((visibility("default")))
int kas_emu_last_fused(void) { return g_last_fused; }

extern "C" __attribute__((visibility("default")))
long kas_emu_last_index_rows(void) { return g_last_index_rows; }
extern "C" __attribute__((visibility("default")))
long kas_emu_last_mid32(void) { return g_last_mid32; }
extern "C" __attribute__((visibility("default")))
long kas_emu_last_relax_quad(void) { return g_last_relax_quad; }
extern "C" __attribute__((visibility("default")))
long kas_emu_last_slim_fill(void) { return g_last_slim_fill; }

// scenarios the last by-rank launch of kas_fill_kernel counted as flagged (KasLaunch::handback; -1: no such launch in the last solve)
extern "C" __attribute__((visibility("default")))
int kas_emu_last_handback(void) { return g_last_handback; }

extern "C" __attribute__((visibility("default")))
int kas_emu_last_relax_idl(void) { return g_last_relax_idl; }

extern "C" __attribute__((visibility("default")))
int kas_emu_last_p4_order(void) { return g_last_p4_order; }

extern "C" __attribute__((visibility("default")))
int kas_emu_last_spread(void) { return g_last_spread; }

extern "C" __attribute__((visibility("default")))
int kas_emu_last_flagged(void) { return g_last_flagged; }

extern "C" __attribute__((visibility("default")))
int kas_emu_last_order_form(void) { return g_last_order_form; }
// 1: the last solve's first fit ran in kas_p4_kernel
extern "C" __attribute__((visibility("default")))
int kas_emu_last_split_p4(void) { return g_last_split_p4; }


// relaxation form of the last kas_emu_solve_batch: out[0..2] = tiles, evaluations, tiles off the straight-line path
extern "C" __attribute__((visibility("default")))
void kas_emu_last_relax_stats(long* out) { out[0] = g_last_relax_tiles; out[1] = g_last_relax_evals; out[2] = g_last_relax_slow; }

// ---------------------------------------------------------------------------------------------
// Unit harness for the parallel P4 of the fill kernel (p4_lists_parallel<3, 4>): the caller gives the
// node state (load, rack, the list of non-full nodes in processing order), the orphan rows in row
// order and their mid rows; the four wavefronts run the windows exactly as the kernel does.  With
// KAS_EMU_WAVE_DIV one wave can be made slow, which is how a test provokes one window overtaking
// another (tests/test_emu_p4_windows.py).  Returns 0, or -100 on divergence / deadlock.
// ---------------------------------------------------------------------------------------------
namespace {
struct P4Args { kas::LdsView L; kas::TopicView T; int32_t live_count; int32_t fail_row; };
void run_p4_unit(void* p) {
  P4Args* r = (P4Args*)p;
  int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t fail_win = -1, fail_row = -1;
  kas::p4_lists_parallel<3, 4>(r->L, r->T, r->live_count, kasw::wave_id(), st, fail_win, fail_row);
  if (fail_win >= 0 && kasw::lane() == 0) r->fail_row = fail_row;     // (any failing window: the tests place everything)
}
}  // namespace

extern "C" __attribute__((visibility("default")))
int kas_emu_p4_unit(int32_t n_nodes, const int32_t* load, const int32_t* rack, int32_t cap, int32_t live_count,
                    const int32_t* live, int32_t n_orphans, int32_t* orphan_rows, int32_t P, uint16_t* mid,
                    int32_t* load_out) {
  const KasLds lay = kas_fill_lds_layout(n_nodes, 3, 4, 0, 0, 1);
  std::vector<unsigned char> lds((size_t)lay.total + 64, 0xCD);
  P4Args r;
  r.L.x = (int32_t*)(lds.data() + lay.off_x);
  r.L.load = (int32_t*)(lds.data() + lay.off_load);
  r.L.qrs = (int32_t*)(lds.data() + lay.off_qrs);
  r.L.rack = (int16_t*)(lds.data() + lay.off_rack);
  r.L.live = (int16_t*)(lds.data() + lay.off_live);
  r.L.ns = 1; r.L.rs = 1;
  r.L.idmap = (int16_t*)(lds.data() + lay.off_idmap);
  r.L.ids = (int32_t*)(lds.data() + lay.off_ids);
  r.L.ring_p = (int32_t*)(lds.data() + lay.off_ring);
  r.L.ring_meta = r.L.ring_p + KAS_RING_CAP;
  r.L.ring_rack = (int16_t*)(r.L.ring_meta + KAS_RING_CAP);
  r.L.ctl = (int32_t*)(lds.data() + lay.off_ctl);
  for (int32_t i = 0; i < n_nodes; ++i) { r.L.load[i] = load[i]; r.L.rack[i] = (int16_t)rack[i]; }
  for (int32_t i = 0; i < live_count; ++i) r.L.live[i] = (int16_t)live[i];
  for (int i = 0; i < KAS_CTL_INTS; ++i) r.L.ctl[i] = i == KAS_CTL_FAILROW ? -1 : (i == KAS_CTL_FAILWIN ? 0x7fffffff : 0);
  r.L.ctl[KAS_CTL_OC] = n_orphans;                               // one list: chunk 0 holds every orphan
  r.L.ctl[KAS_CTL_LIVE] = live_count;
  memset(&r.T, 0, sizeof(r.T));
  r.T.orph = orphan_rows; r.T.mid = mid;
  r.T.P = P; r.T.cw = 3; r.T.rf = 3; r.T.ow = 3; r.T.nt = (P + 63) >> 6; r.T.N = n_nodes; r.T.cap = cap;
  r.live_count = live_count; r.fail_row = -1;
  if (kasw::run_block(run_p4_unit, &r, 4) != 0) return -100;
  for (int32_t i = 0; i < n_nodes; ++i) load_out[i] = r.L.load[i];
  return r.fail_row >= 0 ? 1 : 0;
}
