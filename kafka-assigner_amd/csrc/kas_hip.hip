// kas_hip.hip — gfx950 kernels + the C ABI of include/kas_abi.h (libkas_hip.so).
//
// A solve is three launches on one stream (device code in kas_solver_body.h):
//   kas_fill_kernel<W, NW>              P0-P4: one workgroup of NW wavefronts per scenario
//   kas_order_permutation_kernel        scenarios by descending P5 chain length
//   kas_order_relax_kernel<W,DUAL,CTX>  P5, relaxation form: one wavefront per scenario (lists <= 3 wide)
//   (or kas_order_ticket_kernel<W, G, PK>, behind kas_order_permutation_kernel: solver / stager / retirer wavefronts
//    per G scenarios; kas_order_wide_kernel<W> for lists 4 and 5 wide; kas_order_round_kernel<W>, the round form)
// Scenarios share nothing, so there is no inter-workgroup communication at all: each workgroup
// streams its own tables from HBM (coalesced 64-row tiles per wave), keeps its node state in LDS
// and writes its own out rows and one 32-byte result record.  Workgroup b lands on XCD b % 8; in
// the what-if layout (many scenarios over one shared cur table) neighbouring scenarios therefore
// spread the shared table over all eight L2s, and the 256 MiB Infinity Cache holds it once.
#define KAS_ABI_FN __host__ __device__ static inline
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kas_abi.h"
#include "kas_plan_math.h"
#include "kas_solver_body.h"
#include "kas_launch_plan.h"   // which kernels a solve launches: the resolver the emulator shares
#include "kas_host_call.h"     // what a host call does: ranges, cell width, buffer sizes, the plan cache's choice
#include "kas_impact.h"   // the impact pass (ABI v6): its kernels are kas_impact.hip's
#include "kas_racks.h"    // the rack pass behind it: its kernels are kas_racks.hip's
#include "kas_topics.h"   // the topic pass behind a solve: its kernels are kas_topics.hip's
#include "kas_choose.h"   // ranking and gathering the best scenarios: its kernels are kas_choose.hip's
#include "kas_front.h"    // marking and ranking the Pareto front: kas_choose.hip's as well
#include "kas_moves.h"    // the move list of a solve: its kernels are kas_moves.hip's
#include "kas_batches.h"  // the execution batches of a solve: its kernel is kas_batches.hip's
#include "kas_rounds.h"   // the packed rounds of a solve: its kernel is kas_rounds.hip's

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// min waves per SIMD of the fill kernel.  Its row scans keep four tiles of rows in flight per lane
// and spill heavily below 128 VGPRs: measured in round 2 (mid rows, lookup mode hoisted, event
// counters compiled out) one batch alone takes 1.30 ms at 128 VGPRs (4 waves per SIMD, 4 workgroups
// per CU) against 1.61 ms at 96 (5, the LDS limit), and with 8 batches in flight the whole-job rate
// is the same within noise (297-299k scenarios/s), so the faster single launch wins.
#ifndef KAS_FILL_MIN_WAVES
#define KAS_FILL_MIN_WAVES 4
#endif
// A launch for flagged scenarios only (KAS_FLAG_ONLY_FLAGGED: behind the slim kernel, behind the spread fill, the wide form's second
// solve) deals them to its workgroups round-robin BY RANK among the flagged ones (kas::fill_block, kas_solver_body.h) — a tenth of
// 1000 scenarios handed back is a hundred workgroups with one scenario each, not 256 of which some hold three (round 6: 25.9 -> 15 ms
// for such a batch, scripts/handback_probe.py) — and workgroup 0 leaves their number where the plan sizes its next such launch
// (KasLaunch::handback, kas_back_grid in kas_launch_plan.h).
template <int W, int NW>
__global__ __launch_bounds__(64 * NW, KAS_FILL_MIN_WAVES) void kas_fill_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::fill_block<W, NW>(a, (int32_t)blockIdx.x, (int32_t)gridDim.x, kas_lds);
}

// The slim fill (round 6): fill_scenario<W, 4, SLIM> — only the path every BASELINE config at RF <= 3 takes (kas_solver_body.h,
// fill_topic's SLIM branch): 120 VGPRs and no scratch where kas_fill_kernel<3,4> has 128 and 368 B per lane.  A scenario that
// needs another path is flagged (KasLaunch::sp_flag) and kas_fill_kernel, launched behind this one with KAS_FLAG_ONLY_FLAGGED on
// a grid of at most KAS_FILL_BACK_GRID workgroups, solves it from its first topic.  Its LDS layout holds only what that path
// touches (kas_fill_slim_lds: 31.6 KB at 1,050 brokers against 35.5).  Measured (experiments/README.md): the smaller layout +1.4 %
// in flight; 96 VGPRs (KAS_SLIM_MIN_WAVES=5: 88 B of scratch) with five workgroups per CU -0.5 %, with four and room for two order
// wavefronts per SIMD beside them (KAS_TUNE_SLIM_LDS_PAD=1280) -2 %.
#ifndef KAS_SLIM_MIN_WAVES
#define KAS_SLIM_MIN_WAVES 4
#endif
#ifndef KAS_TUNE_SLIM_LDS_PAD
#define KAS_TUNE_SLIM_LDS_PAD 0
#endif
// (M32: the instance for launches with dword mid rows, KAS_FLAG_MID32 — one store path in either instance)
template <int W, bool M32 = false>
__global__ __launch_bounds__(256, KAS_SLIM_MIN_WAVES) void kas_fill_slim_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  for (int32_t s = (int32_t)blockIdx.x; s < a.n_scenarios; s += (int32_t)gridDim.x)
    kas::fill_scenario<W, 4, true, M32 ? 1 : 0>(a, s, kas_lds);
}

// min waves per SIMD of the ticket-form order kernel (0 = whatever the allocation comes to: 92 VGPRs, 5)
#ifndef KAS_ORDER_MIN_WAVES
#define KAS_ORDER_MIN_WAVES 0
#endif
#if KAS_ORDER_MIN_WAVES > 0
#define KAS_ORDER_BOUNDS __launch_bounds__(192, KAS_ORDER_MIN_WAVES)
#else
#define KAS_ORDER_BOUNDS __launch_bounds__(192)
#endif
template <int W, int G, bool PK>
__global__ KAS_ORDER_BOUNDS void kas_order_ticket_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::order_tickets<W, G, PK>(a, (int32_t)blockIdx.x * G, kas_lds);
}

__global__ __launch_bounds__(64 * KAS_PERM_WAVES) void kas_order_permutation_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::order_permutation(a, kas_lds);
}

template <int W>
__global__ __launch_bounds__(64) void kas_order_round_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::order_scenario_rounds<W>(a, (int32_t)blockIdx.x, kas_lds);
}

// first fit (P4) of the topics the fill kernel handed over: one workgroup of four wavefronts per scenario on a slim LDS layout
// (kas_solver_body.h, p4_scenario; KAS_FLAG_SPLIT_P4)
// ONE wavefront per scenario: its windows follow each other without a hand-over between wavefronts, so nothing in the kernel
// polls — alone that is slower (fill + first fit 1.39 ms per 1000 scenarios against 1.07 ms inside the fill workgroup, 1.09 with
// four wavefronts here), with eight batches in flight it is the fastest (672k scenarios/s in a 20-step region against 617k
// inside the fill workgroup, 620k with four wavefronts, 646k with two: experiments/README.md)
// (M32: the instance for launches with dword mid rows, KAS_FLAG_MID32 — the layout is a constant of either instance)
template <int W, bool M32 = false>
__global__ __launch_bounds__(64 * KAS_P4_KERNEL_WAVES) void kas_p4_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  if constexpr (KAS_P4_PRIO > 0) kasw::set_priority<KAS_P4_PRIO>();
  kas::p4_scenario<W, KAS_P4_KERNEL_WAVES, false, (W == 3 && M32) ? 1 : 0>(a, (int32_t)blockIdx.x, kas_lds);
}

// Self-test of the one hardware property the relaxation form of P5 and the fill's quota draw rely on and the ISA documents do
// not state: the LDS serves the lanes of ONE ds_add_rtn instruction that name the same word in ascending lane order, so
// that the value returned to lane i is the word before the instruction plus the addends of the ACTIVE lanes below i
// (kas_wave.h, lds_add_rtn_u32).  Round 5: in the regime the kernels live in — four wavefronts per workgroup of which
// three hammer the same CU's LDS with atomics (with and without return, as the fill kernel's histogram and quota draws do),
// enough workgroups to put several on every CU at once, and every other round under a random EXEC mask (the fill draws
// its quota from inside a branch; round 4's test ran all 64 lanes always).  Pseudo-random words of tables of 1 .. 1024
// entries; *bad counts the lane-operations that came back with anything else.
__global__ __launch_bounds__(256) void kas_lds_order_selftest_kernel(unsigned int* bad, int iters) {
  __shared__ uint32_t tab[1024];
  __shared__ uint32_t noise[2048];
  const int lane = (int)(threadIdx.x & 63u);
  for (int i = (int)threadIdx.x; i < 1024; i += (int)blockDim.x) { tab[i] = 0u; noise[i] = 0u; noise[1024 + i] = 0u; }
  __syncthreads();
  uint32_t rng = 0x9E3779B9u * (blockIdx.x * 1024u + threadIdx.x + 1u);
  unsigned int nbad = 0;
  if (threadIdx.x < 64u) {
    const uint32_t mask = (1u << (2u * (blockIdx.x % 6u))) - 1u;      // 1, 4, 16, 64, 256, 1024 words
    for (int it = 0; it < iters; ++it) {
      rng = rng * 1664525u + 1013904223u;
      const uint32_t w = (rng >> 11) & mask, add = 1u + ((rng >> 5) & 15u);
      const bool on = (it & 1) == 0 || ((rng >> 24) & 3u) != 0u;      // odd rounds: a random three quarters of the lanes draw
      const uint32_t before = tab[w];                               // (only this wavefront writes tab)
      kasw::lockstep();
      uint32_t got = 0u;
      if (on) got = kasw::lds_add_rtn_u32(&tab[w], add);
      kasw::lockstep();
      const uint64_t onm = kasw::ballot(on);
      uint32_t lower = 0u;
      for (int l = 0; l < 64; ++l) {
        const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)w, l), al = (uint32_t)__builtin_amdgcn_readlane((int)add, l);
        lower += (l < lane && wl == w && ((onm >> l) & 1ull)) ? al : 0u;
      }
      nbad += (on && got != before + lower) ? 1u : 0u;
    }
  } else {
    for (int it = 0; it < 2 * iters; ++it) {
      rng = rng * 1664525u + 1013904223u;
      const uint32_t w = (rng >> 9) & 2047u;
      if (it & 1) atomicAdd(&noise[w], 1u << (16u * ((rng >> 3) & 1u)));       // (the fill's uint16 histogram cells)
      else if ((rng >> 28) & 1u) (void)kasw::lds_add_rtn_u32(&noise[w], 0xffffffffu);   // (its quota draw, under a mask)
    }
  }
  if (nbad) atomicAdd(bad, nbad);
}

// lists up to 3 wide: the relaxation form, one wavefront (= one workgroup) per scenario (kas_order_relax.h)
// (DUAL: the instance with double tiles, kas_relax_double_tiles)
// (CTX: the instance for batches in which some scenario hands a Context in or wants it back)
// (VERIFY: the instances for plans with KAS_PLAN_VERIFY_SAMPLE)
// (C16: the instances for plans with 16-bit cells, kas_plan_create16)
// (IDL: the instances for int32 cells with the scenario's broker ids in the LDS — kas_relax_lds_ids; the gather instances,
//  IDL = false on int32 cells, exist without the sampled verification only)
// (M32: the instances for launches with dword mid rows, KAS_FLAG_MID32 — lists 3 wide, IDL, no Context, no sampled verification)
// (QUAD: the instance with quad tiles — 256 rows a step — on dword mid rows, KAS_PLAN_RELAX_TILES(3))
template <int W, bool DUAL, bool CTX, bool VERIFY = false, bool C16 = false, bool IDL = false, bool M32 = false, bool QUAD = false>
__global__ __launch_bounds__(64) void kas_order_relax_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::order_relax<W, DUAL, CTX, VERIFY, C16, IDL, false, M32, QUAD>(a, (int32_t)blockIdx.x, kas_lds);
}

// first fit (P4) and the relaxation form of P5 in one workgroup of two wavefronts (kas_order_relax.h, p4_order_scenario): the order
// wavefront follows first fit's progress instead of waiting behind a kernel boundary — for launches whose latency is a scenario's
template <int W, bool DUAL, bool C16, bool IDL, bool M32 = false, bool QUAD = false>
__global__ __launch_bounds__(128) void kas_p4_order_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::p4_order_scenario<W, DUAL, C16, IDL, M32, QUAD>(a, (int32_t)blockIdx.x, kas_lds);
}

// lists 4 and 5 wide, relaxation form: one wavefront (= one workgroup) per scenario (kas_order_relax_wide.h)
template <int W>
__global__ __launch_bounds__(64) void kas_order_relax_wide_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::order_relax_wide<W>(a, (int32_t)blockIdx.x, kas_lds);
}

// lists 4 and 5 wide: one scenario per workgroup (stager, retirer, three solver wavefronts: kas_order_wide.h)
template <int W>
__global__ __launch_bounds__(KAS_ORDER_WIDE_BLOCK) void kas_order_wide_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::order_tickets_wide<W>(a, (int32_t)blockIdx.x, kas_lds);
}

// spread fill (kas_solver_body.h, "Spread fill"): (scenario, chunk) one-wavefront workgroups for the two
// row scans, a thread per (scenario, node) for the quota, one workgroup per scenario for P4
template <int W>
__global__ __launch_bounds__(64) void kas_spread_a_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::spread_pass_a<W>(a, (int32_t)blockIdx.y, (int32_t)blockIdx.x, kas_lds);
}
template <int W>
__global__ __launch_bounds__(256) void kas_spread_q_kernel(KasLaunch a) {
  kas::spread_quota<W>(a, (int32_t)blockIdx.y, (int32_t)(blockIdx.x * 256u + threadIdx.x));
}
template <int W>
__global__ __launch_bounds__(64) void kas_spread_b_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::spread_pass_b<W>(a, (int32_t)blockIdx.y, (int32_t)blockIdx.x, kas_lds);
}
template <int W>
__global__ __launch_bounds__(64 * KAS_SPREAD_P4_WAVES) void kas_spread_p4_kernel(KasLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_lds[];
  kas::spread_p4<W, KAS_SPREAD_P4_WAVES>(a, (int32_t)blockIdx.x, kas_lds);
}

typedef void (*kas_kernel_fn)(KasLaunch);
// Which instances this build holds.  A full build: every one.  The tuning builds (scripts/build_variant.sh, seconds to compile)
// refuse other shapes in kas_plan_create: KAS_MINIMAL_INSTANCES=5 holds what BASELINE.json configs[4] launches (lists 5 wide,
// 4 fill waves), any other value what configs[2] launches (lists 3 wide, 4 fill waves, 1 or 2 scenarios per solver wavefront; the
// relaxation form's instances also 2 wide).  The instances for dword mid rows (M32: lists 3 wide) are in every build.
#if defined(KAS_MINIMAL_INSTANCES) && KAS_MINIMAL_INSTANCES == 5
#define KAS_ONLY_WIDTH 5
#elif defined(KAS_MINIMAL_INSTANCES) && KAS_MINIMAL_INSTANCES != 0
#define KAS_ONLY_WIDTH 3
#else
#define KAS_ONLY_WIDTH 0
#endif
static constexpr bool kas_built(int family, int W, int NW = 4, int G = 2) {
  if (KAS_ONLY_WIDTH == 0) return true;
  if (family == KAS_K_ORDER_RELAX || family == KAS_K_P4_ORDER) return KAS_ONLY_WIDTH == 3 && W <= 3;
  if (W != KAS_ONLY_WIDTH || NW != 4) return false;
  if (KAS_ONLY_WIDTH == 5)
    return family != KAS_K_FILL_SLIM && family != KAS_K_ORDER_TICKET;
  return G <= 2 && (family == KAS_K_FILL || family == KAS_K_FILL_SLIM || family == KAS_K_P4 || family == KAS_K_ORDER_TICKET ||
                    family == KAS_K_ORDER_ROUND);
}
static bool kas_minimal_ok(int Wc, int NW, int G) { return kas_built(KAS_K_FILL, Wc, NW, G); }

// relaxation form: the instance for (tiles, Context); double tiles are rows of three holders
template <int W, bool VERIFY, bool C16, bool IDL>
static kas_kernel_fn kas_relax_instance(const KasKernelId& k) {
  if constexpr (W == 3)
    if (k.tiles == 1) return k.ctx ? kas_order_relax_kernel<3, true, true, VERIFY, C16, IDL> : kas_order_relax_kernel<3, true, false, VERIFY, C16, IDL>;
  if (k.tiles != 0) return nullptr;
  return k.ctx ? kas_order_relax_kernel<W, false, true, VERIFY, C16, IDL> : kas_order_relax_kernel<W, false, false, VERIFY, C16, IDL>;
}
// first fit beside it: int32 cells with the broker ids in the LDS, or 16-bit cells — the instances that wait for no gather
template <int W, bool C16>
static kas_kernel_fn kas_p4_order_instance(const KasKernelId& k) {
  if constexpr (W == 3)
    if (k.tiles == 1) return kas_p4_order_kernel<3, true, C16, !C16>;
  return k.tiles == 0 ? kas_p4_order_kernel<W, false, C16, !C16> : nullptr;
}

// THE mapping kernel identity -> kernel; nullptr: no such instance (in this build)
template <int W>
static kas_kernel_fn kas_kernel_w(const KasKernelId& k) {
  switch (k.family) {
    case KAS_K_FILL:   // (8 wavefronts per scenario: only on the CPU emulator — a minute of build time a width, and never the faster choice on the GPU)
      if constexpr (kas_built(KAS_K_FILL, W, 4)) if (k.NW == 4) return kas_fill_kernel<W, 4>;
      if constexpr (kas_built(KAS_K_FILL, W, 2)) if (k.NW == 2) return kas_fill_kernel<W, 2>;
      if constexpr (kas_built(KAS_K_FILL, W, 1)) if (k.NW == 1) return kas_fill_kernel<W, 1>;
      return nullptr;
    case KAS_K_FILL_SLIM:
      if constexpr (W == 3) if (k.m32) return kas_fill_slim_kernel<3, true>;
      if constexpr (W <= 3 && kas_built(KAS_K_FILL_SLIM, W)) if (!k.m32) return kas_fill_slim_kernel<W>;
      return nullptr;
    case KAS_K_P4:
      if constexpr (W == 3) if (k.m32) return kas_p4_kernel<3, true>;
      if constexpr (kas_built(KAS_K_P4, W)) if (!k.m32) return kas_p4_kernel<W>;
      return nullptr;
    case KAS_K_ORDER_RELAX:
      if constexpr (W == 3)
        if (k.m32) {
          if (!k.idl || k.ctx || k.verify || k.c16) return nullptr;
          return k.tiles == 2 ? kas_order_relax_kernel<3, true, false, false, false, true, true, true>
                 : k.tiles == 1 ? kas_order_relax_kernel<3, true, false, false, false, true, true>
                                : kas_order_relax_kernel<3, false, false, false, false, true, true>;
        }
      if constexpr (W <= 3 && kas_built(KAS_K_ORDER_RELAX, W)) {
        if (k.m32 || (k.c16 && k.idl)) return nullptr;
        if (k.c16) return k.verify ? kas_relax_instance<W, true, true, false>(k) : kas_relax_instance<W, false, true, false>(k);
        if (k.idl) return k.verify ? kas_relax_instance<W, true, false, true>(k) : kas_relax_instance<W, false, false, true>(k);
        return k.verify ? nullptr : kas_relax_instance<W, false, false, false>(k);   // (the gather instances: without the sampled verification only)
      }
      return nullptr;
    case KAS_K_P4_ORDER:
      if constexpr (W == 3)
        if (k.m32) {
          if (!k.idl || k.c16) return nullptr;
          return k.tiles == 2 ? kas_p4_order_kernel<3, true, false, true, true, true>
                 : k.tiles == 1 ? kas_p4_order_kernel<3, true, false, true, true> : kas_p4_order_kernel<3, false, false, true, true>;
        }
      if constexpr (W <= 3 && kas_built(KAS_K_P4_ORDER, W)) {
        if (k.m32 || (k.c16 != 0) == (k.idl != 0)) return nullptr;
        return k.c16 ? kas_p4_order_instance<W, true>(k) : kas_p4_order_instance<W, false>(k);
      }
      return nullptr;
    case KAS_K_ORDER_RELAX_WIDE:
      if constexpr ((W == 4 || W == 5) && kas_built(KAS_K_ORDER_RELAX_WIDE, W)) return kas_order_relax_wide_kernel<W>;
      return nullptr;
    case KAS_K_ORDER_TICKET:
      if constexpr (W <= 3 && kas_built(KAS_K_ORDER_TICKET, W, 4, 2)) {
        if (k.G == 1) return k.packed ? kas_order_ticket_kernel<W, 1, true> : kas_order_ticket_kernel<W, 1, false>;
        if (k.G == 2) return k.packed ? kas_order_ticket_kernel<W, 2, true> : kas_order_ticket_kernel<W, 2, false>;
      }
      if constexpr (W <= 3 && kas_built(KAS_K_ORDER_TICKET, W, 4, 4))
        if (k.G == 4) return k.packed ? kas_order_ticket_kernel<W, 4, true> : kas_order_ticket_kernel<W, 4, false>;
      return nullptr;
    case KAS_K_ORDER_WIDE:
      if constexpr ((W == 4 || W == 5) && kas_built(KAS_K_ORDER_WIDE, W)) return kas_order_wide_kernel<W>;
      return nullptr;
    case KAS_K_ORDER_ROUND:
      if constexpr (kas_built(KAS_K_ORDER_ROUND, W)) return kas_order_round_kernel<W>;
      return nullptr;
    default:
      if constexpr (W >= 3 && W <= 5 && kas_built(KAS_K_SPREAD_A, W)) {
        if (k.family == KAS_K_SPREAD_A) return kas_spread_a_kernel<W>;
        if (k.family == KAS_K_SPREAD_Q) return kas_spread_q_kernel<W>;
        if (k.family == KAS_K_SPREAD_B) return kas_spread_b_kernel<W>;
        if (k.family == KAS_K_SPREAD_P4) return kas_spread_p4_kernel<W>;
      }
      return nullptr;
  }
}
static kas_kernel_fn kas_kernel_for(const KasKernelId& k) {
  if (k.family == KAS_K_PERMUTATION) return kas_order_permutation_kernel;
  switch (k.W) {
    case 2: return kas_kernel_w<2>(k);
    case 3: return kas_kernel_w<3>(k);
    case 4: return kas_kernel_w<4>(k);
    case 5: return kas_kernel_w<5>(k);
    case 8: return kas_kernel_w<8>(k);
    default: return nullptr;
  }
}
// the families this build holds at a width class (KasLaunchIn::built)
static uint32_t kas_built_mask(int Wc, int cells16) {
  auto have = [&](int family, int c16, int idl) {
    KasKernelId k;
    k.family = family; k.W = Wc; k.c16 = c16; k.idl = idl;
    return kas_kernel_for(k) != nullptr;
  };
  return (have(KAS_K_ORDER_RELAX, 0, 0) ? KAS_BUILT_RELAX : 0u) | (have(KAS_K_ORDER_RELAX_WIDE, 0, 0) ? KAS_BUILT_RELAXW : 0u) |
         (have(KAS_K_ORDER_WIDE, 0, 0) ? KAS_BUILT_WIDE : 0u) | (have(KAS_K_FILL_SLIM, 0, 0) ? KAS_BUILT_SLIM : 0u) |
         (have(KAS_K_P4_ORDER, cells16, !cells16) ? KAS_BUILT_P4_ORDER : 0u) | (have(KAS_K_SPREAD_A, 0, 0) ? KAS_BUILT_SPREAD : 0u);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define KAS_HIP_TRY(expr)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return set_error(KAS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

// device buffer that only ever grows (plans rebuilt in place, the host path's table buffers)
struct KasBuf { void* p = nullptr; size_t cap = 0; };

// Host-path cache of a context (kas_solve_host): device buffers that only ever grow, and the plans
// of the most recent batch shapes — a caller that solves the same cluster shape again (the CLI's
// per-topic loop, a JVM calling once per topic) finds its plan byte for byte; a what-if planner that
// changes the broker sets on every call gets the least recently used plan rebuilt in place over the
// scratch it already owns.  Neither pays hipMalloc / hipFree after the first call of a shape.
struct KasCachedPlan {
  kas_plan* plan = nullptr;
  uint64_t key = 0;
  std::vector<unsigned char> desc;      // the bytes the key was computed from (compared on a hit)
  uint64_t sig = 0;                     // batch size + topic descriptors only: what-if variants of one snapshot share it
  uint64_t last_use = 0;
  uint64_t call = 0;                    // host call that last used the entry (its ranges must not evict each other)
};
struct kas_ctx {
  int device;
  hipStream_t stream;
  hipStream_t hstream[KAS_HOST_STREAMS];   // the host path's chains (upload -> solve -> download of a scenario range)
  // a call cut into scenario ranges: every upload on one stream, every download on another (copies of one direction
  // queue behind each other anyway, and the two directions only run at the same time when no stream carries both),
  // the solves on hstream[]; events hand a range from upload to solve to download
  hipStream_t hup, hdown;
  hipEvent_t hev_up[KAS_HOST_STREAMS], hev_done[KAS_HOST_STREAMS];
  std::mutex host_mu;                   // kas_solve_host calls on one context are serialised
  KasBuf hbuf[KAS_HB_BUFFERS];            // device pools, record staging, impact records, a choice and its staging, a move list, a front's classes and counts, rack records, topic records, batch records, round records (KasHostBuf, kas_host_call.h)
  std::vector<int32_t> ident_ids;       // node_id pool of a 16-bit call: node i of every scenario has id i
  uint64_t ident_stamp = 0;             // ... and which node ranges it was filled for (kas_ident_batch)
  KasCachedPlan plans[KAS_HOST_PLAN_CACHE];
  uint64_t use_clock = 0;
  uint64_t host_calls = 0, host_plan_hits = 0, host_allocs = 0;
  int lds_lane_order_ok = 0;            // the self-test passed: the relaxation form of P5 and the fill's quota draw by ds_add_rtn may run here
  int lds_lane_order_state = -1;        // 1 passed, 0 FAILED (some lane-operation came back out of lane order), -1 could not run
                                        // (allocation / launch error), -2 switched off (environment: KAS_NO_LANE_ORDER=1)
  long lds_lane_order_checked = 0;      // lane-operations checked so far (context creation + every plan creation)
};

#define KAS_TIMER_SLOTS 64

struct kas_plan {
  uint32_t full_fill = 0;               // KAS_PLAN_FULL_FILL of the last kas_plan_set_flags: no slim fill kernel
  uint32_t mid32_bits = 0;              // KAS_PLAN_NO_MID32 / KAS_PLAN_MID32 of the last kas_plan_set_flags (kas_mid32_wanted)
  uint32_t index_rows_bits = 0;         // KAS_PLAN_NO_INDEX_ROWS / KAS_PLAN_INDEX_ROWS of the last kas_plan_set_flags (kas_index_rows_wanted)
  kas_ctx* ctx;
  KasShape shape;
  int Wc;                       // instantiated width class
  int NW;                       // wavefronts per scenario workgroup of the fill kernel
  int G;                        // scenarios per wavefront of the ticket-form order kernel
  int tickets;                  // 1: ticket form of P5, 0: round form
  int fused;                    // 1: per-chunk histograms in the fill (KasShape::fused_ok), see kas_resolve_launch
  uint32_t flags;               // KAS_FLAG_*
  KasLds lds, lds_fused;
  int32_t n_scenarios, n_topics;
  // device copies and scratch owned by the plan (grow-only: a plan can be rebuilt for another batch)
  KasBuf b_scen, b_topics, b_node_id, b_node_rack, b_accmask_off, b_accmask, b_orph_off, b_orph, b_perm, b_stats,
         b_ord_flag, b_sp_hist, b_sp_quota, b_sp_node, b_sp_flag, b_sp_oc, b_p4s;
  uint64_t* allocs;             // allocation counter to report to (the context's, or NULL)
  int single_topic;             // every scenario has exactly one topic
  int cells16;                  // kas_plan_create16: cur / out cells are uint16 node indices (KAS_FLAG_CELLS16 in every launch)
  int32_t sp_alloc_chunks;      // chunks per scenario the spread-fill scratch is sized for
  int32_t* h_handback = nullptr; // pinned host word the device writes: scenarios the slim fill kernel handed back in the last solve that has got that far
  int32_t* d_handback = nullptr; // ... its device address
  hipStream_t last_stream;
  int last_slot;                // timer slot of the most recent solve (-1: none yet)
  // kernel timing: event pairs recorded around every launch on the launch stream
  hipEvent_t ev_start[KAS_TIMER_SLOTS], ev_mid[KAS_TIMER_SLOTS], ev_stop[KAS_TIMER_SLOTS];
  int timer_next, timer_count;
  // impact pass (ABI v6): the work list is built at the plan's first impact call and kept until the plan is rebuilt; plans
  // that never ask own none of this
  int impact_ready = 0;
  KasImpactPlan impact;
  KasBuf b_imp_items, b_imp_merge, b_imp_base, b_imp_roff, b_imp_region;
  hipEvent_t ev_impact = nullptr;       // recorded behind the plan's last impact pass
  hipStream_t impact_stream = nullptr;
  int impact_pending = 0;               // ev_impact has been recorded
  // rack pass (kas_rack_impact_device / 16): the report table and rack_off are built and uploaded at the plan's first rack call
  // and again when a call brings another table; ev_impact is recorded again behind every rack pass
  int rack_ready = 0;
  KasRackPlan rack;
  KasBuf b_rk_rr, b_rk_off, b_rk_sums;
  int64_t node_pool_len = 0;
  int rack_host_ready = 0;              // the two below have been read back (a rack call without the batch in host memory)
  std::vector<kas_scenario_desc> rk_scen;
  std::vector<int32_t> rk_node_rack;
  // topic pass (kas_topic_impact_device / 16): the work list is built at the plan's first topic call and kept until the plan is
  // rebuilt; an event of its own, so that the pass needs no impact pass and the passes behind the impact pass see only that one
  int topics_ready = 0;
  KasTopicPlan topics;
  KasBuf b_tp_items, b_tp_merge, b_tp_roff, b_tp_region;
  hipEvent_t ev_topics = nullptr;       // recorded behind the plan's last topic pass, and again behind a choice that reads its records
  hipStream_t topics_stream = nullptr;
  int topics_pending = 0;               // ev_topics has been recorded
  // choosing on the device (kas_choose_device / 16): the size and segment tables, built at the plan's first such call
  int choose_ready = 0;
  KasChoosePlan choose;
  KasBuf b_ch_sizes, b_ch_segs;
  KasBuf b_fr_cls;                      // the classes of a front (kas_front_device / 16), allocated at the plan's first such call
  // the move list on the device (kas_moves_device / 16): the scenario and segment tables are built on the host with the plan and
  // uploaded at the plan's first such call, with the (listed scenario, item) scratch
  int moves_ready = 0;
  KasMovesPlan moves;
  KasBuf b_mv_scen, b_mv_segs, b_mv_scratch;
  hipEvent_t ev_moves = nullptr;        // recorded behind the plan's last moves pass: it reads the tables a later solve rewrites
  hipStream_t moves_stream = nullptr;
  int moves_pending = 0;
};

static int kas_buf_reserve(KasBuf* b, size_t bytes, uint64_t* allocs, const char* what) {
  if (bytes == 0) bytes = 16;
  if (bytes <= b->cap) return KAS_E_OK;
  if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
  hipError_t e = hipMalloc(&b->p, bytes);
  if (e != hipSuccess) { b->p = nullptr; return set_error(KAS_E_NOMEM, std::string(what) + ": " + hipGetErrorString(e)); }
  b->cap = bytes;
  if (allocs) *allocs += 1;
  return KAS_E_OK;
}
static void kas_buf_free(KasBuf* b) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }

#pragma GCC visibility push(default)
extern "C" {

int kas_abi_version(void) { return KAS_ABI_VERSION; }

const char* kas_strerror(int code) {
  switch (code) {
    case KAS_E_OK: return "ok";
    case KAS_E_INVALID_ARG: return "invalid argument";
    case KAS_E_HIP: return "HIP runtime error or no HIP device";
    case KAS_E_UNSUPPORTED: return "batch shape not supported by the kernels";
    case KAS_E_NOMEM: return "out of memory";
    default: return "unknown error code";
  }
}

const char* kas_status_string(int status) {
  switch (status) {
    case KAS_OK: return "OK";
    case KAS_FAIL_UNASSIGNABLE: return "partition could not be fully assigned (KAS:183-184)";
    case KAS_FAIL_RF_NOT_POSITIVE: return "replication factor is not positive (KTA:65-66)";
    case KAS_FAIL_RF_GT_BROKERS: return "replication factor exceeds available brokers (KTA:67-69)";
    case KAS_FAIL_HASH_INDEX: return "topic hashCode is Integer.MIN_VALUE: negative index (KAS:190-192)";
    case KAS_FAIL_RF_MISMATCH: return "partition with unexpected replication factor (KTA:58-60)";
    case KAS_SKIPPED: return "skipped: an earlier topic of the scenario failed";
    case KAS_FAIL_BAD_NODES: return "node table not strictly ascending / non-negative, or rack out of range";
    case KAS_FAIL_WATCHDOG: return "a wavefront polled past KAS_SPIN_BOUND without progress (internal error: the solve was abandoned instead of hanging)";
    default: return "unknown status";
  }
}

const char* kas_last_error(void) { return g_last_error.c_str(); }

// KTA:47-69 (host arithmetic): see include/kas_abi.h
int kas_resolve_replication_factor(const int32_t* partition_ids, const int32_t* list_sizes, int32_t n_partitions,
                                   int32_t desired_rf, int32_t n_brokers, kas_rf_result* res) {
  if (!res || n_partitions < 0 || (n_partitions > 0 && (!partition_ids || !list_sizes)))
    return set_error(KAS_E_INVALID_ARG, "kas_resolve_replication_factor: null argument or negative count");
  res->status = KAS_OK; res->fail_partition = -1; res->fail_list_size = -1;
  int32_t rf = desired_rf;
  for (int32_t i = 0; i < n_partitions; ++i) {
    if (rf < 0) {
      rf = list_sizes[i];                                      // KTA:55-56 (a list cannot be shorter than empty)
    } else if (desired_rf < 0 && rf != list_sizes[i]) {        // KTA:57-60
      res->status = KAS_FAIL_RF_MISMATCH; res->rf = rf;
      res->fail_partition = partition_ids[i]; res->fail_list_size = list_sizes[i];
      return 0;
    }
  }
  res->rf = rf;
  if (!(rf > 0)) res->status = KAS_FAIL_RF_NOT_POSITIVE;       // KTA:65-66
  else if (!(rf <= n_brokers)) res->status = KAS_FAIL_RF_GT_BROKERS;   // KTA:67-69
  return 0;
}

int kas_failure_text(const char* topic, int32_t status, int32_t fail_partition, int32_t rf, int32_t list_size, char* buf, int n) {
  if (!buf || n <= 0) return 0;
  buf[0] = 0;
  const std::string t = topic ? topic : "null";               // (Java prints a null String as "null")
  std::string m;
  switch (status) {
    case KAS_FAIL_UNASSIGNABLE: m = "Partition " + std::to_string(fail_partition) + " could not be fully assigned!"; break;
    case KAS_FAIL_RF_MISMATCH:
      m = "Topic " + t + " has partition " + std::to_string(fail_partition) + " with unexpected replication factor " + std::to_string(list_size);
      break;
    case KAS_FAIL_RF_NOT_POSITIVE: m = "Topic " + t + " does not have a positive replication factor!"; break;
    case KAS_FAIL_RF_GT_BROKERS: m = "Topic " + t + " has a higher replication factor (" + std::to_string(rf) + ") than available brokers!"; break;
    default: return 0;
  }
  const size_t len = m.size() < (size_t)(n - 1) ? m.size() : (size_t)(n - 1);
  memcpy(buf, m.data(), len);
  buf[len] = 0;
  return (int)len;
}

int kas_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Runs the self-test (grid workgroups x iters rounds x 64 lanes) on the context's stream, blocking; folds the outcome into
// the context: a failure is final, a run that could not happen leaves an earlier pass standing.
static void kas_lds_order_selftest(kas_ctx* c, int grid, int iters) {
  if (c->lds_lane_order_state == 0 || c->lds_lane_order_state == -2) return;
  if (const char* off = getenv("KAS_NO_LANE_ORDER")) {
    if (off[0] != 0 && off[0] != '0') { c->lds_lane_order_state = -2; c->lds_lane_order_ok = 0; return; }
  }
  unsigned int* d_bad = nullptr;
  unsigned int h_bad = 1u;
  bool ran = false;
  if (hipMalloc((void**)&d_bad, sizeof(unsigned int)) == hipSuccess) {
    if (hipMemsetAsync(d_bad, 0, sizeof(unsigned int), c->stream) == hipSuccess) {
      hipLaunchKernelGGL(kas_lds_order_selftest_kernel, dim3((unsigned)grid), dim3(256), 0, c->stream, d_bad, iters);
      ran = hipGetLastError() == hipSuccess &&
            hipMemcpyAsync(&h_bad, d_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
            hipStreamSynchronize(c->stream) == hipSuccess;
    }
    (void)hipFree(d_bad);
  }
  if (!ran) { (void)hipGetLastError(); return; }             // (state stays: -1 if it never ran, 1 if an earlier run passed)
  c->lds_lane_order_checked += (long)grid * iters * 64;
  c->lds_lane_order_state = h_bad == 0u ? 1 : 0;
  c->lds_lane_order_ok = h_bad == 0u ? 1 : 0;
}

int kas_ctx_create(int device, kas_ctx** out_ctx) {
  if (!out_ctx) return set_error(KAS_E_INVALID_ARG, "out_ctx == NULL");
  *out_ctx = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return set_error(KAS_E_HIP, "no HIP device visible: this library has no CPU path");
  if (device < 0 || device >= n) return set_error(KAS_E_INVALID_ARG, "device index out of range");
  KAS_HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  KAS_HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(KAS_E_HIP, std::string("device is ") + prop.gcnArchName +
                                    ", the kernels are built for gfx950 only");
  kas_ctx* c = new kas_ctx();
  c->device = device;
  c->stream = nullptr; c->hup = nullptr; c->hdown = nullptr;
  for (hipStream_t& h : c->hstream) h = nullptr;
  for (hipEvent_t& ev : c->hev_up) ev = nullptr;
  for (hipEvent_t& ev : c->hev_done) ev = nullptr;
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  // (hstream[]: made by the first host call that needs them, kas_host_solve_streams — round 5: a context used to create
  // all eight with itself, each took one of the process's GPU_MAX_HW_QUEUES hardware queues, and the streams of a caller
  // that never makes a host call — bench.py's eight slots — were left to share what remained: the kernel trace showed
  // two pairs of slots on one queue each, their solves serialised.  hup / hdown: kas_host_copy_streams.)
  for (hipEvent_t& ev : c->hev_up) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  for (hipEvent_t& ev : c->hev_done) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    kas_ctx_destroy(c);
    return set_error(KAS_E_HIP, hipGetErrorString(e));
  }
  // the relaxation form of P5 runs only where the LDS hands out the lanes' additions in lane order (see the kernel)
  kas_lds_order_selftest(c, 2048, 200);
  *out_ctx = c;
  return KAS_E_OK;
}

void kas_ctx_destroy(kas_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (hipStream_t h : ctx->hstream) if (h) (void)hipStreamSynchronize(h);
  if (ctx->hup) (void)hipStreamSynchronize(ctx->hup);
  if (ctx->hdown) (void)hipStreamSynchronize(ctx->hdown);
  for (KasCachedPlan& c : ctx->plans) if (c.plan) kas_plan_destroy(c.plan);
  for (int i = 0; i < KAS_HB_BUFFERS; ++i) {
    KasBuf* b = &ctx->hbuf[i];
    if (!kas_host_buf_pinned(i)) { kas_buf_free(b); continue; }
    if (b->p) (void)hipHostFree(b->p);
    b->p = nullptr; b->cap = 0;
  }
  for (hipEvent_t ev : ctx->hev_up) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : ctx->hev_done) if (ev) (void)hipEventDestroy(ev);
  if (ctx->hup) (void)hipStreamDestroy(ctx->hup);
  if (ctx->hdown) (void)hipStreamDestroy(ctx->hdown);
  for (hipStream_t h : ctx->hstream) if (h) (void)hipStreamDestroy(h);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int kas_ctx_lds_lane_order(const kas_ctx* ctx, int64_t* lane_ops_checked) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (lane_ops_checked) *lane_ops_checked = (int64_t)ctx->lds_lane_order_checked;
  return ctx->lds_lane_order_state;
}

int kas_ctx_synchronize(kas_ctx* ctx) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KAS_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return KAS_E_OK;
}

void kas_plan_destroy(kas_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  if (p->last_slot >= 0) (void)hipEventSynchronize(p->ev_stop[p->last_slot]);
  if (p->impact_pending) (void)hipEventSynchronize(p->ev_impact);
  if (p->moves_pending) (void)hipEventSynchronize(p->ev_moves);
  if (p->topics_pending) (void)hipEventSynchronize(p->ev_topics);
  for (KasBuf* b : {&p->b_tp_items, &p->b_tp_merge, &p->b_tp_roff, &p->b_tp_region}) kas_buf_free(b);
  if (p->ev_topics) (void)hipEventDestroy(p->ev_topics);
  for (KasBuf* b : {&p->b_mv_scen, &p->b_mv_segs, &p->b_mv_scratch}) kas_buf_free(b);
  if (p->ev_moves) (void)hipEventDestroy(p->ev_moves);
  for (KasBuf* b : {&p->b_imp_items, &p->b_imp_merge, &p->b_imp_base, &p->b_imp_roff, &p->b_imp_region, &p->b_ch_sizes, &p->b_ch_segs, &p->b_fr_cls,
                    &p->b_rk_rr, &p->b_rk_off, &p->b_rk_sums}) kas_buf_free(b);
  if (p->ev_impact) (void)hipEventDestroy(p->ev_impact);
  for (KasBuf* b : {&p->b_scen, &p->b_topics, &p->b_node_id, &p->b_node_rack, &p->b_accmask_off, &p->b_accmask,
                    &p->b_orph_off, &p->b_orph, &p->b_perm, &p->b_stats, &p->b_ord_flag, &p->b_sp_hist, &p->b_sp_quota,
                    &p->b_sp_node, &p->b_sp_flag, &p->b_sp_oc, &p->b_p4s})
    kas_buf_free(b);
  for (int i = 0; i < KAS_TIMER_SLOTS; ++i) {
    if (p->ev_start[i]) (void)hipEventDestroy(p->ev_start[i]);
    if (p->ev_stop[i]) (void)hipEventDestroy(p->ev_stop[i]);
    if (p->ev_mid[i]) (void)hipEventDestroy(p->ev_mid[i]);
  }
  if (p->h_handback) (void)hipHostFree(p->h_handback);
  delete p;
}

// everything the launch decisions read (kas_launch_plan.h), from the plan as it stands
static KasLaunchIn kas_plan_launch_in(const kas_plan* p) {
  KasLaunchIn in;
  in.shape = &p->shape;
  in.n_scenarios = p->n_scenarios; in.single_topic = p->single_topic; in.cells16 = p->cells16;
  in.flags = p->flags; in.index_rows_bits = p->index_rows_bits; in.mid32_bits = p->mid32_bits; in.full_fill = p->full_fill;
  in.NW = p->NW; in.G = p->G; in.fused = p->fused;
  in.lds_total = p->lds.total; in.lds_fused_total = p->lds_fused.total;
  in.lane_order_ok = p->ctx->lds_lane_order_ok; in.lane_order_state = p->ctx->lds_lane_order_state;
  in.have_p4s = p->b_p4s.p != nullptr; in.have_back_flags = p->b_sp_flag.p != nullptr;
  in.last_handback = p->h_handback ? *(volatile int32_t*)p->h_handback : 0;
  in.built = kas_built_mask(p->Wc, p->cells16);
  return in;
}

// opt every kernel this plan may launch into its dynamic LDS size: the stages the resolver can return for it (never on the launch path)
static int kas_plan_set_kernels(kas_plan* p) {
  struct Opt { kas_kernel_fn fn; uint32_t lds; };
  std::vector<Opt> opts;
  kas_enumerate_launches(kas_plan_launch_in(p), [&opts](const KasStage& st) {
    const kas_kernel_fn fn = kas_kernel_for(st.k);
    if (!fn || st.lds == 0u || st.lds > (uint32_t)KAS_LDS_LIMIT) return;   // (not in this build / nothing to opt into / can never be launched)
    for (Opt& o : opts)
      if (o.fn == fn) { if (st.lds > o.lds) o.lds = st.lds; return; }
    opts.push_back(Opt{fn, st.lds});
  });
  for (const Opt& o : opts) KAS_HIP_TRY(hipFuncSetAttribute((const void*)o.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)o.lds));
  return KAS_E_OK;
}
// scratch of the spread fill for the plan's current flags (kas_plan_create / kas_plan_set_flags, never a solve)
static int kas_plan_spread_scratch(kas_plan* p) {
  const int32_t chunks = kas_resolve_launch(kas_plan_launch_in(p)).spread_chunks;
  if (chunks > 0) {
    const size_t S = (size_t)p->n_scenarios, NM = (size_t)(p->shape.n_max > 0 ? p->shape.n_max : 1), C = (size_t)chunks;
    int rc;
    if ((rc = kas_buf_reserve(&p->b_sp_hist, 4 * S * C * (size_t)p->Wc * NM, p->allocs, "spread-fill scratch")) != KAS_E_OK ||
        (rc = kas_buf_reserve(&p->b_sp_quota, 4 * S * C * NM, p->allocs, "spread-fill scratch")) != KAS_E_OK ||
        (rc = kas_buf_reserve(&p->b_sp_node, 4 * S * 2 * NM, p->allocs, "spread-fill scratch")) != KAS_E_OK ||
        (rc = kas_buf_reserve(&p->b_sp_flag, 4 * (S + 1), p->allocs, "spread-fill scratch")) != KAS_E_OK ||
        (rc = kas_buf_reserve(&p->b_sp_oc, 4 * S * (C + 2), p->allocs, "spread-fill scratch")) != KAS_E_OK)
      return rc;
  }
  else {                                                         // (the slim fill kernel's hand-back flags: 4 B per scenario)
    const int rc = kas_buf_reserve(&p->b_sp_flag, 4 * ((size_t)p->n_scenarios + 1), p->allocs, "fill hand-back flags");
    if (rc != KAS_E_OK) return rc;
  }
  p->sp_alloc_chunks = chunks;
  return KAS_E_OK;
}

// (Re)build a plan for a batch: shape, device copies of the descriptors and node tables, scratch.  The
// plan's buffers only grow, so rebuilding for a batch of the same size allocates nothing.
static int kas_plan_build(kas_plan* p, const kas_batch_desc* batch) {
  KasShape sh;
  std::string err;
  int rc = kas_shape_batch(batch, &sh, &err, 0, 0);
  if (rc != KAS_E_OK) return set_error(rc, err);
  kas_ctx* ctx = p->ctx;
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  // a rebuilt plan may still have its last solve in flight on some stream
  if (p->last_slot >= 0) KAS_HIP_TRY(hipEventSynchronize(p->ev_stop[p->last_slot]));
  if (p->impact_pending) KAS_HIP_TRY(hipEventSynchronize(p->ev_impact));   // (its work list is about to go)
  if (p->moves_pending) KAS_HIP_TRY(hipEventSynchronize(p->ev_moves));
  if (p->topics_pending) KAS_HIP_TRY(hipEventSynchronize(p->ev_topics));   // (its work list too)
  p->topics_ready = 0; p->topics_pending = 0;
  p->impact_ready = 0; p->impact_pending = 0; p->choose_ready = 0; p->moves_ready = 0; p->moves_pending = 0;
  p->rack_ready = 0; p->rack_host_ready = 0; p->node_pool_len = batch->node_pool_len;
  kas_moves_plan_build(batch, &p->moves);
  kas_choose_plan_build(batch, &p->choose);                    // (host arithmetic over the descriptors: kas_choose_device refuses from it before any GPU work)
  p->shape = sh;
  p->Wc = sh.Wc; p->NW = sh.NW; p->G = sh.G;
  p->tickets = sh.tickets_ok; p->fused = sh.fused_ok;
  p->lds = sh.lds; p->lds_fused = sh.lds_fused;
  p->flags = 0; p->index_rows_bits = 0; p->full_fill = 0; p->mid32_bits = 0;
  // (the hand-back count of the plan's last solve stays when the plan is rebuilt in place for another batch — the host path's
  // cached plans: a what-if caller hands over fresh broker sets on every call, and whether its rows are rack-diverse is the
  // SNAPSHOT's property.  A stale count costs one launch with idle workgroups, then it is this batch's own.)
  p->n_scenarios = batch->n_scenarios; p->n_topics = batch->n_topics;
  p->single_topic = kas_batch_single_topic(batch) ? 1 : 0;
  p->sp_alloc_chunks = 0;
  p->last_stream = ctx->stream; p->last_slot = -1;
  p->timer_next = 0; p->timer_count = 0;
  if (p->lds.total > KAS_LDS_LIMIT)
    return set_error(KAS_E_UNSUPPORTED, "LDS carve-up exceeds 160 KiB at the instantiated width");
  if (!kas_minimal_ok(p->Wc, p->NW, p->G))
    return set_error(KAS_E_UNSUPPORTED, "tuning build (KAS_MINIMAL_INSTANCES): only lists 3 wide, 4 fill waves");
  // some order kernel must be able to take the batch HERE: beyond 8,191 brokers at lists <= 3 wide that is the relaxation
  // form alone, which needs the LDS lane order the context's self-test looks for (such a plan used to fail at its
  // first solve with a launch error)
  const uint32_t built = kas_built_mask(sh.Wc, p->cells16);
  if (p->cells16 && !kas_cells16_ok(sh, ctx->lds_lane_order_ok, built))   // (anything else is the caller's to widen: kas_solve_host16 does)
    return set_error(KAS_E_UNSUPPORTED, "16-bit cells: lists up to 3 wide, and a batch the relaxation form (LDS lane-order self-test passed) or the round form of the order kernel takes");
  {
    const bool relax_here = sh.relax_ok && ctx->lds_lane_order_ok && (built & KAS_BUILT_RELAX);
    if (!sh.round_fits && !sh.tickets_ok && !sh.wide_ok && !relax_here)
      return set_error(KAS_E_UNSUPPORTED,
                       sh.relax_ok ? (ctx->lds_lane_order_state == -1
                                          ? "this broker count x list width is served by the relaxation form only, and the context's LDS lane-order self-test could not run"
                                          : "this broker count x list width is served by the relaxation form only, and the context does not use it (LDS lane-order self-test failed or KAS_NO_LANE_ORDER)")
                                   : "no order kernel fits this broker count x list width (INTEGRATION.md, limits)");
  }
  hipStream_t st = ctx->stream;
  const size_t S = (size_t)batch->n_scenarios, T = (size_t)batch->n_topics, NP = (size_t)batch->node_pool_len;
  struct Up { KasBuf* b; const void* src; size_t bytes; const char* what; };
  const Up ups[] = {
      {&p->b_scen, batch->scenarios, sizeof(kas_scenario_desc) * S, "scenario descriptors"},
      {&p->b_topics, batch->topics, sizeof(kas_topic_desc) * T, "topic descriptors"},
      {&p->b_node_id, batch->node_id, sizeof(int32_t) * NP, "node ids"},
      {&p->b_node_rack, batch->node_rack, sizeof(int32_t) * NP, "node racks"},
      {&p->b_accmask_off, sh.accmask_off.data(), sizeof(int64_t) * sh.accmask_off.size(), "accept-mask offsets"},
      {&p->b_orph_off, sh.orph_off.data(), sizeof(int64_t) * sh.orph_off.size(), "orphan-list offsets"},
  };
  for (const Up& u : ups) {
    if ((rc = kas_buf_reserve(u.b, u.bytes, p->allocs, u.what)) != KAS_E_OK) return rc;
    if (u.bytes > 0) KAS_HIP_TRY(hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, st));
  }
  const size_t stats_bytes = sizeof(int64_t) * KAS_STATS_PER_SCENARIO * (S + 1);
  if ((rc = kas_buf_reserve(&p->b_accmask, sizeof(uint64_t) * (size_t)(sh.accmask_words + 1), p->allocs, "accept-mask scratch")) != KAS_E_OK ||
      (rc = kas_buf_reserve(&p->b_orph, sizeof(int32_t) * (size_t)(sh.orph_ints + 64), p->allocs, "orphan-list scratch")) != KAS_E_OK ||
      (rc = kas_buf_reserve(&p->b_perm, sizeof(int32_t) * (S + 1), p->allocs, "scenario-order scratch")) != KAS_E_OK ||
      (rc = kas_buf_reserve(&p->b_ord_flag, sizeof(int32_t) * (S + 1), p->allocs, "order-form flags")) != KAS_E_OK ||
      (rc = kas_buf_reserve(&p->b_stats, stats_bytes, p->allocs, "stats buffer")) != KAS_E_OK)
    return rc;
  KAS_HIP_TRY(hipMemsetAsync(p->b_stats.p, 0, stats_bytes, st));
  // hand-over of the first fit to kas_p4_kernel: head words + the brokers' loads, per topic
  if (sh.with_x && (rc = kas_buf_reserve(&p->b_p4s, sizeof(int32_t) * T * (size_t)(KAS_P4S_HEAD + (sh.n_max > 0 ? sh.n_max : 1)),
                                         p->allocs, "first-fit hand-over scratch")) != KAS_E_OK)
    return rc;
  if ((rc = kas_plan_spread_scratch(p)) != KAS_E_OK) return rc;
  if ((rc = kas_plan_set_kernels(p)) != KAS_E_OK) return rc;
  // descriptors are resident before the caller may free its copies
  KAS_HIP_TRY(hipStreamSynchronize(st));
  return KAS_E_OK;
}

static int kas_plan_new(kas_ctx* ctx, const kas_batch_desc* batch, uint64_t* allocs, kas_plan** out_plan, int cells16 = 0) {
  *out_plan = nullptr;
  kas_plan* p = new kas_plan();
  p->cells16 = cells16;
  memset((void*)p->ev_start, 0, sizeof(p->ev_start));
  memset((void*)p->ev_stop, 0, sizeof(p->ev_stop));
  memset((void*)p->ev_mid, 0, sizeof(p->ev_mid));
  p->ctx = ctx; p->allocs = allocs; p->last_slot = -1; p->last_stream = ctx->stream;
  if (hipSetDevice(ctx->device) != hipSuccess) { delete p; return set_error(KAS_E_HIP, "hipSetDevice failed"); }
  for (int i = 0; i < KAS_TIMER_SLOTS; ++i) {
    if (hipEventCreate(&p->ev_start[i]) != hipSuccess || hipEventCreate(&p->ev_stop[i]) != hipSuccess ||
        hipEventCreate(&p->ev_mid[i]) != hipSuccess) {
      kas_plan_destroy(p);
      return set_error(KAS_E_HIP, "hipEventCreate failed");
    }
  }
  // (the hand-back count comes back through a word of pinned host memory: no copy, no synchronisation; without it the launch
  // behind the slim kernel keeps its small grid)
  if (hipHostMalloc((void**)&p->h_handback, sizeof(int32_t), hipHostMallocMapped) == hipSuccess) {
    *p->h_handback = 0;
    if (hipHostGetDevicePointer((void**)&p->d_handback, p->h_handback, 0) != hipSuccess) p->d_handback = nullptr;
  } else {
    (void)hipGetLastError();
    p->h_handback = nullptr;
  }
  // (a short run of the LDS lane-order self-test again: the property is checked where and when the form is about to be used)
  if (ctx->lds_lane_order_ok) {
    KasShape pre;
    std::string err;
    if (kas_shape_batch(batch, &pre, &err, 0, 0) == KAS_E_OK && pre.relax_ok) kas_lds_order_selftest(ctx, 1024, 40);
  }
  const int rc = kas_plan_build(p, batch);
  if (rc != KAS_E_OK) { kas_plan_destroy(p); return rc; }
  *out_plan = p;
  return KAS_E_OK;
}

int kas_plan_create(kas_ctx* ctx, const kas_batch_desc* batch, kas_plan** out_plan) {
  if (!ctx || !batch || !out_plan) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  return kas_plan_new(ctx, batch, nullptr, out_plan);
}

int kas_plan_create16(kas_ctx* ctx, const kas_batch_desc* batch, kas_plan** out_plan) {
  if (!ctx || !batch || !out_plan) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::vector<int32_t> ids;
  kas_batch_desc ib;
  std::string err;
  const int rc = kas_ident_batch(batch, &ids, &ib, nullptr, &err);
  if (rc != KAS_E_OK) return set_error(rc, err);
  return kas_plan_new(ctx, &ib, nullptr, out_plan, 1);
}

int kas_plan_describe(const kas_plan* p, char* buf, int n) {
  if (!p || !buf || n <= 0) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  const int len = snprintf(buf, (size_t)n, "%s", kas_describe_launch(kas_resolve_launch(kas_plan_launch_in(p))).c_str());
  return len < n ? len : n - 1;
}

int64_t kas_plan_algorithmic_bytes(const kas_plan* plan) {
  if (!plan) return -1;
  return plan->cells16 ? plan->shape.algorithmic_bytes16 : plan->shape.algorithmic_bytes;   // (the plan's own cell width)
}

// the 16-bit side of a host call (nullptr members: the int32 call)
struct KasCells16 {
  const uint16_t* cur = nullptr;
  uint16_t* out = nullptr;
};
// a kas_tables16 as the kas_tables the kernels and the host path take: everything but the cells is the int32 call's (the kernels
// take the cell width from KAS_FLAG_CELLS16, the host path from `c16`)
static kas_tables kas_tables_of16(const kas_tables16* t16, KasCells16* c16) {
  kas_tables t;
  memset(&t, 0, sizeof(t));
  t.aux = t16->aux; t.ctx = t16->ctx; t.topic_results = t16->topic_results; t.scenario_results = t16->scenario_results;
  t.cur_len = t16->cur_len; t.out_len = t16->out_len; t.aux_len = t16->aux_len; t.ctx_len = t16->ctx_len;
  if (c16) { c16->cur = t16->cur; c16->out = t16->out; }
  else { t.cur = reinterpret_cast<const int32_t*>(t16->cur); t.out = reinterpret_cast<int32_t*>(t16->out); }
  return t;
}

static int kas_solve_device_impl(kas_plan* p, const kas_tables* t, void* hip_stream);

int kas_solve_device(kas_plan* p, const kas_tables* t, void* hip_stream) {
  if (!p || !t) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 is solved by kas_solve_device16");
  return kas_solve_device_impl(p, t, hip_stream);
}

int kas_solve_device16(kas_plan* p, const kas_tables16* t16, void* hip_stream) {
  if (!p || !t16) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_solve_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_solve_device_impl(p, &t, hip_stream);
}

static int kas_solve_device_impl(kas_plan* p, const kas_tables* t, void* hip_stream) {
  if (p->n_scenarios == 0) return KAS_E_OK;
  if (!t->out || !t->topic_results || !t->scenario_results || (p->shape.cur_need > 0 && !t->cur) ||
      (p->shape.aux_need > 0 && !t->aux) || (p->shape.ctx_need > 0 && !t->ctx))
    return set_error(KAS_E_INVALID_ARG, "a table the descriptors refer to is NULL");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : p->ctx->stream;
  KasLaunch a;
  a.scen = (const kas_scenario_desc*)p->b_scen.p; a.topics = (const kas_topic_desc*)p->b_topics.p;
  a.node_id = (const int32_t*)p->b_node_id.p; a.node_rack = (const int32_t*)p->b_node_rack.p;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.ctx = t->ctx;
  a.topic_results = t->topic_results; a.scenario_results = t->scenario_results;
  a.accmask = (uint64_t*)p->b_accmask.p; a.accmask_off = (const int64_t*)p->b_accmask_off.p;
  a.stats = (int64_t*)p->b_stats.p;
  a.orph = (int32_t*)p->b_orph.p; a.orph_off = (const int64_t*)p->b_orph_off.p;
  a.perm = nullptr;
  a.ord_flag = (int32_t*)p->b_ord_flag.p;
  // the plan's scratch serves one solve at a time: order this solve behind the previous one
  if (p->last_slot >= 0 && p->last_stream != st)
    KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->impact_pending && p->impact_stream != st)           // (... and behind an impact pass that reads the tables it rewrites)
    KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_impact, 0));
  if (p->moves_pending && p->moves_stream != st)             // (... and a moves pass: the same)
    KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_moves, 0));
  if (p->topics_pending && p->topics_stream != st)           // (... and a topic pass: the same)
    KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_topics, 0));
  p->last_stream = st;
  a.n_scenarios = p->n_scenarios; a.n_max = p->shape.n_max;
  a.idmap_entries = p->shape.idmap_entries; a.need_bsearch = p->shape.need_bsearch;
  a.p4s = (int32_t*)p->b_p4s.p;
  a.sp_hist = nullptr; a.sp_quota = nullptr; a.sp_node = nullptr; a.sp_flag = nullptr; a.sp_oc = nullptr; a.sp_chunks = 0;
  a.handback = nullptr;
  // which kernels, on which grids, with which launch words: kas_resolve_launch (kas_launch_plan.h); nothing is chosen here
  const KasResolvedLaunch L = kas_resolve_launch(kas_plan_launch_in(p));
  const int slot = p->timer_next;
  if (L.spread_chunks != p->sp_alloc_chunks)
    return set_error(KAS_E_INVALID_ARG, "internal: spread-fill scratch not sized for this plan state");
  KAS_HIP_TRY(hipEventRecord(p->ev_start[slot], st));
  if (L.spread_chunks > 0) {
    KAS_HIP_TRY(hipMemsetAsync(p->b_sp_flag.p, 0, 4 * ((size_t)p->n_scenarios + 1), st));
    KAS_HIP_TRY(hipMemsetAsync(p->b_sp_oc.p, 0, 4 * (size_t)p->n_scenarios * ((size_t)L.spread_chunks + 2), st));
  }
  bool order_phase = false;
  for (int32_t i = 0; i < L.n_stages; ++i) {
    const KasStage& sg = L.stages[i];
    if (sg.role >= KAS_STAGE_PERMUTATION && !order_phase) {      // the fill (+ first fit) is on the stream: the order kernels follow
      order_phase = true;
      KAS_HIP_TRY(hipEventRecord(p->ev_mid[slot], st));
      if (L.find(KAS_STAGE_ROUND_FLAGGED)) KAS_HIP_TRY(hipMemsetAsync(a.ord_flag, 0, 4 * ((size_t)p->n_scenarios + 1), st));
    }
    // (tuning builds, scripts/build_variant.sh -- -DKAS_TUNE_...: one of the two kernels alone, to see what each saturates at.
    // ORDER_ONLY: the fill runs in the plan's first solve only, and KAS_TUNE_NO_ROW_STORES keeps its mid rows in place.)
#if defined(KAS_TUNE_ORDER_ONLY)
    if ((sg.role == KAS_STAGE_SLIM || sg.role == KAS_STAGE_FILL) && p->last_slot >= 0) continue;
#endif
#if defined(KAS_TUNE_SKIP_ORDER)
    if (sg.role == KAS_STAGE_ORDER) continue;
#endif
    const kas_kernel_fn fn = kas_kernel_for(sg.k);
    if (!fn) return set_error(KAS_E_UNSUPPORTED, "internal: " + kas_kernel_name(sg.k) + " is not an instance of this build");
    KasLaunch b = a;
    b.flags = sg.flags;
    b.perm = sg.perm ? (int32_t*)p->b_perm.p : nullptr;
    b.sp_flag = sg.sp_flag == KAS_SP_FLAG_PLAN ? (int32_t*)p->b_sp_flag.p : (sg.sp_flag == KAS_SP_FLAG_ORD ? a.ord_flag : nullptr);
    if (sg.spread) {
      b.sp_hist = (int32_t*)p->b_sp_hist.p; b.sp_quota = (int32_t*)p->b_sp_quota.p; b.sp_node = (int32_t*)p->b_sp_node.p;
      b.sp_oc = (int32_t*)p->b_sp_oc.p; b.sp_chunks = L.spread_chunks;
    }
    if (sg.handback) b.handback = p->d_handback;
    hipLaunchKernelGGL(fn, dim3(sg.grid_x, sg.grid_y), dim3(sg.block), (size_t)sg.lds, st, b);
    KAS_HIP_TRY(hipGetLastError());
  }
  KAS_HIP_TRY(hipEventRecord(p->ev_stop[slot], st));
  p->last_slot = slot;
  p->timer_next = (slot + 1) % KAS_TIMER_SLOTS;
  if (p->timer_count < KAS_TIMER_SLOTS) p->timer_count += 1;
  return KAS_E_OK;
}

// ---- the impact pass (ABI v6; kernels: kas_impact.hip) ----------------------------------------------------------------
// The plan's work list: built at its first impact call from the batch in host memory (`hb`, the host path's slice) or, without
// one, from the descriptors the plan holds on the device (read back once), uploaded, and kept until the plan is rebuilt.
static int kas_impact_prepare(kas_plan* p, const kas_batch_desc* hb) {
  if (p->impact_ready) return KAS_E_OK;
  std::vector<kas_scenario_desc> sc;
  std::vector<kas_topic_desc> tp;
  kas_batch_desc b;
  memset(&b, 0, sizeof(b));
  if (hb) {
    b = *hb;
  } else {
    sc.resize((size_t)p->n_scenarios); tp.resize((size_t)p->n_topics);
    if (!sc.empty()) KAS_HIP_TRY(hipMemcpy(sc.data(), p->b_scen.p, sizeof(kas_scenario_desc) * sc.size(), hipMemcpyDeviceToHost));
    if (!tp.empty()) KAS_HIP_TRY(hipMemcpy(tp.data(), p->b_topics.p, sizeof(kas_topic_desc) * tp.size(), hipMemcpyDeviceToHost));
    b.n_scenarios = p->n_scenarios; b.n_topics = p->n_topics; b.scenarios = sc.data(); b.topics = tp.data();
  }
  KasImpactPlan& ip = p->impact;
  kas_impact_plan_build(&b, p->shape.n_max, p->shape.idmap_entries, p->shape.need_bsearch, p->cells16, -1, kas_impact_rows_per_item(&b), &ip);
  struct Up { KasBuf* b; const void* src; size_t bytes; const char* what; };
  const Up ups[] = {
      {&p->b_imp_items, ip.items.data(), sizeof(KasImpactItem) * ip.items.size(), "impact work list"},
      {&p->b_imp_merge, ip.merge_scen.data(), sizeof(int32_t) * ip.merge_scen.size(), "impact merge list"},
      {&p->b_imp_base, ip.node_base.data(), sizeof(int64_t) * ip.node_base.size(), "impact record offsets"},
      {&p->b_imp_roff, ip.region_off.data(), sizeof(int64_t) * ip.region_off.size(), "impact counter offsets"},
  };
  int rc;
  for (const Up& u : ups) {
    if ((rc = kas_buf_reserve(u.b, u.bytes, p->allocs, u.what)) != KAS_E_OK) return rc;
    if (u.bytes > 0) KAS_HIP_TRY(hipMemcpy(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice));
  }
  if ((rc = kas_buf_reserve(&p->b_imp_region, sizeof(int32_t) * (size_t)(ip.region_ints + 1), p->allocs, "impact counters")) != KAS_E_OK)
    return rc;
  if (!p->ev_impact) KAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_impact, hipEventDisableTiming));
  p->impact_ready = 1;
  return KAS_E_OK;
}

// The impact of the plan's previous solve, from the tables `t` it used, into `imp` (device pointers), on `st`.
static int kas_impact_impl(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, hipStream_t st, const kas_batch_desc* hb) {
  if (p->n_scenarios == 0) return KAS_E_OK;
  if (!imp->scenarios || !t->out || !t->topic_results || (p->shape.cur_need > 0 && !t->cur) || (p->shape.aux_need > 0 && !t->aux))
    return set_error(KAS_E_INVALID_ARG, "a table the impact pass reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc = kas_impact_prepare(p, hb);
  if (rc != KAS_E_OK) return rc;
  const KasImpactPlan& ip = p->impact;
  if (ip.nodes_total > 0 && !imp->nodes) return set_error(KAS_E_INVALID_ARG, "kas_impact_tables.nodes == NULL");
  // ordered behind the plan's previous solve, and behind its previous impact pass (the counters are the plan's)
  if (p->last_slot >= 0 && p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->impact_pending && p->impact_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_impact, 0));
  if (ip.region_ints > 0) KAS_HIP_TRY(hipMemsetAsync(p->b_imp_region.p, 0, sizeof(int32_t) * (size_t)ip.region_ints, st));
  KasImpactLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = (const kas_scenario_desc*)p->b_scen.p; a.topics = (const kas_topic_desc*)p->b_topics.p;
  a.node_id = (const int32_t*)p->b_node_id.p;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.items = (const KasImpactItem*)p->b_imp_items.p; a.merge_scen = (const int32_t*)p->b_imp_merge.p;
  a.node_base = (const int64_t*)p->b_imp_base.p; a.region_off = (const int64_t*)p->b_imp_roff.p;
  a.region = (int32_t*)p->b_imp_region.p;
  a.nodes = imp->nodes; a.scenarios = imp->scenarios;
  a.n_items = (int32_t)ip.items.size(); a.n_merge = (int32_t)ip.merge_scen.size();
  a.node_cap = ip.node_cap; a.idmap_entries = p->shape.idmap_entries;
  a.off_look = ip.off_look; a.off_red = ip.off_red; a.lds_bytes = ip.lds_bytes;
  a.cells16 = p->cells16;
  const int e = kas_impact_launch(&a, p->Wc, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("impact pass: ") + hipGetErrorString((hipError_t)e));
  KAS_HIP_TRY(hipEventRecord(p->ev_impact, st));
  p->impact_stream = st;
  p->impact_pending = 1;
  return KAS_E_OK;
}

int kas_impact_device(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, void* hip_stream) {
  if (!p || !t || !imp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_impact_device16");
  return kas_impact_impl(p, t, imp, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr);
}

int kas_impact_device16(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, void* hip_stream) {
  if (!p || !t16 || !imp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_impact_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_impact_impl(p, &t, imp, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr);
}

// ---- the rack pass (kernels: kas_racks.hip) -----------------------------------------------------------------------------
// The rack impact of the plan's previous solve and impact pass, from the tables `t` and the records `imp` (device pointers),
// into rk->racks / rk->scenarios (device pointers), on `st`.  report: the caller's table in host memory or NULL; hb: the
// plan's batch in host memory (the host path's slice) or NULL (the descriptors and node_rack are then read back once).
// rk->rack_off (host memory, may be NULL) gets the plan's prefix sums.
static int kas_rack_impl(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const int32_t* report, const kas_rack_tables* rk,
                         hipStream_t st, const kas_batch_desc* hb) {
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  kas_batch_desc b;
  memset(&b, 0, sizeof(b));
  if (hb) {
    b = *hb;
  } else {
    if (!p->rack_host_ready) {
      p->rk_scen.resize((size_t)p->n_scenarios); p->rk_node_rack.resize((size_t)p->node_pool_len);
      if (!p->rk_scen.empty()) KAS_HIP_TRY(hipMemcpy(p->rk_scen.data(), p->b_scen.p, sizeof(kas_scenario_desc) * p->rk_scen.size(), hipMemcpyDeviceToHost));
      if (!p->rk_node_rack.empty()) KAS_HIP_TRY(hipMemcpy(p->rk_node_rack.data(), p->b_node_rack.p, sizeof(int32_t) * p->rk_node_rack.size(), hipMemcpyDeviceToHost));
      p->rack_host_ready = 1;
    }
    b.n_scenarios = p->n_scenarios; b.scenarios = p->rk_scen.data();
    b.node_rack = p->rk_node_rack.data(); b.node_pool_len = p->node_pool_len;
  }
  if (report && b.node_pool_len <= 0) return set_error(KAS_E_INVALID_ARG, "report_rack: a table for a batch without nodes");
  const int32_t* table = report ? report : b.node_rack;
  const size_t NP = (size_t)(b.node_pool_len > 0 ? b.node_pool_len : 0);
  const int64_t S = p->n_scenarios;
  // the same table as the previous call's (its contents): nothing to build, nothing to upload
  const bool same = p->rack_ready && kas_rack_plan_serves(p->rack, table, b.node_pool_len);
  KasRackPlan fresh;
  if (!same) {
    std::string err;
    const int rc = kas_rack_plan_build(&b, table, p->shape.n_max, p->shape.idmap_entries, p->shape.need_bsearch, p->cells16, -1, &fresh, &err);
    if (rc != KAS_E_OK) return set_error(rc, err);
  }
  const KasRackPlan& want = same ? p->rack : fresh;
  if (rk->racks_cap < want.rack_off[(size_t)S]) return set_error(KAS_E_INVALID_ARG, "kas_rack_tables: racks_cap below the sum of the scenarios' rack counts");
  if ((S > 0 && !rk->scenarios) || (want.rack_off[(size_t)S] > 0 && !rk->racks))
    return set_error(KAS_E_INVALID_ARG, "kas_rack_tables: racks / scenarios == NULL");
  if (S > 0 && (p->last_slot < 0 || !p->impact_pending || !p->impact_ready))
    return set_error(KAS_E_INVALID_ARG, "kas_rack_impact_device: the plan has no solve and impact pass to report on");
  if (S > 0 && (!imp->scenarios || !t->out || !t->topic_results || (p->shape.cur_need > 0 && !t->cur) || (p->shape.aux_need > 0 && !t->aux) ||
                (p->impact.nodes_total > 0 && !imp->nodes)))
    return set_error(KAS_E_INVALID_ARG, "a table the rack pass reads is NULL");
  if (!same) {
    if (p->impact_pending) KAS_HIP_TRY(hipEventSynchronize(p->ev_impact));   // (an earlier rack pass may still read the tables)
    p->rack_ready = 0;
    p->rack = std::move(fresh);
    int rc;
    if ((rc = kas_buf_reserve(&p->b_rk_rr, sizeof(int32_t) * (NP + 1), p->allocs, "report rack table")) != KAS_E_OK ||
        (rc = kas_buf_reserve(&p->b_rk_off, sizeof(int64_t) * ((size_t)S + 1), p->allocs, "rack record offsets")) != KAS_E_OK ||
        (rc = kas_buf_reserve(&p->b_rk_sums, sizeof(int32_t) * KAS_RACK_SUMS * ((size_t)S + 1), p->allocs, "rack row sums")) != KAS_E_OK)
      return rc;
    if (NP > 0) KAS_HIP_TRY(hipMemcpy(p->b_rk_rr.p, p->rack.rr.data(), sizeof(int32_t) * NP, hipMemcpyHostToDevice));
    KAS_HIP_TRY(hipMemcpy(p->b_rk_off.p, p->rack.rack_off.data(), sizeof(int64_t) * ((size_t)S + 1), hipMemcpyHostToDevice));
    p->rack_ready = 1;
  }
  if (rk->rack_off) memcpy(rk->rack_off, p->rack.rack_off.data(), sizeof(int64_t) * ((size_t)S + 1));
  if (S == 0) return KAS_E_OK;
  // ordered behind the plan's previous solve and impact pass (and its previous rack pass: the sums are the plan's)
  if (p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->impact_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_impact, 0));
  KAS_HIP_TRY(hipMemsetAsync(p->b_rk_sums.p, 0, sizeof(int32_t) * KAS_RACK_SUMS * (size_t)S, st));
  const KasImpactPlan& ip = p->impact;
  KasRackLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = (const kas_scenario_desc*)p->b_scen.p; a.topics = (const kas_topic_desc*)p->b_topics.p;
  a.node_id = (const int32_t*)p->b_node_id.p;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.items = (const KasImpactItem*)p->b_imp_items.p;
  a.rr = (const int32_t*)p->b_rk_rr.p;
  a.node_base = (const int64_t*)p->b_imp_base.p; a.rack_off = (const int64_t*)p->b_rk_off.p;
  a.sums = (int32_t*)p->b_rk_sums.p;
  a.nodes = imp->nodes; a.racks = rk->racks; a.scenarios = rk->scenarios;
  a.n_items = (int32_t)ip.items.size(); a.n_scenarios = (int32_t)S;
  a.idmap_entries = p->shape.idmap_entries;
  a.off_rack = p->rack.off_rack; a.racks_in_lds = p->rack.racks_in_lds;
  a.lds_bytes = p->rack.lds_bytes; a.reduce_lds_bytes = p->rack.reduce_lds_bytes;
  a.cells16 = p->cells16;
  const int e = kas_rack_launch(&a, p->Wc, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("rack pass: ") + hipGetErrorString((hipError_t)e));
  // a later solve, impact pass or choice waits for this pass as it waits for the impact pass
  KAS_HIP_TRY(hipEventRecord(p->ev_impact, st));
  p->impact_stream = st;
  return KAS_E_OK;
}

int kas_rack_impact_device(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const int32_t* host_report_rack,
                           const kas_rack_tables* out, void* hip_stream) {
  if (!p || !t || !imp || !out) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_rack_impact_device16");
  return kas_rack_impl(p, t, imp, host_report_rack, out, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr);
}

int kas_rack_impact_device16(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const int32_t* host_report_rack,
                             const kas_rack_tables* out, void* hip_stream) {
  if (!p || !t16 || !imp || !out) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_rack_impact_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_rack_impl(p, &t, imp, host_report_rack, out, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr);
}

// ---- the topic pass (kernels: kas_topics.hip) ---------------------------------------------------------------------------
// The plan's work list: built at its first topic call from the batch in host memory (`hb`, the host path's slice) or, without
// one, from the descriptors the plan holds on the device (read back once); kept until the plan is rebuilt.  Nothing is
// uploaded or allocated before the scratch limit has been checked.
static int kas_topic_prepare(kas_plan* p, const kas_batch_desc* hb) {
  if (p->topics_ready) return KAS_E_OK;
  std::vector<kas_scenario_desc> sc;
  std::vector<kas_topic_desc> tp;
  kas_batch_desc b;
  memset(&b, 0, sizeof(b));
  if (hb) {
    b = *hb;
  } else {
    sc.resize((size_t)p->n_scenarios); tp.resize((size_t)p->n_topics);
    if (!sc.empty()) KAS_HIP_TRY(hipMemcpy(sc.data(), p->b_scen.p, sizeof(kas_scenario_desc) * sc.size(), hipMemcpyDeviceToHost));
    if (!tp.empty()) KAS_HIP_TRY(hipMemcpy(tp.data(), p->b_topics.p, sizeof(kas_topic_desc) * tp.size(), hipMemcpyDeviceToHost));
    b.n_scenarios = p->n_scenarios; b.n_topics = p->n_topics; b.scenarios = sc.data(); b.topics = tp.data();
  }
  KasTopicPlan& k = p->topics;
  kas_topic_plan_build(&b, p->shape.n_max, p->shape.idmap_entries, p->shape.need_bsearch, p->cells16, -1, kas_impact_rows_per_item(&b), &k);
  if (!kas_topic_scratch_ok(k)) return set_error(KAS_E_UNSUPPORTED, KAS_TOPIC_SCRATCH_TEXT);
  struct Up { KasBuf* b; const void* src; size_t bytes; const char* what; };
  const Up ups[] = {
      {&p->b_tp_items, k.items.data(), sizeof(KasImpactItem) * k.items.size(), "topic work list"},
      {&p->b_tp_merge, k.merge.data(), sizeof(KasTopicMerge) * k.merge.size(), "topic merge list"},
      {&p->b_tp_roff, k.region_off.data(), sizeof(int64_t) * k.region_off.size(), "topic counter offsets"},
  };
  int rc;
  for (const Up& u : ups) {
    if ((rc = kas_buf_reserve(u.b, u.bytes, p->allocs, u.what)) != KAS_E_OK) return rc;
    if (u.bytes > 0) KAS_HIP_TRY(hipMemcpy(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice));
  }
  if ((rc = kas_buf_reserve(&p->b_tp_region, sizeof(int32_t) * (size_t)(k.region_ints + 1), p->allocs, "topic counters")) != KAS_E_OK)
    return rc;
  if (!p->ev_topics) KAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_topics, hipEventDisableTiming));
  p->topics_ready = 1;
  return KAS_E_OK;
}

// The topic impact of the plan's previous solve, from the tables `t` it used, into `out` (device pointers), on `st`.
static int kas_topic_impl(kas_plan* p, const kas_tables* t, const kas_topic_impact_tables* out, hipStream_t st, const kas_batch_desc* hb) {
  const int64_t S = p->n_scenarios, T = p->n_topics;
  if ((T > 0 && !out->topics) || (S > 0 && !out->scenarios)) return set_error(KAS_E_INVALID_ARG, "kas_topic_impact_tables: topics / scenarios == NULL");
  if (T > 0 && (!t->out || !t->topic_results || (p->shape.cur_need > 0 && !t->cur) || (p->shape.aux_need > 0 && !t->aux)))
    return set_error(KAS_E_INVALID_ARG, "a table the topic pass reads is NULL");
  if (S == 0) return KAS_E_OK;
  if (p->last_slot < 0) return set_error(KAS_E_INVALID_ARG, "kas_topic_impact_device: the plan has no solve to report on");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc = kas_topic_prepare(p, hb);
  if (rc != KAS_E_OK) return rc;
  const KasTopicPlan& k = p->topics;
  // ordered behind the plan's previous solve, and behind its previous topic pass (the counters are the plan's)
  if (p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->topics_pending && p->topics_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_topics, 0));
  if (k.region_ints > 0) KAS_HIP_TRY(hipMemsetAsync(p->b_tp_region.p, 0, sizeof(int32_t) * (size_t)k.region_ints, st));
  KasTopicLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = (const kas_scenario_desc*)p->b_scen.p; a.topics = (const kas_topic_desc*)p->b_topics.p;
  a.node_id = (const int32_t*)p->b_node_id.p;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.items = (const KasImpactItem*)p->b_tp_items.p; a.merge = (const KasTopicMerge*)p->b_tp_merge.p;
  a.region_off = (const int64_t*)p->b_tp_roff.p; a.region = (int32_t*)p->b_tp_region.p;
  a.topic_out = out->topics; a.scenarios = out->scenarios;
  a.n_items = (int32_t)k.items.size(); a.n_merge = (int32_t)k.merge.size(); a.n_scenarios = (int32_t)S;
  a.idmap_entries = p->shape.idmap_entries;
  a.off_look = k.off_look; a.off_red = k.off_red; a.lds_bytes = k.lds_bytes;
  a.cells16 = p->cells16;
  const int e = kas_topic_launch(&a, p->Wc, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("topic pass: ") + hipGetErrorString((hipError_t)e));
  KAS_HIP_TRY(hipEventRecord(p->ev_topics, st));
  p->topics_stream = st;
  p->topics_pending = 1;
  return KAS_E_OK;
}

int kas_topic_impact_device(kas_plan* p, const kas_tables* t, const kas_topic_impact_tables* out, void* hip_stream) {
  if (!p || !t || !out) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_topic_impact_device16");
  return kas_topic_impl(p, t, out, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr);
}

int kas_topic_impact_device16(kas_plan* p, const kas_tables16* t16, const kas_topic_impact_tables* out, void* hip_stream) {
  if (!p || !t16 || !out) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_topic_impact_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_topic_impl(p, &t, out, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr);
}

// ---- choosing the best scenarios (kernels: kas_choose.hip) --------------------------------------------------------------
int kas_rank_device(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                    int32_t n_scenarios, const kas_choose_spec* spec, int32_t* rank, int32_t* chosen, int32_t* n_ok, void* hip_stream) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (n_scenarios < 0) return set_error(KAS_E_INVALID_ARG, "n_scenarios < 0");
  const char* bad = kas_choose_spec_error(spec, n_scenarios);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (!n_ok || (n_scenarios > 0 && (!scenario_results || !scenario_impact || !rank)) || (spec->k > 0 && !chosen))
    return set_error(KAS_E_INVALID_ARG, "kas_rank_device: an array the call reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KasChooseLaunch a;
  memset(&a, 0, sizeof(a));
  a.sr = scenario_results; a.si = scenario_impact;
  kas_choose_fill_spec(&a, spec, n_scenarios);
  a.rank = rank; a.chosen = chosen; a.n_ok = n_ok;
  const int e = kas_rank_launch(&a, hip_stream ? hip_stream : (void*)ctx->stream);
  if (e != 0) return set_error(KAS_E_HIP, std::string("kas_rank_kernel: ") + hipGetErrorString((hipError_t)e));
  return KAS_E_OK;
}

int kas_front_rank_device(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                          int32_t n_scenarios, const kas_front_spec* spec, int32_t* rank, int32_t* chosen, int32_t* counts, int32_t* scratch,
                          void* hip_stream) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (n_scenarios < 0) return set_error(KAS_E_INVALID_ARG, "n_scenarios < 0");
  const char* bad = kas_front_spec_error(spec, n_scenarios);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (!counts || (n_scenarios > 0 && (!scenario_results || !scenario_impact || !rank || !scratch)) || (spec->k > 0 && !chosen))
    return set_error(KAS_E_INVALID_ARG, "kas_front_rank_device: an array the call reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KasFrontLaunch a;
  memset(&a, 0, sizeof(a));
  a.c.sr = scenario_results; a.c.si = scenario_impact;
  kas_front_fill_spec(&a, spec, n_scenarios);
  a.c.rank = rank; a.c.chosen = chosen; a.c.n_ok = counts;       // (n_ok is counts[0])
  a.cls = scratch; a.counts = counts;
  void* st = hip_stream ? hip_stream : (void*)ctx->stream;
  int e = kas_front_mark_launch(&a, st);
  if (e == 0) e = kas_front_rank_launch(&a, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("front kernels: ") + hipGetErrorString((hipError_t)e));
  return KAS_E_OK;
}

// kas_rank_device / kas_front_rank_device with the scenario rack records as a third source of criteria.  A spec without a rack
// criterion goes to the parent entry (its kernel instances, its bytes).
int kas_rank_device_racks(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                          const kas_scenario_rack_impact* rack_scenarios, int32_t n_scenarios, const kas_choose_spec* spec, int32_t* rank,
                          int32_t* chosen, int32_t* n_ok, void* hip_stream) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (n_scenarios < 0) return set_error(KAS_E_INVALID_ARG, "n_scenarios < 0");
  const char* bad = kas_choose_spec_error_keys(spec, n_scenarios, true);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (!kas_choose_spec_uses_racks(spec))
    return kas_rank_device(ctx, scenario_results, scenario_impact, n_scenarios, spec, rank, chosen, n_ok, hip_stream);
  if (!rack_scenarios) return set_error(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
  if (!n_ok || (n_scenarios > 0 && (!scenario_results || !scenario_impact || !rank)) || (spec->k > 0 && !chosen))
    return set_error(KAS_E_INVALID_ARG, "kas_rank_device: an array the call reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KasRackChooseLaunch a;
  memset(&a, 0, sizeof(a));
  a.c.sr = scenario_results; a.c.si = scenario_impact; a.srk = rack_scenarios;
  kas_choose_fill_spec(&a.c, spec, n_scenarios);
  a.c.rank = rank; a.c.chosen = chosen; a.c.n_ok = n_ok;
  const int e = kas_rank_racks_launch(&a, hip_stream ? hip_stream : (void*)ctx->stream);
  if (e != 0) return set_error(KAS_E_HIP, std::string("kas_rank_racks_kernel: ") + hipGetErrorString((hipError_t)e));
  return KAS_E_OK;
}

int kas_front_rank_device_racks(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                                const kas_scenario_rack_impact* rack_scenarios, int32_t n_scenarios, const kas_front_spec* spec,
                                int32_t* rank, int32_t* chosen, int32_t* counts, int32_t* scratch, void* hip_stream) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (n_scenarios < 0) return set_error(KAS_E_INVALID_ARG, "n_scenarios < 0");
  const char* bad = kas_front_spec_error_keys(spec, n_scenarios, true);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (!kas_front_spec_uses_racks(spec))
    return kas_front_rank_device(ctx, scenario_results, scenario_impact, n_scenarios, spec, rank, chosen, counts, scratch, hip_stream);
  if (!rack_scenarios) return set_error(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
  if (!counts || (n_scenarios > 0 && (!scenario_results || !scenario_impact || !rank || !scratch)) || (spec->k > 0 && !chosen))
    return set_error(KAS_E_INVALID_ARG, "kas_front_rank_device: an array the call reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KasRackFrontLaunch a;
  memset(&a, 0, sizeof(a));
  a.f.c.sr = scenario_results; a.f.c.si = scenario_impact; a.srk = rack_scenarios;
  kas_front_fill_spec(&a.f, spec, n_scenarios);
  a.f.c.rank = rank; a.f.c.chosen = chosen; a.f.c.n_ok = counts;   // (n_ok is counts[0])
  a.f.cls = scratch; a.f.counts = counts;
  void* st = hip_stream ? hip_stream : (void*)ctx->stream;
  int e = kas_front_mark_racks_launch(&a, st);
  if (e == 0) e = kas_front_rank_racks_launch(&a, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("front kernels: ") + hipGetErrorString((hipError_t)e));
  return KAS_E_OK;
}

// ... and with the scenario topic records as a fourth.  A spec without a topic criterion goes to the *_racks entry (which sends
// one without a rack criterion on to the oldest entry): its kernel instances, its bytes.
int kas_rank_device_topics(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                           const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                           int32_t n_scenarios, const kas_choose_spec* spec, int32_t* rank, int32_t* chosen, int32_t* n_ok, void* hip_stream) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (n_scenarios < 0) return set_error(KAS_E_INVALID_ARG, "n_scenarios < 0");
  const char* bad = kas_choose_spec_error_keys(spec, n_scenarios, true, true);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (kas_choose_spec_uses_racks(spec) && !rack_scenarios) return set_error(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
  if (!kas_choose_spec_uses_topics(spec))
    return kas_rank_device_racks(ctx, scenario_results, scenario_impact, rack_scenarios, n_scenarios, spec, rank, chosen, n_ok, hip_stream);
  if (!topic_scenarios) return set_error(KAS_E_INVALID_ARG, KAS_NO_TOPIC_RECORDS);
  if (!n_ok || (n_scenarios > 0 && (!scenario_results || !scenario_impact || !rank)) || (spec->k > 0 && !chosen))
    return set_error(KAS_E_INVALID_ARG, "kas_rank_device: an array the call reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KasTopicChooseLaunch a;
  memset(&a, 0, sizeof(a));
  a.c.sr = scenario_results; a.c.si = scenario_impact; a.srk = rack_scenarios; a.stp = topic_scenarios;
  kas_choose_fill_spec(&a.c, spec, n_scenarios);
  a.c.rank = rank; a.c.chosen = chosen; a.c.n_ok = n_ok;
  const int e = kas_rank_topics_launch(&a, hip_stream ? hip_stream : (void*)ctx->stream);
  if (e != 0) return set_error(KAS_E_HIP, std::string("kas_rank_topics_kernel: ") + hipGetErrorString((hipError_t)e));
  return KAS_E_OK;
}

int kas_front_rank_device_topics(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                                 const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                                 int32_t n_scenarios, const kas_front_spec* spec, int32_t* rank, int32_t* chosen, int32_t* counts,
                                 int32_t* scratch, void* hip_stream) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  if (n_scenarios < 0) return set_error(KAS_E_INVALID_ARG, "n_scenarios < 0");
  const char* bad = kas_front_spec_error_keys(spec, n_scenarios, true, true);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (kas_front_spec_uses_racks(spec) && !rack_scenarios) return set_error(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
  if (!kas_front_spec_uses_topics(spec))
    return kas_front_rank_device_racks(ctx, scenario_results, scenario_impact, rack_scenarios, n_scenarios, spec, rank, chosen, counts, scratch,
                                       hip_stream);
  if (!topic_scenarios) return set_error(KAS_E_INVALID_ARG, KAS_NO_TOPIC_RECORDS);
  if (!counts || (n_scenarios > 0 && (!scenario_results || !scenario_impact || !rank || !scratch)) || (spec->k > 0 && !chosen))
    return set_error(KAS_E_INVALID_ARG, "kas_front_rank_device: an array the call reads or writes is NULL");
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  KasTopicFrontLaunch a;
  memset(&a, 0, sizeof(a));
  a.f.c.sr = scenario_results; a.f.c.si = scenario_impact; a.srk = rack_scenarios; a.stp = topic_scenarios;
  kas_front_fill_spec(&a.f, spec, n_scenarios);
  a.f.c.rank = rank; a.f.c.chosen = chosen; a.f.c.n_ok = counts;   // (n_ok is counts[0])
  a.f.cls = scratch; a.f.counts = counts;
  void* st = hip_stream ? hip_stream : (void*)ctx->stream;
  int e = kas_front_mark_topics_launch(&a, st);
  if (e == 0) e = kas_front_rank_topics_launch(&a, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("front kernels: ") + hipGetErrorString((hipError_t)e));
  return KAS_E_OK;
}

// The plan's size and segment tables (built on the host with the plan) on the device: allocated and uploaded at the plan's first
// choice — blocking copies, once — and kept until the plan is rebuilt.
static int kas_choose_prepare(kas_plan* p) {
  if (p->choose_ready) return KAS_E_OK;
  const KasChoosePlan& cp = p->choose;
  int rc;
  if ((rc = kas_buf_reserve(&p->b_ch_sizes, sizeof(KasChooseSize) * cp.sizes.size(), p->allocs, "choose size table")) != KAS_E_OK) return rc;
  if ((rc = kas_buf_reserve(&p->b_ch_segs, sizeof(KasChooseSeg) * cp.segs.size(), p->allocs, "choose segment table")) != KAS_E_OK) return rc;
  if (!cp.sizes.empty()) KAS_HIP_TRY(hipMemcpy(p->b_ch_sizes.p, cp.sizes.data(), sizeof(KasChooseSize) * cp.sizes.size(), hipMemcpyHostToDevice));
  if (!cp.segs.empty()) KAS_HIP_TRY(hipMemcpy(p->b_ch_segs.p, cp.segs.data(), sizeof(KasChooseSeg) * cp.segs.size(), hipMemcpyHostToDevice));
  p->choose_ready = 1;
  return KAS_E_OK;
}

// front: the Pareto front in place of the ranking (kas_front_device / 16; `spec` is then not read, `counts` is the call's).
// rack_keys: the spec may name rack criteria (the *_racks entries), read from srk, the scenario rack records of the plan's rack pass.
// topic_keys: ... and topic criteria (the *_topics entries), read from stp, the scenario topic records of the plan's topic pass.
static int kas_choose_impl(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_choose_spec* spec,
                           const kas_choice* ch, hipStream_t st, const kas_front_spec* front = nullptr, int32_t* counts = nullptr,
                           bool rack_keys = false, const kas_scenario_rack_impact* srk = nullptr, bool topic_keys = false,
                           const kas_scenario_topic_impact* stp = nullptr) {
  const int32_t S = p->n_scenarios;
  kas_choose_spec front_cs;
  if (front) {
    const char* bad = kas_front_spec_error_keys(front, S, rack_keys, topic_keys);
    if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
    front_cs = kas_front_choose_spec(front);
    spec = &front_cs;
  }
  const char* bad = kas_choose_spec_error_keys(spec, S, rack_keys, topic_keys);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  const bool by_racks = rack_keys && (front ? kas_front_spec_uses_racks(front) : kas_choose_spec_uses_racks(spec));
  if (by_racks && !srk) return set_error(KAS_E_INVALID_ARG, KAS_NO_RACK_RECORDS);
  const bool by_topics = topic_keys && (front ? kas_front_spec_uses_topics(front) : kas_choose_spec_uses_topics(spec));
  if (by_topics && !stp) return set_error(KAS_E_INVALID_ARG, KAS_NO_TOPIC_RECORDS);
  const KasChoosePlan& cp = p->choose;
  int64_t rows_need = 0, nodes_need = 0;
  kas_choose_k_largest(cp, spec->k, &rows_need, &nodes_need);
  if (ch->rows_cap < rows_need) return set_error(KAS_E_INVALID_ARG, "kas_choice: rows_cap below the packed rows of the k largest scenarios");
  if (ch->nodes_cap < nodes_need) return set_error(KAS_E_INVALID_ARG, "kas_choice: nodes_cap below the node records of the k largest scenarios");
  if ((S > 0 && !ch->rank) || (spec->k > 0 && !ch->chosen) || !ch->row_off || !ch->node_off || !ch->n_ok || (rows_need > 0 && !ch->rows) ||
      (nodes_need > 0 && !ch->nodes) || (front && !counts))
    return set_error(KAS_E_INVALID_ARG, "kas_choice: an array the call writes is NULL");
  if (S > 0 && (!t->scenario_results || !imp->scenarios || (rows_need > 0 && !t->out) || (nodes_need > 0 && !imp->nodes)))
    return set_error(KAS_E_INVALID_ARG, "a table the choice reads is NULL");
  if (S > 0 && (p->last_slot < 0 || !p->impact_pending))
    return set_error(KAS_E_INVALID_ARG, "kas_choose_device: the plan has no solve and impact pass to choose from");
  const int32_t cell = p->cells16 ? 2 : 4;
  if (((uintptr_t)ch->rows | (uintptr_t)t->out) % (uintptr_t)cell != 0 || ((uintptr_t)ch->nodes | (uintptr_t)imp->nodes) % 4 != 0 ||
      ((uintptr_t)ch->row_off | (uintptr_t)ch->node_off) % 8 != 0 || (uintptr_t)counts % 4 != 0)
    return set_error(KAS_E_INVALID_ARG, "kas_choice: rows / out must be cell-aligned, node records 4-byte aligned, the offset arrays 8-byte aligned");
  const int64_t chunks = kas_choose_chunks(cp, cell);
  if ((int64_t)spec->k * chunks > INT32_MAX) return set_error(KAS_E_UNSUPPORTED, "kas_choice: k scenarios of this size are more than one gather launch takes");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc = kas_choose_prepare(p);
  if (rc != KAS_E_OK) return rc;
  if (front && 4 * ((size_t)S + 1) > p->b_fr_cls.cap) {         // the class scratch, behind the pass that may still be using it
    if (p->impact_pending) KAS_HIP_TRY(hipEventSynchronize(p->ev_impact));
    if ((rc = kas_buf_reserve(&p->b_fr_cls, 4 * ((size_t)S + 1), p->allocs, "front classes")) != KAS_E_OK) return rc;
  }
  // ordered behind the plan's previous solve and its impact pass; a later solve waits for the gather as it waits for that pass
  if (p->last_slot >= 0 && p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->impact_pending && p->impact_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_impact, 0));
  // a choice by topic criteria reads what the plan's topic pass wrote: that pass records ev_topics, not ev_impact
  if (by_topics && p->topics_pending && p->topics_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_topics, 0));
  KasChooseLaunch a;
  memset(&a, 0, sizeof(a));
  a.sr = t->scenario_results; a.si = imp->scenarios;
  a.sizes = (const KasChooseSize*)p->b_ch_sizes.p; a.segs = (const KasChooseSeg*)p->b_ch_segs.p;
  kas_choose_fill_spec(&a, spec, S);
  a.rank = ch->rank; a.chosen = ch->chosen; a.row_off = ch->row_off; a.node_off = ch->node_off; a.n_ok = ch->n_ok;
  a.out = t->out; a.src_nodes = imp->nodes; a.rows = ch->rows; a.nodes = ch->nodes;
  a.src_cell = a.dst_cell = cell; a.chunks = (int32_t)chunks;
  int e;
  if (front) {
    KasFrontLaunch f;
    memset(&f, 0, sizeof(f));
    kas_front_fill_spec(&f, front, S);
    f.c = a;
    f.cls = (int32_t*)p->b_fr_cls.p; f.counts = counts;
    const KasRackFrontLaunch fr{f, srk};
    const KasTopicFrontLaunch ft{f, srk, stp};
    e = by_topics ? kas_front_mark_topics_launch(&ft, st) : by_racks ? kas_front_mark_racks_launch(&fr, st) : kas_front_mark_launch(&f, st);
    if (e == 0) e = by_topics ? kas_front_rank_topics_launch(&ft, st) : by_racks ? kas_front_rank_racks_launch(&fr, st) : kas_front_rank_launch(&f, st);
  } else {
    const KasRackChooseLaunch ar{a, srk};
    const KasTopicChooseLaunch at{a, srk, stp};
    e = by_topics ? kas_rank_topics_launch(&at, st) : by_racks ? kas_rank_racks_launch(&ar, st) : kas_rank_launch(&a, st);
  }
  if (e == 0) e = kas_gather_launch(&a, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("choose kernels: ") + hipGetErrorString((hipError_t)e));
  if (p->impact_pending) {
    KAS_HIP_TRY(hipEventRecord(p->ev_impact, st));
    p->impact_stream = st;
  }
  if (by_topics && p->topics_pending) {                         // (a later topic pass rewrites the records this choice reads)
    KAS_HIP_TRY(hipEventRecord(p->ev_topics, st));
    p->topics_stream = st;
  }
  return KAS_E_OK;
}

int kas_choose_device(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_choose_spec* spec, const kas_choice* ch,
                      void* hip_stream) {
  if (!p || !t || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_choose_device16");
  return kas_choose_impl(p, t, imp, spec, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

int kas_choose_device16(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const kas_choose_spec* spec, const kas_choice* ch,
                        void* hip_stream) {
  if (!p || !t16 || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_choose_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_choose_impl(p, &t, imp, spec, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

int kas_front_device(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_front_spec* spec, const kas_choice* ch,
                     int32_t* counts, void* hip_stream) {
  if (!p || !t || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_front_device16");
  if (!spec) return set_error(KAS_E_INVALID_ARG, "kas_front_spec == NULL");
  return kas_choose_impl(p, t, imp, nullptr, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, spec, counts);
}

int kas_front_device16(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const kas_front_spec* spec, const kas_choice* ch,
                       int32_t* counts, void* hip_stream) {
  if (!p || !t16 || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_front_device16 needs a plan of kas_plan_create16");
  if (!spec) return set_error(KAS_E_INVALID_ARG, "kas_front_spec == NULL");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_choose_impl(p, &t, imp, nullptr, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, spec, counts);
}

// the same four with the scenario rack records of the plan's rack pass (ordered behind it through the plan's impact event)
int kas_choose_device_racks(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                            const kas_choose_spec* spec, const kas_choice* ch, void* hip_stream) {
  if (!p || !t || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_choose_device16");
  return kas_choose_impl(p, t, imp, spec, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr, nullptr, true, srk);
}

int kas_choose_device16_racks(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                              const kas_choose_spec* spec, const kas_choice* ch, void* hip_stream) {
  if (!p || !t16 || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_choose_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_choose_impl(p, &t, imp, spec, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr, nullptr, true, srk);
}

int kas_front_device_racks(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                           const kas_front_spec* spec, const kas_choice* ch, int32_t* counts, void* hip_stream) {
  if (!p || !t || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_front_device16");
  if (!spec) return set_error(KAS_E_INVALID_ARG, "kas_front_spec == NULL");
  return kas_choose_impl(p, t, imp, nullptr, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, spec, counts, true, srk);
}

int kas_front_device16_racks(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                             const kas_front_spec* spec, const kas_choice* ch, int32_t* counts, void* hip_stream) {
  if (!p || !t16 || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_front_device16 needs a plan of kas_plan_create16");
  if (!spec) return set_error(KAS_E_INVALID_ARG, "kas_front_spec == NULL");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_choose_impl(p, &t, imp, nullptr, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, spec, counts, true, srk);
}

// ... and with the scenario topic records of the plan's topic pass as well (ordered behind it through the plan's topic event)
int kas_choose_device_topics(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                             const kas_scenario_topic_impact* stp, const kas_choose_spec* spec, const kas_choice* ch, void* hip_stream) {
  if (!p || !t || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_choose_device16");
  return kas_choose_impl(p, t, imp, spec, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr, nullptr, true, srk, true, stp);
}

int kas_choose_device16_topics(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                               const kas_scenario_topic_impact* stp, const kas_choose_spec* spec, const kas_choice* ch, void* hip_stream) {
  if (!p || !t16 || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_choose_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_choose_impl(p, &t, imp, spec, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, nullptr, nullptr, true, srk, true, stp);
}

int kas_front_device_topics(kas_plan* p, const kas_tables* t, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                            const kas_scenario_topic_impact* stp, const kas_front_spec* spec, const kas_choice* ch, int32_t* counts,
                            void* hip_stream) {
  if (!p || !t || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_front_device16");
  if (!spec) return set_error(KAS_E_INVALID_ARG, "kas_front_spec == NULL");
  return kas_choose_impl(p, t, imp, nullptr, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, spec, counts, true, srk, true, stp);
}

int kas_front_device16_topics(kas_plan* p, const kas_tables16* t16, const kas_impact_tables* imp, const kas_scenario_rack_impact* srk,
                              const kas_scenario_topic_impact* stp, const kas_front_spec* spec, const kas_choice* ch, int32_t* counts,
                              void* hip_stream) {
  if (!p || !t16 || !imp || !ch) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_front_device16 needs a plan of kas_plan_create16");
  if (!spec) return set_error(KAS_E_INVALID_ARG, "kas_front_spec == NULL");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_choose_impl(p, &t, imp, nullptr, ch, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream, spec, counts, true, srk, true, stp);
}

// ---- the move list (kernels: kas_moves.hip) ----------------------------------------------------------------------------
// the plan's scenario and segment tables on the device (the moves pass and the batches pass read them): blocking copies, once
static int kas_moves_tables_ready(kas_plan* p) {
  if (p->moves_ready) return KAS_E_OK;
  const KasMovesPlan& mp = p->moves;
  int rc;
  if ((rc = kas_buf_reserve(&p->b_mv_scen, sizeof(KasMovesScen) * mp.scen.size(), p->allocs, "moves scenario table")) != KAS_E_OK) return rc;
  if ((rc = kas_buf_reserve(&p->b_mv_segs, sizeof(KasMovesSeg) * mp.segs.size(), p->allocs, "moves segment table")) != KAS_E_OK) return rc;
  if (!mp.scen.empty()) KAS_HIP_TRY(hipMemcpy(p->b_mv_scen.p, mp.scen.data(), sizeof(KasMovesScen) * mp.scen.size(), hipMemcpyHostToDevice));
  if (!mp.segs.empty()) KAS_HIP_TRY(hipMemcpy(p->b_mv_segs.p, mp.segs.data(), sizeof(KasMovesSeg) * mp.segs.size(), hipMemcpyHostToDevice));
  if (!p->ev_moves) KAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_moves, hipEventDisableTiming));
  p->moves_ready = 1;
  return KAS_E_OK;
}

static int kas_moves_impl(kas_plan* p, const kas_tables* t, const int32_t* select, int32_t n_select, const kas_moves* mv, hipStream_t st) {
  const int32_t cell = p->cells16 ? 2 : 4;
  const char* bad = kas_moves_args_error(mv, cell);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (n_select < 0 || (n_select > 0 && !select)) return set_error(KAS_E_INVALID_ARG, "kas_moves_device: select == NULL / n_select < 0");
  if (((uintptr_t)t->cur | (uintptr_t)t->out) % (uintptr_t)cell != 0 || (uintptr_t)select % 4 != 0)
    return set_error(KAS_E_INVALID_ARG, "kas_moves_device: cur / out must be cell-aligned, select 4-byte aligned");
  const KasMovesPlan& mp = p->moves;
  bad = kas_moves_shape_error(mp, n_select);
  if (bad[0]) return set_error(KAS_E_UNSUPPORTED, bad);
  if (p->n_scenarios > 0 && (!t->out || !t->topic_results || (p->shape.cur_need > 0 && !t->cur) || (p->shape.aux_need > 0 && !t->aux)))
    return set_error(KAS_E_INVALID_ARG, "a table the moves pass reads is NULL");
  if (p->n_scenarios > 0 && p->last_slot < 0) return set_error(KAS_E_INVALID_ARG, "kas_moves_device: the plan has no solve to list the moves of");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc;
  if ((rc = kas_moves_tables_ready(p)) != KAS_E_OK) return rc;
  // the (listed scenario, item) table: sized at the first call for a list as long as the batch; a longer list grows it, behind
  // the pass that may still be using it
  const size_t entries = (size_t)(n_select > p->n_scenarios ? n_select : p->n_scenarios) * (size_t)mp.max_items + 1;
  if (sizeof(KasMovesCount) * entries > p->b_mv_scratch.cap) {
    if (p->moves_pending) KAS_HIP_TRY(hipEventSynchronize(p->ev_moves));
    if ((rc = kas_buf_reserve(&p->b_mv_scratch, sizeof(KasMovesCount) * entries, p->allocs, "moves scratch")) != KAS_E_OK) return rc;
  }
  // ordered behind the plan's previous solve and its previous moves pass (the scratch is the plan's)
  if (p->last_slot >= 0 && p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->moves_pending && p->moves_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_moves, 0));
  KasMovesLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = (const KasMovesScen*)p->b_mv_scen.p; a.segs = (const KasMovesSeg*)p->b_mv_segs.p;
  a.select = select;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.scratch = (KasMovesCount*)p->b_mv_scratch.p;
  a.move_off = mv->move_off; a.cell_off = mv->cell_off; a.moves = mv->moves; a.cells = mv->cells;
  a.moves_cap = mv->moves_cap; a.cells_cap = mv->cells_cap;
  a.n = n_select; a.stride = mp.max_items; a.S = p->n_scenarios; a.mask = mv->mask;
  a.src16 = a.dst16 = p->cells16;
  const int e = kas_moves_launch(&a, p->Wc, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("moves pass: ") + hipGetErrorString((hipError_t)e));
  KAS_HIP_TRY(hipEventRecord(p->ev_moves, st));
  p->moves_stream = st;
  p->moves_pending = 1;
  return KAS_E_OK;
}

int kas_moves_device(kas_plan* p, const kas_tables* t, const int32_t* select, int32_t n_select, const kas_moves* mv, void* hip_stream) {
  if (!p || !t || !mv) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_moves_device16");
  return kas_moves_impl(p, t, select, n_select, mv, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

int kas_moves_device16(kas_plan* p, const kas_tables16* t16, const int32_t* select, int32_t n_select, const kas_moves* mv, void* hip_stream) {
  if (!p || !t16 || !mv) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_moves_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_moves_impl(p, &t, select, n_select, mv, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

// ---- execution batches (kernel: kas_batches.hip) -------------------------------------------------------------------------
// The batches of the plan's previous solve, from the tables `t` it used, for the device list `select`, into `o` (device
// pointers), on `st`.  The pass reads the plan's moves tables and owns no scratch: it is ordered as a moves pass is.
static int kas_batches_impl(kas_plan* p, const kas_tables* t, const int32_t* select, int32_t n_select, const kas_batch_spec* sp,
                            const kas_batches* o, hipStream_t st) {
  const int32_t cell = p->cells16 ? 2 : 4;
  const char* bad = kas_batches_args_error(sp, o, n_select);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (n_select < 0 || (n_select > 0 && !select)) return set_error(KAS_E_INVALID_ARG, "kas_batches_device: select == NULL / n_select < 0");
  if (((uintptr_t)t->cur | (uintptr_t)t->out) % (uintptr_t)cell != 0 || (uintptr_t)select % 4 != 0)
    return set_error(KAS_E_INVALID_ARG, "kas_batches_device: cur / out must be cell-aligned, select 4-byte aligned");
  if (p->shape.n_max > KAS_BATCH_NODE_LIMIT) return set_error(KAS_E_UNSUPPORTED, KAS_BATCH_NODES_TEXT);
  if (!kas_batches_room_ok(n_select, o->stride)) return set_error(KAS_E_UNSUPPORTED, KAS_BATCH_ROOM_TEXT);
  if (p->n_scenarios > 0 && (!t->out || !t->topic_results || (p->shape.cur_need > 0 && !t->cur) || (p->shape.aux_need > 0 && !t->aux)))
    return set_error(KAS_E_INVALID_ARG, "a table the batches pass reads is NULL");
  if (p->n_scenarios > 0 && p->last_slot < 0) return set_error(KAS_E_INVALID_ARG, "kas_batches_device: the plan has no solve to cut the moves of");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc;
  if ((rc = kas_moves_tables_ready(p)) != KAS_E_OK) return rc;
  if (p->last_slot >= 0 && p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->moves_pending && p->moves_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_moves, 0));
  KasBatchesLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = (const KasMovesScen*)p->b_mv_scen.p; a.segs = (const KasMovesSeg*)p->b_mv_segs.p;
  a.sdesc = (const kas_scenario_desc*)p->b_scen.p; a.node_id = (const int32_t*)p->b_node_id.p;
  a.select = select;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.scenarios = o->scenarios; a.batches = o->batches; a.stride = o->stride; a.spec = *sp;
  a.n = n_select; a.S = p->n_scenarios; a.n_cap = p->shape.n_max; a.src16 = p->cells16;
  a.lds = kas_batches_lds(a.n_cap, p->Wc <= 3 ? 3 : (p->Wc <= 5 ? 5 : 8), p->cells16);
  const int e = kas_batches_launch(&a, p->Wc, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("batches pass: ") + hipGetErrorString((hipError_t)e));
  KAS_HIP_TRY(hipEventRecord(p->ev_moves, st));                 // (a later solve waits for it as for a moves pass)
  p->moves_stream = st;
  p->moves_pending = 1;
  return KAS_E_OK;
}

int kas_batches_device(kas_plan* p, const kas_tables* t, const int32_t* select, int32_t n_select, const kas_batch_spec* sp,
                       const kas_batches* o, void* hip_stream) {
  if (!p || !t || !sp || !o) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_batches_device16");
  return kas_batches_impl(p, t, select, n_select, sp, o, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

int kas_batches_device16(kas_plan* p, const kas_tables16* t16, const int32_t* select, int32_t n_select, const kas_batch_spec* sp,
                         const kas_batches* o, void* hip_stream) {
  if (!p || !t16 || !sp || !o) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_batches_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_batches_impl(p, &t, select, n_select, sp, o, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

// ---- packed rounds (kernel: kas_rounds.hip) ------------------------------------------------------------------------------
// The rounds of the plan's previous solve: kas_batches_impl with the round spec, the two strides and KAS_ROUND_NODE_LIMIT.
static int kas_rounds_impl(kas_plan* p, const kas_tables* t, const int32_t* select, int32_t n_select, const kas_round_spec* sp,
                           const kas_rounds* o, hipStream_t st) {
  const int32_t cell = p->cells16 ? 2 : 4;
  const char* bad = kas_rounds_args_error(sp, o, n_select);
  if (bad[0]) return set_error(KAS_E_INVALID_ARG, bad);
  if (n_select < 0 || (n_select > 0 && !select)) return set_error(KAS_E_INVALID_ARG, "kas_rounds_device: select == NULL / n_select < 0");
  if (((uintptr_t)t->cur | (uintptr_t)t->out) % (uintptr_t)cell != 0 || (uintptr_t)select % 4 != 0)
    return set_error(KAS_E_INVALID_ARG, "kas_rounds_device: cur / out must be cell-aligned, select 4-byte aligned");
  if (p->shape.n_max > KAS_ROUND_NODE_LIMIT) return set_error(KAS_E_UNSUPPORTED, KAS_ROUND_NODES_TEXT);
  for (int32_t s = 0; s < p->n_scenarios; ++s)                  // (the list is on the device: every scenario of the plan counts)
    if (!kas_rounds_caps_fit(sp, p->moves.scen.data(), p->moves.segs.data(), s)) return set_error(KAS_E_UNSUPPORTED, KAS_ROUND_CAPS_TEXT);
  bad = kas_rounds_room_error(n_select, o);
  if (bad[0]) return set_error(KAS_E_UNSUPPORTED, bad);
  if (p->n_scenarios > 0 && (!t->out || !t->topic_results || (p->shape.cur_need > 0 && !t->cur) || (p->shape.aux_need > 0 && !t->aux)))
    return set_error(KAS_E_INVALID_ARG, "a table the rounds pass reads is NULL");
  if (p->n_scenarios > 0 && p->last_slot < 0) return set_error(KAS_E_INVALID_ARG, "kas_rounds_device: the plan has no solve to schedule the moves of");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc;
  if ((rc = kas_moves_tables_ready(p)) != KAS_E_OK) return rc;
  if (p->last_slot >= 0 && p->last_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_stop[p->last_slot], 0));
  if (p->moves_pending && p->moves_stream != st) KAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_moves, 0));
  KasRoundsLaunch a;
  memset(&a, 0, sizeof(a));
  a.scen = (const KasMovesScen*)p->b_mv_scen.p; a.segs = (const KasMovesSeg*)p->b_mv_segs.p;
  a.sdesc = (const kas_scenario_desc*)p->b_scen.p; a.node_id = (const int32_t*)p->b_node_id.p;
  a.select = select;
  a.cur = t->cur; a.out = t->out; a.aux = t->aux; a.topic_results = t->topic_results;
  a.scenarios = o->scenarios; a.rounds = o->rounds; a.round_of = o->round_of;
  a.round_stride = o->round_stride; a.move_stride = o->move_stride; a.spec = *sp;
  a.n = n_select; a.S = p->n_scenarios; a.n_cap = p->shape.n_max; a.src16 = p->cells16;
  a.lds = kas_rounds_lds(a.n_cap, p->Wc <= 3 ? 3 : (p->Wc <= 5 ? 5 : 8), p->cells16);
  const int e = kas_rounds_launch(&a, p->Wc, st);
  if (e != 0) return set_error(KAS_E_HIP, std::string("rounds pass: ") + hipGetErrorString((hipError_t)e));
  KAS_HIP_TRY(hipEventRecord(p->ev_moves, st));                 // (a later solve waits for it as for a moves pass)
  p->moves_stream = st;
  p->moves_pending = 1;
  return KAS_E_OK;
}

int kas_rounds_device(kas_plan* p, const kas_tables* t, const int32_t* select, int32_t n_select, const kas_round_spec* sp,
                      const kas_rounds* o, void* hip_stream) {
  if (!p || !t || !sp || !o) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (p->cells16) return set_error(KAS_E_INVALID_ARG, "a plan of kas_plan_create16 takes kas_rounds_device16");
  return kas_rounds_impl(p, t, select, n_select, sp, o, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

int kas_rounds_device16(kas_plan* p, const kas_tables16* t16, const int32_t* select, int32_t n_select, const kas_round_spec* sp,
                        const kas_rounds* o, void* hip_stream) {
  if (!p || !t16 || !sp || !o) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  if (!p->cells16) return set_error(KAS_E_INVALID_ARG, "kas_rounds_device16 needs a plan of kas_plan_create16");
  const kas_tables t = kas_tables_of16(t16, nullptr);
  return kas_rounds_impl(p, &t, select, n_select, sp, o, hip_stream ? (hipStream_t)hip_stream : p->ctx->stream);
}

static int kas_plan_times(kas_plan* p, double* fill_us, double* order_us, int* launches) {
  *fill_us = 0.0; *order_us = 0.0; *launches = 0;
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  double f_ms = 0.0, o_ms = 0.0;
  int n = 0;
  for (int i = 0; i < p->timer_count; ++i) {
    int slot = (p->timer_next - 1 - i + 2 * KAS_TIMER_SLOTS) % KAS_TIMER_SLOTS;
    KAS_HIP_TRY(hipEventSynchronize(p->ev_stop[slot]));
    float ms = 0.f;
    KAS_HIP_TRY(hipEventElapsedTime(&ms, p->ev_start[slot], p->ev_mid[slot]));
    f_ms += ms;
    KAS_HIP_TRY(hipEventElapsedTime(&ms, p->ev_mid[slot], p->ev_stop[slot]));
    o_ms += ms;
    ++n;
  }
  p->timer_count = 0;
  *launches = n;
  if (n) { *fill_us = f_ms * 1000.0 / n; *order_us = o_ms * 1000.0 / n; }
  return KAS_E_OK;
}

int kas_plan_kernel_time_us(kas_plan* p, double* avg_us, int* launches) {
  if (!p || !avg_us || !launches) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  double f = 0.0, o = 0.0;
  int rc = kas_plan_times(p, &f, &o, launches);
  *avg_us = f + o;
  return rc;
}

int kas_plan_phase_times_us(kas_plan* p, double* fill_us, double* order_us, int* launches) {
  if (!p || !fill_us || !order_us || !launches) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  return kas_plan_times(p, fill_us, order_us, launches);
}

int kas_plan_set_flags(kas_plan* p, uint32_t flags) {
  if (!p) return set_error(KAS_E_INVALID_ARG, "plan == NULL");
  const int nw = (int)((flags >> 8) & 0xfu), g = (int)((flags >> 12) & 0xfu);
  if (nw != 0 && nw != 1 && nw != 2 && nw != 4)
    return set_error(KAS_E_INVALID_ARG, "KAS_PLAN_WAVES: waves per scenario must be 1, 2 or 4");
  if (g != 0 && g != 1 && g != 2 && g != 4)
    return set_error(KAS_E_INVALID_ARG, "KAS_PLAN_GROUPS: scenarios per wavefront must be 1, 2 or 4");
  if (const char* why = kas_flags_refusal(p->shape, p->cells16 != 0, flags, false)) return set_error(KAS_E_UNSUPPORTED, why);
  if (!kas_minimal_ok(p->Wc, nw ? nw : p->NW, g ? g : p->G))
    return set_error(KAS_E_UNSUPPORTED, "tuning build (KAS_MINIMAL_INSTANCES): only 4 fill waves, 1 or 2 groups");
  const KasShape& sh = p->shape;
  // (every refusal before the plan is touched: a call that returns an error leaves the plan as it was — ADVICE r4)
  KasLds l_nw = p->lds;
  if (nw != 0 && nw != p->NW) {
    l_nw = kas_fill_lds_layout(sh.n_max, sh.Wc, nw, sh.idmap_entries, sh.need_bsearch, sh.with_x);
    if (l_nw.total > KAS_LDS_LIMIT)
      return set_error(KAS_E_UNSUPPORTED, "LDS carve-up exceeds 160 KiB at that many waves");
  }
  if (g != 0 && g != p->G &&
      (kas_order_ticket_lds(sh.n_max, g, 0) > KAS_LDS_LIMIT || (int64_t)g * kas_order_ticket_group_bytes(sh.n_max, g, 0) > 65536))
    return set_error(KAS_E_UNSUPPORTED, "LDS of the order kernel exceeds 160 KiB at that many groups");
  if (nw != 0 && nw != p->NW) {
    p->lds = l_nw;
    p->NW = nw;
    KasShape tmp = sh;                                       // per-chunk histograms at the new workgroup width?
    tmp.NW = nw; tmp.lds = l_nw;
    kas_choose_fused(&tmp);
    p->fused = tmp.fused_ok; p->lds_fused = tmp.lds_fused;
  }
  if (g != 0 && g != p->G) p->G = g;
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  int rc = kas_plan_set_kernels(p);
  if (rc != KAS_E_OK) return rc;
  const KasUserFlags u = kas_user_flags(flags);
  p->index_rows_bits = u.index_rows_bits; p->mid32_bits = u.mid32_bits; p->full_fill = u.full_fill; p->flags = u.flags;
  // the spread fill's scratch follows the flags (allocated here, never inside a solve); a solve of this
  // plan may still be in flight on the old scratch
  if (kas_resolve_launch(kas_plan_launch_in(p)).spread_chunks != p->sp_alloc_chunks) {
    if (p->last_slot >= 0) KAS_HIP_TRY(hipEventSynchronize(p->ev_stop[p->last_slot]));
    if ((rc = kas_plan_spread_scratch(p)) != KAS_E_OK) return rc;
  }
  return KAS_E_OK;
}

int kas_plan_stats(kas_plan* p, int64_t* out, int64_t n) {
  if (!p || !out) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  const int64_t need = (int64_t)KAS_STATS_PER_SCENARIO * p->n_scenarios;
  if (n < need) return set_error(KAS_E_INVALID_ARG, "stats buffer too small");
  KAS_HIP_TRY(hipSetDevice(p->ctx->device));
  KAS_HIP_TRY(hipStreamSynchronize(p->last_stream));
  if (need > 0) KAS_HIP_TRY(hipMemcpy(out, p->b_stats.p, sizeof(int64_t) * (size_t)need, hipMemcpyDeviceToHost));
  return KAS_E_OK;
}

// ---------------------------------------------------------------------------------------------
// host path
// ---------------------------------------------------------------------------------------------
int kas_host_alloc(int64_t bytes, void** out_ptr) {
  if (!out_ptr || bytes < 0) return set_error(KAS_E_INVALID_ARG, "kas_host_alloc: NULL / negative size");
  *out_ptr = nullptr;
  hipError_t e = hipHostMalloc(out_ptr, (size_t)(bytes > 0 ? bytes : 16), hipHostMallocPortable);
  if (e != hipSuccess) { *out_ptr = nullptr; return set_error(KAS_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
  return KAS_E_OK;
}

void kas_host_free(void* ptr) { if (ptr) (void)hipHostFree(ptr); }

void kas_shard_range(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi) { kas_range_of(total, rank, world, lo, hi); }

int kas_batch_slice(const kas_batch_desc* b, int64_t lo, int64_t hi, kas_scenario_desc* scratch, kas_batch_desc* out,
                    const kas_tables* tables, kas_tables* tables_out) {
  std::string err;
  const int rc = kas_slice_batch(b, lo, hi, scratch, out, tables, tables_out, &err);
  return rc == KAS_E_OK ? rc : set_error(rc, err);
}

// The plan of this batch from the context's cache (kas_cache_choose): the one whose descriptors and node tables are the
// same byte for byte, else the victim rebuilt in place (or a new one into a free entry).
static int kas_host_plan(kas_ctx* ctx, const kas_batch_desc* b, kas_plan** out_plan, int cells16 = 0) {
  *out_plan = nullptr;
  if (!kas_batch_ident_ok(b)) return set_error(KAS_E_INVALID_ARG, "null/negative batch");
  const KasBatchIdent id(b, cells16);
  KasCacheEntry entries[KAS_HOST_PLAN_CACHE];
  for (int i = 0; i < KAS_HOST_PLAN_CACHE; ++i) {
    const KasCachedPlan& c = ctx->plans[i];
    entries[i] = KasCacheEntry{c.plan != nullptr, c.key, c.sig, c.last_use, c.call};
  }
  ctx->use_clock += 1;
  const KasCacheChoice choice = kas_cache_choose(entries, KAS_HOST_PLAN_CACHE, id.key, id.sig, ctx->host_calls);
  for (int i = 0; i < KAS_HOST_PLAN_CACHE; ++i) {
    KasCachedPlan& c = ctx->plans[i];
    if (!((choice.hits >> i) & 1u) || !id.same_bytes(c.desc)) continue;
    c.last_use = ctx->use_clock; c.call = ctx->host_calls;
    ctx->host_plan_hits += 1;
    *out_plan = c.plan;
    return KAS_E_OK;                                           // (its flags are the ones set below when it was built)
  }
  if (choice.victim < 0) return set_error(KAS_E_NOMEM, "host-path plan cache exhausted by one call");
  KasCachedPlan* victim = &ctx->plans[choice.victim];
  int rc;
  if (victim->plan) {
    victim->plan->cells16 = cells16;
    rc = kas_plan_build(victim->plan, b);                      // in place: its buffers are reused where they are large enough
    if (rc != KAS_E_OK) { kas_plan_destroy(victim->plan); victim->plan = nullptr; victim->desc.clear(); victim->sig = 0; return rc; }
  } else {
    kas_plan* plan = nullptr;
    rc = kas_plan_new(ctx, b, &ctx->host_allocs, &plan, cells16);
    if (rc != KAS_E_OK) return rc;
    victim->plan = plan;
  }
  id.copy_to(&victim->desc);
  victim->key = id.key; victim->sig = id.sig; victim->last_use = ctx->use_clock; victim->call = ctx->host_calls;
  // a host call blocks until its results are back: its solve has the GPU to itself (or shares it with the few other
  // scenario ranges of the same call), so the relaxation form takes double tiles whatever the batch size — the order
  // kernel of a 1000-variant what-if call 2.0 -> 1.7 ms
  // ... and its first fit runs as a wavefront of the order kernel's workgroup where that applies (kas_p4_with_order: round 6, a
  // batch of 1000 alone 2.15 ms against 2.42 ms with first fit on the fill workgroup's four wavefronts, round 5's choice — which
  // the same two bits still give every plan the new kernel does not serve: kas_split_p4 / kas_p4_with_order)
  victim->plan->flags |= KAS_FLAG_RELAX_TILES_128 | KAS_FLAG_P4_WITH_ORDER;
  *out_plan = victim->plan;
  return KAS_E_OK;
}

// grow-only buffer of the host path (KasHostBuf): device memory, or pinned host memory for the record staging
static int kas_host_reserve(kas_ctx* ctx, int id, size_t bytes) {
  KasBuf* b = &ctx->hbuf[id];
  if (bytes <= b->cap) return KAS_E_OK;
  const size_t want = bytes + bytes / 4 + 256;
  // (every host call drains its streams before it returns: nothing is in flight on the old buffer)
  if (!kas_host_buf_pinned(id)) return kas_buf_reserve(b, want, &ctx->host_allocs, "host-path buffer");
  if (b->p) (void)hipHostFree(b->p);
  b->p = nullptr; b->cap = 0;
  if (hipHostMalloc(&b->p, want, hipHostMallocDefault) != hipSuccess) { b->p = nullptr; return set_error(KAS_E_NOMEM, "hipHostMalloc failed (host-path record staging)"); }
  b->cap = want;
  ctx->host_allocs += 1;
  return KAS_E_OK;
}

// the host path's solve streams: the first n of hstream[] exist after this
static int kas_host_solve_streams(kas_ctx* c, int n) {
  for (int i = 0; i < n && i < KAS_HOST_STREAMS; ++i)
    if (!c->hstream[i]) KAS_HIP_TRY(hipStreamCreateWithFlags(&c->hstream[i], hipStreamNonBlocking));
  return KAS_E_OK;
}

// The two copy streams of a host call that is cut into scenario ranges, made on first use.  They get hardware queues
// of their own: the runtime maps ordinary streams onto a pool of GPU_MAX_HW_QUEUES (default 4) queues, and an upload
// that shares a queue with the solve of another range waits behind its kernels (a copy trace of the plain path:
// uploads in bursts of three).  A stream created with a CU mask is not pooled — the mask is a property of the queue —
// and the mask here is every CU.  Only these two: a process that holds dozens of queues is time-sliced by the
// hardware scheduler (every stream of the host path on a queue of its own, two contexts alive: configs[4]'s 35 ms
// chain kernel ran 13 % slower, configs[3]'s share fell from 590k to 341k scenarios/s).
static int kas_host_copy_streams(kas_ctx* c) {
  if (c->hup && c->hdown) return KAS_E_OK;
  hipDeviceProp_t prop;
  KAS_HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const int words = (prop.multiProcessorCount + 31) / 32;
  std::vector<uint32_t> all((size_t)words, 0xffffffffu);
  if (prop.multiProcessorCount % 32) all[(size_t)words - 1] = (1u << (prop.multiProcessorCount % 32)) - 1u;
  for (hipStream_t* st : {&c->hup, &c->hdown}) {
    if (*st) continue;
    if (hipExtStreamCreateWithCUMask(st, (uint32_t)words, all.data()) != hipSuccess) {
      (void)hipGetLastError();
      *st = nullptr;
      KAS_HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    }
  }
  return KAS_E_OK;
}

// ---- 16-bit cells at the host boundary (kas_solve_host16, include/kas_abi.h) --------------------------------------
// The solver kernels read and write int32 cells; a 16-bit call moves half the bytes over PCIe and converts on the device,
// where a cell costs 6 bytes of HBM traffic against the link's 2: KAS_CELL16_NONE <-> -1, every other value as it is.
// A thread takes 8 cells, the 16-byte side of its accesses aligned (the pools start at whatever cell the descriptors
// say; the cells before the first aligned group and behind the last go one by one).
__global__ __launch_bounds__(256) void kas_cells_widen_kernel(const uint16_t* __restrict__ in, int32_t* __restrict__ out, int64_t n) {
  const int64_t head0 = (int64_t)((16u - (uint32_t)((uintptr_t)in & 15u)) & 15u) >> 1;
  const int64_t head = head0 < n ? head0 : n;
  const int64_t groups = (n - head) >> 3;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  auto one = [&](int64_t i) { const uint32_t v = in[i]; out[i] = v == 0xffffu ? -1 : (int32_t)v; };
  for (int64_t g = tid; g < groups; g += nth) {
    const int64_t at = head + (g << 3);
    const uint4 v = *reinterpret_cast<const uint4*>(in + at);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = w[k] & 0xffffu, hi = w[k] >> 16;
      out[at + 2 * k] = lo == 0xffffu ? -1 : (int32_t)lo;
      out[at + 2 * k + 1] = hi == 0xffffu ? -1 : (int32_t)hi;
    }
  }
  for (int64_t i = tid; i < head; i += nth) one(i);
  for (int64_t i = head + (groups << 3) + tid; i < n; i += nth) one(i);
}

__global__ __launch_bounds__(256) void kas_cells_narrow_kernel(const int32_t* __restrict__ in, uint16_t* __restrict__ out, int64_t n) {
  const int64_t head0 = (int64_t)((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u) >> 1;
  const int64_t head = head0 < n ? head0 : n;
  const int64_t groups = (n - head) >> 3;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  // (a node index is below 32,768 and the pad value is -1: the low half of the cell is the 16-bit cell)
  for (int64_t g = tid; g < groups; g += nth) {
    const int64_t at = head + (g << 3);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = ((uint32_t)in[at + 2 * k] & 0xffffu) | ((uint32_t)in[at + 2 * k + 1] << 16);
    *reinterpret_cast<uint4*>(out + at) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (int64_t i = tid; i < head; i += nth) out[i] = (uint16_t)in[i];
  for (int64_t i = head + (groups << 3) + tid; i < n; i += nth) out[i] = (uint16_t)in[i];
}

static unsigned kas_cells_grid(int64_t n) {
  const int64_t g = (n / 8 + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}


// a cur / out pool of a host call as it travels: device and host base (both take the descriptors' absolute cell offsets), bytes a cell
struct KasCellPool {
  char *dev, *host;
  size_t cell;
  char* d(int64_t at) const { return dev + (int64_t)cell * at; }
  char* h(int64_t at) const { return host + (int64_t)cell * at; }
};

// One host call: plan it (kas_host_call.h: validation, cell width, offsets, scenario ranges, buffer sizes), reserve, fetch the
// ranges' plans, enqueue, drain, copy the records.
static int kas_solve_host_locked(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select,
                                 int32_t n_select, const KasCells16* c16 = nullptr, const kas_impact_tables* himp = nullptr,
                                 const kas_choose_spec* spec = nullptr, const kas_choice* hch = nullptr, const kas_moves* hmv = nullptr,
                                 bool rows_optional = false, const kas_front_spec* front = nullptr, int32_t* counts = nullptr,
                                 const kas_rack_tables* hrk = nullptr, const int32_t* report_rack = nullptr, bool rack_keys = false,
                                 bool topic_pass = false, const kas_topic_impact_tables* htp = nullptr, bool topic_keys = false,
                                 const kas_batch_spec* bsp = nullptr, const kas_batches* hbt = nullptr,
                                 const kas_round_spec* rsp = nullptr, const kas_rounds* hrd = nullptr) {
  KAS_HIP_TRY(hipSetDevice(ctx->device));
  ctx->host_calls += 1;
  KasHostCallIn in;
  in.batch = batch;
  in.cur_len = h->cur_len; in.out_len = h->out_len; in.aux_len = h->aux_len; in.ctx_len = h->ctx_len;
  in.have_cur = c16 ? c16->cur != nullptr : h->cur != nullptr;
  in.have_out = c16 ? c16->out != nullptr : h->out != nullptr;
  in.have_aux = h->aux != nullptr; in.have_ctx = h->ctx != nullptr;
  in.have_topic_results = h->topic_results != nullptr; in.have_scenario_results = h->scenario_results != nullptr;
  in.select = select; in.n_select = n_select;
  in.cells16 = c16 != nullptr; in.ident_ids = &ctx->ident_ids; in.ident_stamp = &ctx->ident_stamp;
  in.impact = himp != nullptr; in.have_imp_nodes = himp && himp->nodes; in.have_imp_scenarios = himp && himp->scenarios;
  if (hch) {                                                   // kas_solve_host_choose / 16: rows and node blocks of the chosen only
    in.choose = spec; in.rows_cap = hch->rows_cap; in.nodes_cap = hch->nodes_cap;
    in.have_ch_rank = hch->rank != nullptr; in.have_ch_chosen = hch->chosen != nullptr; in.have_ch_row_off = hch->row_off != nullptr;
    in.have_ch_node_off = hch->node_off != nullptr; in.have_ch_n_ok = hch->n_ok != nullptr;
    in.have_ch_rows = hch->rows != nullptr; in.have_ch_nodes = hch->nodes != nullptr;
  }
  if (front) {                                                 // kas_solve_host_front / 16: `spec` is the planner's (hc.ch_spec)
    in.choose = nullptr; in.front = front; in.have_fr_counts = counts != nullptr; in.ch_rows_optional = rows_optional;
  }
  if (hmv) {                                                   // kas_solve_host_moves / kas_solve_host_choose_moves / 16
    in.moves = hmv; in.ch_rows_optional = rows_optional;
    if (!hch) { in.mv_select = select; in.mv_n_select = n_select; in.select = nullptr; in.n_select = 0; select = nullptr; n_select = 0; }
  }
  in.rack_keys = rack_keys;                                    // kas_solve_host_choose_racks / kas_solve_host_front_racks / 16
  if (rack_keys) in.ch_rows_optional = rows_optional;          // (with moves or without)
  if (hrk) {                                                   // kas_solve_host_rack_impact / 16, and those
    in.racks = true; in.report_rack = report_rack; in.racks_cap = hrk->racks_cap;
    in.have_rk_racks = hrk->racks != nullptr; in.have_rk_scenarios = hrk->scenarios != nullptr; in.have_rk_off = hrk->rack_off != nullptr;
  }
  in.topic_keys = topic_keys;                                  // kas_solve_host_choose_topics / kas_solve_host_front_topics / 16
  if (topic_pass) {                                            // kas_solve_host_topic_impact / 16, and those
    in.topics = true; in.have_tp_tables = htp != nullptr;
    in.have_tp_topics = htp && htp->topics; in.have_tp_scenarios = htp && htp->scenarios;
  }
  if (hbt) {                                                   // kas_solve_host_batches / 16: no rows, the list is the call's
    in.batches = bsp; in.bt_out = hbt; in.bt_select = select; in.bt_n_select = n_select;
    in.select = nullptr; in.n_select = 0; select = nullptr; n_select = 0;
  }
  if (hrd) {                                                   // kas_solve_host_rounds / 16: the same
    in.rounds = rsp; in.rd_out = hrd; in.rd_select = select; in.rd_n_select = n_select;
    in.select = nullptr; in.n_select = 0; select = nullptr; n_select = 0;
  }
  in.lane_order_ok = ctx->lds_lane_order_ok;
  for (int Wc : {2, 3, 4, 5, 8}) in.built16[Wc] = kas_built_mask(Wc, 1);
  if (const char* e = getenv("KAS_HOST_RANGES")) in.ranges_override = atoi(e);
  KasHostCall hc;
  int rc;
  {
    std::string err;
    if ((rc = kas_plan_host_call(in, &hc, &err)) != KAS_E_OK) return set_error(rc, err);
  }
  if (front) spec = &hc.ch_spec;
  batch = &hc.batch;                                           // (a 16-bit call: node i of every scenario has the id i)
  const KasShape& full = hc.full;
  const int K = hc.K;
  const int64_t S = batch->n_scenarios;
  const bool all_rows = hc.all_rows, native16 = hc.native16, widened = c16 && !native16;
  // The result records come back through pinned staging of the context's own: the caller's record arrays are ordinary
  // (pageable) memory even when its bulk tables are pinned, and a copy to pageable memory blocks the issuing thread
  // until the stream gets there — every range's records would hold the next range's upload back until its own solve
  // has finished (a memory-copy trace of the plain path showed exactly that: uploads 2-3 ms apart).
  for (int i = 0; i < KAS_HB_BUFFERS; ++i)
    if ((rc = kas_host_reserve(ctx, i, hc.bytes[i])) != KAS_E_OK) return rc;
  // device pools: the pointers are rebased so that the descriptors' absolute offsets apply (nullptr: not this call's)
  auto rebased = [&](int id, int64_t cell, int64_t lo) { return hc.bytes[id] ? (char*)ctx->hbuf[id].p - cell * lo : nullptr; };
  int32_t* d_cur = (int32_t*)rebased(KAS_HB_CUR, 4, full.cur_lo);
  int32_t* d_out = (int32_t*)rebased(KAS_HB_OUT, 4, full.out_lo);
  uint16_t* d_cur16 = (uint16_t*)rebased(KAS_HB_CUR16, 2, full.cur_lo);
  uint16_t* d_out16 = (uint16_t*)rebased(KAS_HB_OUT16, 2, full.out_lo);
  int32_t* d_aux = (int32_t*)rebased(KAS_HB_AUX, 4, full.aux_lo);
  int32_t* d_ctx = (int32_t*)rebased(KAS_HB_CTX, 4, full.ctx_lo);
  kas_topic_result* d_tr = (kas_topic_result*)ctx->hbuf[KAS_HB_TR].p;
  kas_scenario_result* d_sr = (kas_scenario_result*)ctx->hbuf[KAS_HB_SR].p;
  kas_topic_result* p_tr = (kas_topic_result*)ctx->hbuf[KAS_HB_TR_PIN].p;
  kas_scenario_result* p_sr = (kas_scenario_result*)ctx->hbuf[KAS_HB_SR_PIN].p;
  // 16-bit cells travel through the 16-bit pools whatever they are solved on
  const KasCellPool cur = c16 ? KasCellPool{(char*)d_cur16, (char*)c16->cur, 2} : KasCellPool{(char*)d_cur, (char*)h->cur, 4};
  const KasCellPool out = c16 ? KasCellPool{(char*)d_out16, (char*)c16->out, 2} : KasCellPool{(char*)d_out, (char*)h->out, 4};

  kas_plan* plans[KAS_HOST_STREAMS];
  for (int i = 0; i < K; ++i) {
    rc = kas_host_plan(ctx, &hc.ranges[(size_t)i].bd, &plans[i], native16 ? 1 : 0);
    if (rc == KAS_E_UNSUPPORTED && native16)                   // (cannot happen: a range's shape is a part of the batch's)
      return set_error(KAS_E_UNSUPPORTED, "internal: a scenario range of a batch the 16-bit kernels take was refused by them: " + g_last_error);
    if (rc != KAS_E_OK) return rc;
  }

  // ---- enqueue.  From here on every exit drains the streams first.
  if ((rc = kas_host_solve_streams(ctx, K)) != KAS_E_OK) return rc;
  hipStream_t s0 = ctx->hstream[0];
  hipError_t he = hipSuccess;
  int fail_rc = KAS_E_OK;
  auto hip_ok = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && he == hipSuccess) { he = e; fail_rc = set_error(KAS_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    return he == hipSuccess;
  };
  // every stream is drained whatever happened; an error that only surfaces at a synchronisation (a kernel fault, a
  // failed copy) is the call's error: the caller must never read out / ctx / records of a solve that did not finish
  if (K > 1 && (rc = kas_host_copy_streams(ctx)) != KAS_E_OK) return rc;
  auto drain = [&]() {
    for (hipStream_t st : ctx->hstream) if (st) hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (ctx->hup) hip_ok(hipStreamSynchronize(ctx->hup), "hipStreamSynchronize");
    if (ctx->hdown) hip_ok(hipStreamSynchronize(ctx->hdown), "hipStreamSynchronize");
  };
  // one range: everything on s0.  Several: uploads on hup, solves on hstream[i], downloads on hdown.
  hipStream_t s_up = K > 1 ? ctx->hup : s0, s_down = K > 1 ? ctx->hdown : s0;
  // a widened call: int32 cells from / to the 16-bit ones, on the stream that solves (the copy streams only copy)
  auto widen = [&](hipStream_t st, int64_t at, int64_t n) {
    hipLaunchKernelGGL(kas_cells_widen_kernel, dim3(kas_cells_grid(n)), dim3(256), 0, st, d_cur16 + at, d_cur + at, n);
    return hip_ok(hipGetLastError(), "kas_cells_widen_kernel");
  };
  // (into the staging buffer, not into the caller's pinned pool: the kernel's stores over the link ran at 20 GB/s —
  // a call of 240 scenarios 10.5 ms against 8.4 ms with the copy engine, experiments/README.md)
  auto narrow = [&](hipStream_t st, int64_t at, int64_t n) {
    hipLaunchKernelGGL(kas_cells_narrow_kernel, dim3(kas_cells_grid(n)), dim3(256), 0, st, d_out + at, d_out16 + at, n);
    return hip_ok(hipGetLastError(), "kas_cells_narrow_kernel");
  };
  auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st, const char* what) {
    return hip_ok(hipMemcpyAsync(dst, src, bytes, kind, st), what);
  };
  const KasExtent aux_x{full.aux_lo, full.aux_need}, ctx_x{full.ctx_lo, full.ctx_need};
  // pools every range reads (aux, Context) go up first (the ranges' own uploads queue behind them on the same stream)
  if (aux_x.hi > aux_x.lo) copy(d_aux + aux_x.lo, h->aux + aux_x.lo, 4 * (size_t)(aux_x.hi - aux_x.lo), hipMemcpyHostToDevice, s_up, "upload aux");
  if (ctx_x.hi > ctx_x.lo) copy(d_ctx + ctx_x.lo, h->ctx + ctx_x.lo, 4 * (size_t)(ctx_x.hi - ctx_x.lo), hipMemcpyHostToDevice, s_up, "upload ctx");
  auto download = [&](int i) {
    const KasHostRange& r = hc.ranges[(size_t)i];
    const KasExtent &o = r.own[KAS_POOL_OUT], &t = r.own[KAS_POOL_TOPICS];
    if (K > 1) hip_ok(hipStreamWaitEvent(s_down, ctx->hev_done[i], 0), "wait");
    if (all_rows && o.hi > o.lo) copy(out.h(o.lo), out.d(o.lo), out.cell * (size_t)(o.hi - o.lo), hipMemcpyDeviceToHost, s_down, "download out");
    if (t.hi > t.lo) copy(p_tr + t.lo, d_tr + t.lo, sizeof(kas_topic_result) * (size_t)(t.hi - t.lo), hipMemcpyDeviceToHost, s_down, "download topic results");
    if (r.hi > r.lo) copy(p_sr + r.lo, d_sr + r.lo, sizeof(kas_scenario_result) * (size_t)(r.hi - r.lo), hipMemcpyDeviceToHost, s_down, "download scenario results");
  };
  // software-pipelined issue order (upload i, solve i, download i - 2): with pageable host memory the copies block
  // the issuing thread, and this order still lets the device overlap them with the solves.  (A range's solve takes
  // about as long as three uploads: behind upload i the solve of range i - 1 is still running, that of i - 2 is done —
  // a lag of one made the thread wait ~1 ms per range: 15.6 ms per call of eight ranges.)
  const int lag = K >= 3 ? 2 : 1;
  for (int i = 0; i < K && he == hipSuccess && fail_rc == KAS_E_OK; ++i) {
    const KasHostRange& r = hc.ranges[(size_t)i];
    const KasExtent &c = r.own[KAS_POOL_CUR], &o = r.own[KAS_POOL_OUT];
    hipStream_t st = K > 1 ? ctx->hstream[i % KAS_HOST_STREAMS] : s0;
    if (c.hi > c.lo) copy(cur.d(c.lo), cur.h(c.lo), cur.cell * (size_t)(c.hi - c.lo), hipMemcpyHostToDevice, s_up, "upload cur");
    if (K > 1) {
      hip_ok(hipEventRecord(ctx->hev_up[i], s_up), "record");
      hip_ok(hipStreamWaitEvent(st, ctx->hev_up[i], 0), "wait");
    }
    if (he != hipSuccess) break;
    if (widened && c.hi > c.lo && !widen(st, c.lo, c.hi - c.lo)) break;
    kas_tables d;
    memset(&d, 0, sizeof(d));
    d.cur = native16 ? reinterpret_cast<const int32_t*>(d_cur16) : d_cur;
    d.out = native16 ? reinterpret_cast<int32_t*>(d_out16) : d_out;
    d.aux = d_aux; d.ctx = d_ctx;
    d.topic_results = d_tr + r.own[KAS_POOL_TOPICS].lo; d.scenario_results = d_sr + r.lo;
    const int src = kas_solve_device_impl(plans[i], &d, st);
    if (src != KAS_E_OK) { fail_rc = src; break; }
    if (himp) {                                                // the impact pass on the range's solve stream, behind its solve
      kas_impact_tables di;
      di.nodes = (kas_node_impact*)ctx->hbuf[KAS_HB_IMP_NODES].p + hc.imp_base[(size_t)r.lo];
      di.scenarios = (kas_scenario_impact*)ctx->hbuf[KAS_HB_IMP_SCEN].p + r.lo;
      const int irc = kas_impact_impl(plans[i], &d, &di, st, &r.bd);
      if (irc != KAS_E_OK) { fail_rc = irc; break; }
      if (hrk) {                                               // ... and the rack pass right behind it
        kas_rack_tables dr;
        dr.racks = (kas_rack_impact*)ctx->hbuf[KAS_HB_RK_RACKS].p + hc.rack.rack_off[(size_t)r.lo];
        dr.scenarios = (kas_scenario_rack_impact*)ctx->hbuf[KAS_HB_RK_SCEN].p + r.lo;
        dr.rack_off = nullptr; dr.racks_cap = INT64_MAX;
        const int32_t* rep = report_rack && r.bd.node_rack ? report_rack + (r.bd.node_rack - batch->node_rack) : nullptr;
        const int rrc = kas_rack_impl(plans[i], &d, &di, rep, &dr, st, &r.bd);
        if (rrc != KAS_E_OK) { fail_rc = rrc; break; }
      }
    }
    if (topic_pass) {                                          // the topic pass on the range's solve stream, behind its solve
      kas_topic_impact_tables dt;
      dt.topics = (kas_topic_impact*)ctx->hbuf[KAS_HB_TP_TOPICS].p + r.own[KAS_POOL_TOPICS].lo;
      dt.scenarios = (kas_scenario_topic_impact*)ctx->hbuf[KAS_HB_TP_SCEN].p + r.lo;
      const int trc = kas_topic_impl(plans[i], &d, &dt, st, &r.bd);
      if (trc != KAS_E_OK) { fail_rc = trc; break; }
    }
    if (widened && all_rows && o.hi > o.lo && !narrow(st, o.lo, o.hi - o.lo)) break;
    if (K > 1) hip_ok(hipEventRecord(ctx->hev_done[i], st), "record");
    if (i >= lag) download(i - lag);
  }
  for (int i = K - lag < 0 ? 0 : K - lag; i < K && he == hipSuccess && fail_rc == KAS_E_OK; ++i) download(i);
  // a choice: rank and gather on s0 behind every range (one range: s0 solved it; several: their done events, which are recorded
  // behind a range's rack pass and its topic pass: a ranking by rack or topic criteria sees every range's records), then its header
  const int64_t ch_k = hch ? spec->k : 0;
  char* const d_head = (char*)ctx->hbuf[KAS_HB_CH_HEAD].p;
  char* const p_head = (char*)ctx->hbuf[KAS_HB_CH_HEAD_PIN].p;
  if (hch && he == hipSuccess && fail_rc == KAS_E_OK) {
    const KasChoosePlan& cp = hc.choose;
    if (!cp.sizes.empty()) copy(ctx->hbuf[KAS_HB_CH_SIZES].p, cp.sizes.data(), sizeof(KasChooseSize) * cp.sizes.size(), hipMemcpyHostToDevice, s0, "upload size table");
    if (!cp.segs.empty()) copy(ctx->hbuf[KAS_HB_CH_SEGS].p, cp.segs.data(), sizeof(KasChooseSeg) * cp.segs.size(), hipMemcpyHostToDevice, s0, "upload segment table");
    for (int i = 0; K > 1 && i < K; ++i) hip_ok(hipStreamWaitEvent(s0, ctx->hev_done[i], 0), "wait");
    KasChooseLaunch a;
    memset(&a, 0, sizeof(a));
    a.sr = d_sr; a.si = (const kas_scenario_impact*)ctx->hbuf[KAS_HB_IMP_SCEN].p;
    a.sizes = (const KasChooseSize*)ctx->hbuf[KAS_HB_CH_SIZES].p; a.segs = (const KasChooseSeg*)ctx->hbuf[KAS_HB_CH_SEGS].p;
    std::vector<KasChooseSize> sizes0;                          // a choice without rows: the gather sees scenarios without cells
    if (!hc.ch_gather_rows && !cp.sizes.empty()) {
      sizes0 = cp.sizes;
      for (KasChooseSize& z : sizes0) { z.cells = 0; z.seg_count = 0; }
      copy(ctx->hbuf[KAS_HB_MV_SIZES0].p, sizes0.data(), sizeof(KasChooseSize) * sizes0.size(), hipMemcpyHostToDevice, s0, "upload size table");
      hip_ok(hipStreamSynchronize(s0), "hipStreamSynchronize");  // (sizes0 is this block's)
    }
    kas_choose_fill_spec(&a, spec, (int32_t)S);
    a.row_off = (int64_t*)(d_head + hc.ch_head.row_off); a.node_off = (int64_t*)(d_head + hc.ch_head.node_off);
    a.rank = (int32_t*)(d_head + hc.ch_head.rank); a.chosen = (int32_t*)(d_head + hc.ch_head.chosen); a.n_ok = (int32_t*)(d_head + hc.ch_head.n_ok);
    a.out = native16 ? (const void*)d_out16 : (const void*)d_out;            // the pool the solve wrote
    a.src_nodes = (const kas_node_impact*)ctx->hbuf[KAS_HB_IMP_NODES].p;
    a.rows = ctx->hbuf[KAS_HB_CH_ROWS].p; a.nodes = (kas_node_impact*)ctx->hbuf[KAS_HB_CH_NODES].p;
    a.src_cell = native16 ? 2 : 4; a.dst_cell = (int32_t)out.cell;            // (a widened call: narrowed on the way)
    a.chunks = (int32_t)hc.ch_chunks;
    if (he == hipSuccess) {
      int e;
      // (the planner refused a rack criterion without a rack pass: the records are this call's)
      const kas_scenario_rack_impact* srk = (const kas_scenario_rack_impact*)ctx->hbuf[KAS_HB_RK_SCEN].p;
      const bool by_racks = rack_keys && hrk && (front ? kas_front_spec_uses_racks(front) : kas_choose_spec_uses_racks(spec));
      // (... and a topic criterion without a topic pass; srk is not read when the spec names no rack criterion)
      const kas_scenario_topic_impact* stp = (const kas_scenario_topic_impact*)ctx->hbuf[KAS_HB_TP_SCEN].p;
      const bool by_topics = topic_keys && topic_pass && (front ? kas_front_spec_uses_topics(front) : kas_choose_spec_uses_topics(spec));
      if (front) {                                              // mark and front rank where the rank kernel runs
        KasFrontLaunch f;
        memset(&f, 0, sizeof(f));
        kas_front_fill_spec(&f, front, (int32_t)S);
        f.c = a;
        f.cls = (int32_t*)ctx->hbuf[KAS_HB_FR_CLS].p; f.counts = (int32_t*)ctx->hbuf[KAS_HB_FR_COUNTS].p;
        const KasRackFrontLaunch fr{f, srk};
        const KasTopicFrontLaunch ft{f, hrk ? srk : nullptr, stp};
        e = by_topics ? kas_front_mark_topics_launch(&ft, s0) : by_racks ? kas_front_mark_racks_launch(&fr, s0) : kas_front_mark_launch(&f, s0);
        if (e == 0) e = by_topics ? kas_front_rank_topics_launch(&ft, s0) : by_racks ? kas_front_rank_racks_launch(&fr, s0) : kas_front_rank_launch(&f, s0);
      } else {
        const KasRackChooseLaunch ar{a, srk};
        const KasTopicChooseLaunch at{a, hrk ? srk : nullptr, stp};
        e = by_topics ? kas_rank_topics_launch(&at, s0) : by_racks ? kas_rank_racks_launch(&ar, s0) : kas_rank_launch(&a, s0);
      }
      if (!hc.ch_gather_rows) a.sizes = (const KasChooseSize*)ctx->hbuf[KAS_HB_MV_SIZES0].p;
      if (e == 0) e = kas_gather_launch(&a, s0);
      hip_ok((hipError_t)e, "choose kernels");
    }
    copy(p_head, d_head, hc.ch_head.bytes, hipMemcpyDeviceToHost, s0, "download the choice");
    if (front) copy(ctx->hbuf[KAS_HB_FR_COUNTS_PIN].p, ctx->hbuf[KAS_HB_FR_COUNTS].p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s0, "download the counts");
  }
  // a move list: the three kernels on s0 behind every range (and behind the rank kernel, whose chosen[] is a choice's list)
  char* const d_mvh = (char*)ctx->hbuf[KAS_HB_MV_HEAD].p;
  int64_t* const p_mvh = (int64_t*)ctx->hbuf[KAS_HB_MV_HEAD_PIN].p;
  const int64_t mv_n = hc.mv_n;
  if (hmv && he == hipSuccess && fail_rc == KAS_E_OK) {
    const KasMovesPlan& mp = hc.moves;
    if (!mp.scen.empty()) copy(ctx->hbuf[KAS_HB_MV_SCEN].p, mp.scen.data(), sizeof(KasMovesScen) * mp.scen.size(), hipMemcpyHostToDevice, s0, "upload moves scenario table");
    if (!mp.segs.empty()) copy(ctx->hbuf[KAS_HB_MV_SEGS].p, mp.segs.data(), sizeof(KasMovesSeg) * mp.segs.size(), hipMemcpyHostToDevice, s0, "upload moves segment table");
    if (!hch && mv_n > 0) copy(ctx->hbuf[KAS_HB_MV_SELECT].p, hc.mv_list.data(), 4 * (size_t)mv_n, hipMemcpyHostToDevice, s0, "upload the moves list");
    for (int i = 0; !hch && K > 1 && i < K; ++i) hip_ok(hipStreamWaitEvent(s0, ctx->hev_done[i], 0), "wait");
    // (records a truncated list leaves unwritten are told from written ones by their len: no written record has 0xff there)
    if (hc.mv_moves_cap > 0 && hmv->cells_cap < hc.mv_room_cells)
      hip_ok(hipMemsetAsync(ctx->hbuf[KAS_HB_MV_MOVES].p, 0xff, sizeof(kas_move) * (size_t)hc.mv_moves_cap, s0), "hipMemsetAsync");
    KasMovesLaunch a;
    memset(&a, 0, sizeof(a));
    a.scen = (const KasMovesScen*)ctx->hbuf[KAS_HB_MV_SCEN].p; a.segs = (const KasMovesSeg*)ctx->hbuf[KAS_HB_MV_SEGS].p;
    a.select = hch ? (const int32_t*)(d_head + hc.ch_head.chosen) : (const int32_t*)ctx->hbuf[KAS_HB_MV_SELECT].p;
    a.cur = native16 ? (const void*)d_cur16 : (const void*)d_cur;
    a.out = native16 ? (const void*)d_out16 : (const void*)d_out;
    a.aux = d_aux; a.topic_results = d_tr;
    a.scratch = (KasMovesCount*)ctx->hbuf[KAS_HB_MV_SCRATCH].p;
    a.move_off = (int64_t*)d_mvh; a.cell_off = (int64_t*)d_mvh + (mv_n + 1);
    a.moves = (kas_move*)ctx->hbuf[KAS_HB_MV_MOVES].p; a.cells = ctx->hbuf[KAS_HB_MV_CELLS].p;
    a.moves_cap = hc.mv_moves_cap; a.cells_cap = hc.mv_cells_cap;
    a.n = (int32_t)mv_n; a.stride = mp.max_items; a.S = (int32_t)S; a.mask = hmv->mask;
    a.src16 = native16 ? 1 : 0; a.dst16 = c16 ? 1 : 0;          // (a widened call: narrowed on the way)
    if (he == hipSuccess) hip_ok((hipError_t)kas_moves_launch(&a, full.Wc, s0), "moves pass");
    copy(p_mvh, d_mvh, 16 * (size_t)(mv_n + 1), hipMemcpyDeviceToHost, s0, "download the move offsets");
  }
  // the batches pass: one workgroup per listed scenario on s0, behind every range
  const int64_t bt_n = hc.bt_n;
  if (hbt && he == hipSuccess && fail_rc == KAS_E_OK) {
    const KasMovesPlan& mp = hc.moves;
    if (!mp.scen.empty()) copy(ctx->hbuf[KAS_HB_MV_SCEN].p, mp.scen.data(), sizeof(KasMovesScen) * mp.scen.size(), hipMemcpyHostToDevice, s0, "upload moves scenario table");
    if (!mp.segs.empty()) copy(ctx->hbuf[KAS_HB_MV_SEGS].p, mp.segs.data(), sizeof(KasMovesSeg) * mp.segs.size(), hipMemcpyHostToDevice, s0, "upload moves segment table");
    if (S > 0) copy(ctx->hbuf[KAS_HB_BT_SDESC].p, batch->scenarios, sizeof(kas_scenario_desc) * (size_t)S, hipMemcpyHostToDevice, s0, "upload scenario descriptors");
    if (!native16 && batch->node_pool_len > 0)
      copy(ctx->hbuf[KAS_HB_BT_NODE_ID].p, batch->node_id, 4 * (size_t)batch->node_pool_len, hipMemcpyHostToDevice, s0, "upload node ids");
    if (bt_n > 0) copy(ctx->hbuf[KAS_HB_BT_SELECT].p, hc.bt_list.data(), 4 * (size_t)bt_n, hipMemcpyHostToDevice, s0, "upload the batches list");
    for (int i = 0; K > 1 && i < K; ++i) hip_ok(hipStreamWaitEvent(s0, ctx->hev_done[i], 0), "wait");
    KasBatchesLaunch a;
    memset(&a, 0, sizeof(a));
    a.scen = (const KasMovesScen*)ctx->hbuf[KAS_HB_MV_SCEN].p; a.segs = (const KasMovesSeg*)ctx->hbuf[KAS_HB_MV_SEGS].p;
    a.sdesc = (const kas_scenario_desc*)ctx->hbuf[KAS_HB_BT_SDESC].p; a.node_id = (const int32_t*)ctx->hbuf[KAS_HB_BT_NODE_ID].p;
    a.select = (const int32_t*)ctx->hbuf[KAS_HB_BT_SELECT].p;
    a.cur = native16 ? (const void*)d_cur16 : (const void*)d_cur;
    a.out = native16 ? (const void*)d_out16 : (const void*)d_out;
    a.aux = d_aux; a.topic_results = d_tr;
    a.scenarios = (kas_scenario_batches*)ctx->hbuf[KAS_HB_BT_SCEN].p; a.batches = (kas_move_batch*)ctx->hbuf[KAS_HB_BT_BATCHES].p;
    a.stride = hbt->stride; a.spec = *bsp;
    a.n = (int32_t)bt_n; a.S = (int32_t)S; a.n_cap = hc.bt_n_cap; a.src16 = native16 ? 1 : 0;
    a.lds = kas_batches_lds(a.n_cap, full.Wc <= 3 ? 3 : (full.Wc <= 5 ? 5 : 8), a.src16);
    if (he == hipSuccess) hip_ok((hipError_t)kas_batches_launch(&a, full.Wc, s0), "batches pass");
  }
  // the rounds pass: where the batches pass runs, from the same tables
  const int64_t rd_n = hc.rd_n;
  if (hrd && he == hipSuccess && fail_rc == KAS_E_OK) {
    const KasMovesPlan& mp = hc.moves;
    if (!mp.scen.empty()) copy(ctx->hbuf[KAS_HB_MV_SCEN].p, mp.scen.data(), sizeof(KasMovesScen) * mp.scen.size(), hipMemcpyHostToDevice, s0, "upload moves scenario table");
    if (!mp.segs.empty()) copy(ctx->hbuf[KAS_HB_MV_SEGS].p, mp.segs.data(), sizeof(KasMovesSeg) * mp.segs.size(), hipMemcpyHostToDevice, s0, "upload moves segment table");
    if (S > 0) copy(ctx->hbuf[KAS_HB_BT_SDESC].p, batch->scenarios, sizeof(kas_scenario_desc) * (size_t)S, hipMemcpyHostToDevice, s0, "upload scenario descriptors");
    if (!native16 && batch->node_pool_len > 0)
      copy(ctx->hbuf[KAS_HB_BT_NODE_ID].p, batch->node_id, 4 * (size_t)batch->node_pool_len, hipMemcpyHostToDevice, s0, "upload node ids");
    if (rd_n > 0) copy(ctx->hbuf[KAS_HB_BT_SELECT].p, hc.rd_list.data(), 4 * (size_t)rd_n, hipMemcpyHostToDevice, s0, "upload the rounds list");
    for (int i = 0; K > 1 && i < K; ++i) hip_ok(hipStreamWaitEvent(s0, ctx->hev_done[i], 0), "wait");
    KasRoundsLaunch a;
    memset(&a, 0, sizeof(a));
    a.scen = (const KasMovesScen*)ctx->hbuf[KAS_HB_MV_SCEN].p; a.segs = (const KasMovesSeg*)ctx->hbuf[KAS_HB_MV_SEGS].p;
    a.sdesc = (const kas_scenario_desc*)ctx->hbuf[KAS_HB_BT_SDESC].p; a.node_id = (const int32_t*)ctx->hbuf[KAS_HB_BT_NODE_ID].p;
    a.select = (const int32_t*)ctx->hbuf[KAS_HB_BT_SELECT].p;
    a.cur = native16 ? (const void*)d_cur16 : (const void*)d_cur;
    a.out = native16 ? (const void*)d_out16 : (const void*)d_out;
    a.aux = d_aux; a.topic_results = d_tr;
    a.scenarios = (kas_scenario_rounds*)ctx->hbuf[KAS_HB_RD_SCEN].p; a.rounds = (kas_move_round*)ctx->hbuf[KAS_HB_RD_ROUNDS].p;
    a.round_of = (int32_t*)ctx->hbuf[KAS_HB_RD_OF].p;
    a.round_stride = hrd->round_stride; a.move_stride = hrd->move_stride; a.spec = *rsp;
    a.n = (int32_t)rd_n; a.S = (int32_t)S; a.n_cap = hc.rd_n_cap; a.src16 = native16 ? 1 : 0;
    a.lds = kas_rounds_lds(a.n_cap, full.Wc <= 3 ? 3 : (full.Wc <= 5 ? 5 : 8), a.src16);
    if (he == hipSuccess) hip_ok((hipError_t)kas_rounds_launch(&a, full.Wc, s0), "rounds pass");
  }
  drain();
  if (he != hipSuccess || fail_rc != KAS_E_OK) return fail_rc != KAS_E_OK ? fail_rc : KAS_E_HIP;
  if (hch) {                                                   // exactly the chosen scenarios' rows and node blocks, through the staging
    const int64_t cells = ((const int64_t*)(p_head + hc.ch_head.row_off))[ch_k], recs = ((const int64_t*)(p_head + hc.ch_head.node_off))[ch_k];
    if (cells < 0 || (hc.ch_gather_rows && cells > hc.ch_rows_need) || recs < 0 || recs > hc.ch_nodes_need)
      return set_error(KAS_E_HIP, "internal: the rank kernel left offsets beyond the k largest scenarios");
    if (cells > 0 && hc.ch_gather_rows) copy(ctx->hbuf[KAS_HB_CH_ROWS_PIN].p, ctx->hbuf[KAS_HB_CH_ROWS].p, out.cell * (size_t)cells, hipMemcpyDeviceToHost, s0, "download chosen rows");
    if (recs > 0) copy(ctx->hbuf[KAS_HB_CH_NODES_PIN].p, ctx->hbuf[KAS_HB_CH_NODES].p, sizeof(kas_node_impact) * (size_t)recs, hipMemcpyDeviceToHost, s0, "download chosen node records");
    if (S > 0) memcpy(hch->rank, p_head + hc.ch_head.rank, 4 * (size_t)S);
    if (ch_k > 0) memcpy(hch->chosen, p_head + hc.ch_head.chosen, 4 * (size_t)ch_k);
    memcpy(hch->row_off, p_head + hc.ch_head.row_off, 8 * (size_t)(ch_k + 1));
    memcpy(hch->node_off, p_head + hc.ch_head.node_off, 8 * (size_t)(ch_k + 1));
    memcpy(hch->n_ok, p_head + hc.ch_head.n_ok, 4);
    if (front) memcpy(counts, ctx->hbuf[KAS_HB_FR_COUNTS_PIN].p, 4 * sizeof(int32_t));
  }
  for (const KasHostRange& r : hc.ranges) {                    // (only what the ranges own: as the direct copies did)
    const KasExtent& t = r.own[KAS_POOL_TOPICS];
    if (t.hi > t.lo) memcpy(h->topic_results + t.lo, p_tr + t.lo, sizeof(kas_topic_result) * (size_t)(t.hi - t.lo));
    if (r.hi > r.lo) memcpy(h->scenario_results + r.lo, p_sr + r.lo, sizeof(kas_scenario_result) * (size_t)(r.hi - r.lo));
  }
  // Context counters back; the selected scenarios' rows, packed
  if (ctx_x.hi > ctx_x.lo) copy(h->ctx + ctx_x.lo, d_ctx + ctx_x.lo, 4 * (size_t)(ctx_x.hi - ctx_x.lo), hipMemcpyDeviceToHost, s0, "download ctx");
  for (int32_t k = 0; !all_rows && k < n_select && he == hipSuccess; ++k) {
    const kas_scenario_desc& sd = batch->scenarios[select[k]];
    int64_t at = hc.sel_off[(size_t)k];
    for (int32_t t = 0; t < sd.topic_count && he == hipSuccess; ++t) {
      const kas_topic_desc& td = batch->topics[sd.topic_begin + t];
      const int64_t cells = (int64_t)td.n_partitions * td.out_width;
      if (cells > 0) {
        if (widened) narrow(s0, td.out_off, cells);
        copy(out.h(at), out.d(td.out_off), out.cell * (size_t)cells, hipMemcpyDeviceToHost, s0, "download selected rows");
      }
      at += cells;
    }
  }
  if (himp) {
    const int64_t nodes = hch ? 0 : hc.imp_base[(size_t)S];      // (a choice leaves the node table on the device)
    if (nodes > 0 && himp->nodes) copy(himp->nodes, ctx->hbuf[KAS_HB_IMP_NODES].p, sizeof(kas_node_impact) * (size_t)nodes, hipMemcpyDeviceToHost, s0, "download node impact");
    if (S > 0) copy(himp->scenarios, ctx->hbuf[KAS_HB_IMP_SCEN].p, sizeof(kas_scenario_impact) * (size_t)S, hipMemcpyDeviceToHost, s0, "download scenario impact");
  }
  if (hrk) {
    const int64_t recs = hc.rack.rack_off[(size_t)S];
    if (recs > 0) copy(hrk->racks, ctx->hbuf[KAS_HB_RK_RACKS].p, sizeof(kas_rack_impact) * (size_t)recs, hipMemcpyDeviceToHost, s0, "download rack impact");
    if (S > 0) copy(hrk->scenarios, ctx->hbuf[KAS_HB_RK_SCEN].p, sizeof(kas_scenario_rack_impact) * (size_t)S, hipMemcpyDeviceToHost, s0, "download scenario rack impact");
    memcpy(hrk->rack_off, hc.rack.rack_off.data(), sizeof(int64_t) * ((size_t)S + 1));
  }
  if (topic_pass) {
    const int64_t T = batch->n_topics;
    if (T > 0) copy(htp->topics, ctx->hbuf[KAS_HB_TP_TOPICS].p, sizeof(kas_topic_impact) * (size_t)T, hipMemcpyDeviceToHost, s0, "download topic impact");
    if (S > 0) copy(htp->scenarios, ctx->hbuf[KAS_HB_TP_SCEN].p, sizeof(kas_scenario_topic_impact) * (size_t)S, hipMemcpyDeviceToHost, s0, "download scenario topic impact");
  }
  // the move list: the offsets (they are here already), then exactly the records that were written and the cells they use
  if (hmv && he == hipSuccess) {
    const int64_t total = p_mvh[mv_n], total_cells = p_mvh[2 * mv_n + 1];
    if (total < 0 || total > hc.mv_room_moves || total_cells < 0 || total_cells > hc.mv_room_cells)
      return set_error(KAS_E_HIP, "internal: the moves pass left offsets beyond the rows of the listed scenarios");
    memcpy(hmv->move_off, p_mvh, 8 * (size_t)(mv_n + 1));
    memcpy(hmv->cell_off, p_mvh + (mv_n + 1), 8 * (size_t)(mv_n + 1));
    int64_t written = total < hc.mv_moves_cap ? total : hc.mv_moves_cap, used = written > 0 ? total_cells : 0;
    const kas_move* d_moves = (const kas_move*)ctx->hbuf[KAS_HB_MV_MOVES].p;
    if (written > 0 && (total_cells > hmv->cells_cap || written < total)) {
      // the written records are a prefix (a list's end grows with its index): find its end by the marker, then the cells it uses
      kas_move probe;
      int64_t lo = 0, hi = written;                             // records below lo are written, records from hi on are not
      while (lo < hi && total_cells > hmv->cells_cap && he == hipSuccess) {
        const int64_t mid = (lo + hi) >> 1;
        hip_ok(hipMemcpy(&probe, d_moves + mid, sizeof(probe), hipMemcpyDeviceToHost), "probe a move record");
        if (probe.len != 0xff) lo = mid + 1; else hi = mid;
      }
      if (total_cells > hmv->cells_cap) written = lo;
      used = 0;
      if (written > 0 && hip_ok(hipMemcpy(&probe, d_moves + written - 1, sizeof(probe), hipMemcpyDeviceToHost), "probe a move record")) {
        int64_t j = 0;                                          // its block: the last listed scenario that starts at or before it
        while (j + 1 < mv_n && p_mvh[j + 1] <= written - 1) ++j;
        used = p_mvh[(mv_n + 1) + j] + probe.cell_at + probe.len;
      }
    }
    if (written > 0) copy(hmv->moves, d_moves, sizeof(kas_move) * (size_t)written, hipMemcpyDeviceToHost, s0, "download the moves");
    if (used > 0) copy(hmv->cells, ctx->hbuf[KAS_HB_MV_CELLS].p, out.cell * (size_t)used, hipMemcpyDeviceToHost, s0, "download the moves' cells");
  }
  // the batches: the scenario records, then exactly the batch records each listed scenario wrote
  if (hbt && he == hipSuccess && bt_n > 0) {
    if (hip_ok(hipMemcpy(hbt->scenarios, ctx->hbuf[KAS_HB_BT_SCEN].p, sizeof(kas_scenario_batches) * (size_t)bt_n, hipMemcpyDeviceToHost), "download scenario batches")) {
      const kas_move_batch* d_b = (const kas_move_batch*)ctx->hbuf[KAS_HB_BT_BATCHES].p;
      for (int64_t j = 0; j < bt_n && hbt->stride > 0 && he == hipSuccess; ++j) {
        const int64_t nb = hbt->scenarios[j].n_batches;
        if (nb < 0) return set_error(KAS_E_HIP, "internal: the batches pass left a negative count");
        const int64_t w = nb < hbt->stride ? nb : hbt->stride;
        if (w > 0) copy(hbt->batches + j * hbt->stride, d_b + j * hbt->stride, sizeof(kas_move_batch) * (size_t)w, hipMemcpyDeviceToHost, s0, "download batch records");
      }
    }
  }
  // the rounds: the scenario records, then exactly the round records and the round_of prefix each listed scenario wrote
  if (hrd && he == hipSuccess && rd_n > 0) {
    if (hip_ok(hipMemcpy(hrd->scenarios, ctx->hbuf[KAS_HB_RD_SCEN].p, sizeof(kas_scenario_rounds) * (size_t)rd_n, hipMemcpyDeviceToHost), "download scenario rounds")) {
      const kas_move_round* d_r = (const kas_move_round*)ctx->hbuf[KAS_HB_RD_ROUNDS].p;
      const int32_t* d_of = (const int32_t*)ctx->hbuf[KAS_HB_RD_OF].p;
      for (int64_t j = 0; j < rd_n && he == hipSuccess; ++j) {
        const int64_t nr = hrd->scenarios[j].n_rounds, nm = hrd->scenarios[j].n_moves;
        if (nr < 0 || nm < 0) return set_error(KAS_E_HIP, "internal: the rounds pass left a negative count");
        const int64_t wr = nr < hrd->round_stride ? nr : hrd->round_stride, wm = nm < hrd->move_stride ? nm : hrd->move_stride;
        if (wr > 0) copy(hrd->rounds + j * hrd->round_stride, d_r + j * hrd->round_stride, sizeof(kas_move_round) * (size_t)wr, hipMemcpyDeviceToHost, s0, "download round records");
        if (wm > 0) copy(hrd->round_of + j * hrd->move_stride, d_of + j * hrd->move_stride, 4 * (size_t)wm, hipMemcpyDeviceToHost, s0, "download round_of");
      }
    }
  }
  hip_ok(hipStreamSynchronize(s0), "hipStreamSynchronize");
  if (hch && he == hipSuccess && hc.ch_gather_rows) {
    const int64_t cells = hch->row_off[ch_k], recs = hch->node_off[ch_k];
    if (cells > 0) memcpy(hch->rows, ctx->hbuf[KAS_HB_CH_ROWS_PIN].p, out.cell * (size_t)cells);
    if (recs > 0) memcpy(hch->nodes, ctx->hbuf[KAS_HB_CH_NODES_PIN].p, sizeof(kas_node_impact) * (size_t)recs);
  } else if (hch && he == hipSuccess) {
    const int64_t recs = hch->node_off[ch_k];
    if (recs > 0) memcpy(hch->nodes, ctx->hbuf[KAS_HB_CH_NODES_PIN].p, sizeof(kas_node_impact) * (size_t)recs);
  }
  return he == hipSuccess ? KAS_E_OK : fail_rc;
}

int kas_solve_host_select(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select) {
  if (!ctx || !batch || !h) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select);
}

int kas_solve_host(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h) {
  return kas_solve_host_select(ctx, batch, h, nullptr, -1);
}

int kas_solve_host16(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select) {
  if (!ctx || !batch || !h16) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16);
}

int kas_solve_host_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select,
                          const kas_impact_tables* himp) {
  if (!ctx || !batch || !h || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select, nullptr, himp);
}

int kas_solve_host16_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select,
                            const kas_impact_tables* himp) {
  if (!ctx || !batch || !h16 || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16, himp);
}

int kas_solve_host_rack_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select,
                               const kas_impact_tables* himp, const int32_t* report_rack, const kas_rack_tables* hrk) {
  if (!ctx || !batch || !h || !himp || !hrk) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select, nullptr, himp, nullptr, nullptr, nullptr, false, nullptr, nullptr, hrk, report_rack);
}

int kas_solve_host16_rack_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select,
                                 const kas_impact_tables* himp, const int32_t* report_rack, const kas_rack_tables* hrk) {
  if (!ctx || !batch || !h16 || !himp || !hrk) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16, himp, nullptr, nullptr, nullptr, false, nullptr, nullptr,
                               hrk, report_rack);
}

// (host_impact may be NULL: no impact pass; host_topics == NULL is the planner's refusal, in its documented place)
int kas_solve_host_topic_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select,
                                const kas_impact_tables* himp, const kas_topic_impact_tables* htp) {
  if (!ctx || !batch || !h) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select, nullptr, himp, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr, nullptr,
                               false, true, htp);
}

int kas_solve_host16_topic_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select,
                                  const kas_impact_tables* himp, const kas_topic_impact_tables* htp) {
  if (!ctx || !batch || !h16) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16, himp, nullptr, nullptr, nullptr, false, nullptr, nullptr,
                               nullptr, nullptr, false, true, htp);
}

int kas_solve_host_batches(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select,
                           const kas_batch_spec* bsp, const kas_batches* hbt) {
  if (!ctx || !batch || !h || !bsp || !hbt) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select < 0 ? -1 : n_select, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr,
                               nullptr, nullptr, false, false, nullptr, false, bsp, hbt);
}

int kas_solve_host16_batches(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select,
                             const kas_batch_spec* bsp, const kas_batches* hbt) {
  if (!ctx || !batch || !h16 || !bsp || !hbt) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr,
                               nullptr, nullptr, false, false, nullptr, false, bsp, hbt);
}

int kas_solve_host_rounds(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select,
                          const kas_round_spec* rsp, const kas_rounds* hrd) {
  if (!ctx || !batch || !h || !rsp || !hrd) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select < 0 ? -1 : n_select, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr,
                               nullptr, nullptr, false, false, nullptr, false, nullptr, nullptr, rsp, hrd);
}

int kas_solve_host16_rounds(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select,
                            const kas_round_spec* rsp, const kas_rounds* hrd) {
  if (!ctx || !batch || !h16 || !rsp || !hrd) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr,
                               nullptr, nullptr, false, false, nullptr, false, nullptr, nullptr, rsp, hrd);
}

int kas_solve_host_choose(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_choose_spec* spec, const kas_choice* hch,
                          const kas_impact_tables* himp) {
  if (!ctx || !batch || !h || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, spec, hch);
}

int kas_solve_host16_choose(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_choose_spec* spec, const kas_choice* hch,
                            const kas_impact_tables* himp) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, spec, hch);
}

int kas_solve_host_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const int32_t* select, int32_t n_select,
                         const kas_moves* hmv) {
  if (!ctx || !batch || !h || !hmv) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, select, n_select < 0 ? -1 : n_select, nullptr, nullptr, nullptr, nullptr, hmv);
}

int kas_solve_host16_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const int32_t* select, int32_t n_select,
                           const kas_moves* hmv) {
  if (!ctx || !batch || !h16 || !hmv) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, select, n_select < 0 ? -1 : n_select, &c16, nullptr, nullptr, nullptr, hmv);
}

int kas_solve_host_choose_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_choose_spec* spec, const kas_choice* hch,
                                const kas_impact_tables* himp, const kas_moves* hmv) {
  if (!ctx || !batch || !h || !spec || !hch || !himp || !hmv) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, spec, hch, hmv, true);
}

int kas_solve_host16_choose_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_choose_spec* spec,
                                  const kas_choice* hch, const kas_impact_tables* himp, const kas_moves* hmv) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp || !hmv) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, spec, hch, hmv, true);
}

int kas_solve_host_front(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_front_spec* spec, const kas_choice* hch,
                         int32_t* counts, const kas_impact_tables* himp, const kas_moves* hmv) {
  if (!ctx || !batch || !h || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, nullptr, hch, hmv, true, spec, counts);
}

int kas_solve_host16_front(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_front_spec* spec, const kas_choice* hch,
                           int32_t* counts, const kas_impact_tables* himp, const kas_moves* hmv) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, nullptr, hch, hmv, true, spec, counts);
}

// kas_solve_host_choose_moves / kas_solve_host_front / 16 plus the rack pass; the spec may name rack criteria
int kas_solve_host_choose_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_choose_spec* spec, const kas_choice* hch,
                                const kas_impact_tables* himp, const kas_moves* hmv, const int32_t* report_rack, const kas_rack_tables* hrk) {
  if (!ctx || !batch || !h || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, spec, hch, hmv, true, nullptr, nullptr, hrk, report_rack, true);
}

int kas_solve_host16_choose_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_choose_spec* spec,
                                  const kas_choice* hch, const kas_impact_tables* himp, const kas_moves* hmv, const int32_t* report_rack,
                                  const kas_rack_tables* hrk) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, spec, hch, hmv, true, nullptr, nullptr, hrk, report_rack, true);
}

int kas_solve_host_front_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_front_spec* spec, const kas_choice* hch,
                               int32_t* counts, const kas_impact_tables* himp, const kas_moves* hmv, const int32_t* report_rack,
                               const kas_rack_tables* hrk) {
  if (!ctx || !batch || !h || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, nullptr, hch, hmv, true, spec, counts, hrk, report_rack, true);
}

int kas_solve_host16_front_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_front_spec* spec,
                                 const kas_choice* hch, int32_t* counts, const kas_impact_tables* himp, const kas_moves* hmv,
                                 const int32_t* report_rack, const kas_rack_tables* hrk) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, nullptr, hch, hmv, true, spec, counts, hrk, report_rack, true);
}

// kas_solve_host_choose_racks / kas_solve_host_front_racks / 16 plus the topic pass (htp != NULL); the spec may name topic criteria
int kas_solve_host_choose_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_choose_spec* spec, const kas_choice* hch,
                                 const kas_impact_tables* himp, const kas_moves* hmv, const int32_t* report_rack, const kas_rack_tables* hrk,
                                 const kas_topic_impact_tables* htp) {
  if (!ctx || !batch || !h || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, spec, hch, hmv, true, nullptr, nullptr, hrk, report_rack, true,
                               htp != nullptr, htp, true);
}

int kas_solve_host16_choose_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_choose_spec* spec,
                                   const kas_choice* hch, const kas_impact_tables* himp, const kas_moves* hmv, const int32_t* report_rack,
                                   const kas_rack_tables* hrk, const kas_topic_impact_tables* htp) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, spec, hch, hmv, true, nullptr, nullptr, hrk, report_rack, true,
                               htp != nullptr, htp, true);
}

int kas_solve_host_front_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* h, const kas_front_spec* spec, const kas_choice* hch,
                                int32_t* counts, const kas_impact_tables* himp, const kas_moves* hmv, const int32_t* report_rack,
                                const kas_rack_tables* hrk, const kas_topic_impact_tables* htp) {
  if (!ctx || !batch || !h || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, h, nullptr, 0, nullptr, himp, nullptr, hch, hmv, true, spec, counts, hrk, report_rack, true,
                               htp != nullptr, htp, true);
}

int kas_solve_host16_front_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* h16, const kas_front_spec* spec,
                                  const kas_choice* hch, int32_t* counts, const kas_impact_tables* himp, const kas_moves* hmv,
                                  const int32_t* report_rack, const kas_rack_tables* hrk, const kas_topic_impact_tables* htp) {
  if (!ctx || !batch || !h16 || !spec || !hch || !himp) return set_error(KAS_E_INVALID_ARG, "NULL argument");
  KasCells16 c16;
  const kas_tables h = kas_tables_of16(h16, &c16);
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  return kas_solve_host_locked(ctx, batch, &h, nullptr, 0, &c16, himp, nullptr, hch, hmv, true, spec, counts, hrk, report_rack, true,
                               htp != nullptr, htp, true);
}

int kas_solve_host_sharded(kas_ctx* const* ctxs, int32_t n_ctx, const kas_batch_desc* batch, const kas_tables* h) {
  if (!ctxs || n_ctx < 1 || !batch || !h) return set_error(KAS_E_INVALID_ARG, "NULL argument / no context");
  for (int32_t r = 0; r < n_ctx; ++r) if (!ctxs[r]) return set_error(KAS_E_INVALID_ARG, "ctxs[r] == NULL");
  if (n_ctx == 1) return kas_solve_host(ctxs[0], batch, h);
  // Every shard downloads the whole extent of `out` (and round-trips the whole extent of `ctx`) its scenarios refer
  // to: with pools that are not laid out in scenario order one shard's download would overwrite rows or Context
  // counters another has already delivered.  Such a batch is solved on one context (same results, no overlap).
  std::vector<KasHostRange> shards;
  {
    std::string err;
    int32_t bad = 0;
    const int rc = kas_cut_ranges(batch, n_ctx, nullptr, &shards, &err, &bad);
    if (rc != KAS_E_OK) return set_error(rc, "shard " + std::to_string(bad) + ": " + err);
  }
  if (!kas_ranges_disjoint(shards, (1u << KAS_POOL_OUT) | (1u << KAS_POOL_CTX), false)) return kas_solve_host(ctxs[0], batch, h);
  std::vector<int> rcs((size_t)n_ctx, KAS_E_OK);
  std::vector<std::string> errs((size_t)n_ctx);
  std::vector<std::thread> threads;
  for (int32_t r = 0; r < n_ctx; ++r) {
    threads.emplace_back([&, r]() {
      const KasHostRange& sh = shards[(size_t)r];
      if (sh.hi <= sh.lo) return;
      const kas_tables ht = kas_tables_at(*h, sh.own[KAS_POOL_TOPICS].lo, sh.lo);
      const int rc = kas_solve_host(ctxs[r], &sh.bd, &ht);
      rcs[(size_t)r] = rc;
      if (rc != KAS_E_OK) errs[(size_t)r] = g_last_error;      // (thread-local: carried to the caller below)
    });
  }
  for (std::thread& t : threads) t.join();
  for (int32_t r = 0; r < n_ctx; ++r)
    if (rcs[(size_t)r] != KAS_E_OK) return set_error(rcs[(size_t)r], "shard " + std::to_string(r) + ": " + errs[(size_t)r]);
  return KAS_E_OK;
}

int kas_ctx_host_stats(kas_ctx* ctx, int64_t* calls, int64_t* plan_hits, int64_t* device_allocs) {
  if (!ctx) return set_error(KAS_E_INVALID_ARG, "ctx == NULL");
  std::lock_guard<std::mutex> lock(ctx->host_mu);
  if (calls) *calls = (int64_t)ctx->host_calls;
  if (plan_hits) *plan_hits = (int64_t)ctx->host_plan_hits;
  if (device_allocs) *device_allocs = (int64_t)ctx->host_allocs;
  return KAS_E_OK;
}

}  // extern "C"
#pragma GCC visibility pop
