// kas_launch_plan.h — which kernels a solve launches, decided ONCE.
//
// Pure host C++ (no HIP calls).  kas_resolve_launch() turns a plan's state into the ordered list of launches of its next solve:
// kernel identity, grid, block, dynamic LDS and launch word of every stage.  The library (kas_hip.hip) walks that list to launch,
// to opt the kernels into their LDS sizes (kas_plan_set_kernels enumerates the resolver) and to print it (kas_plan_describe); the
// CPU emulator (tests/emu/emu_driver.cpp) walks the same list.  Neither holds a launch decision of its own.
// Include behind kas_solver_body.h (KAS_PERM_WAVES / KAS_PERM_BINS are the permutation kernel's own constants).
#pragma once
#include <stdio.h>

#include <string>

#include "kas_plan_math.h"

// tuning builds only: extra dynamic LDS per workgroup, to measure how much residency is worth
#ifndef KAS_TUNE_ORDER_LDS_PAD
#define KAS_TUNE_ORDER_LDS_PAD 0
#endif
#ifndef KAS_TUNE_FILL_LDS_PAD
#define KAS_TUNE_FILL_LDS_PAD 0
#endif
#ifndef KAS_TUNE_SLIM_LDS_PAD
#define KAS_TUNE_SLIM_LDS_PAD 0
#endif
// wavefronts per scenario of kas_p4_kernel (kas_hip.hip: measured 1, 2 and 4)
#ifndef KAS_P4_KERNEL_WAVES
#define KAS_P4_KERNEL_WAVES 1
#endif
// workgroups of the kas_fill_kernel launch behind the slim kernel (see kas_back_grid)
#define KAS_FILL_BACK_GRID 256u
#define KAS_FILL_BACK_GRID_STEP 64u

enum KasKernelFamily {
  KAS_K_SPREAD_A, KAS_K_SPREAD_Q, KAS_K_SPREAD_B, KAS_K_SPREAD_P4, KAS_K_FILL_SLIM, KAS_K_FILL, KAS_K_P4, KAS_K_PERMUTATION,
  KAS_K_ORDER_RELAX, KAS_K_P4_ORDER, KAS_K_ORDER_RELAX_WIDE, KAS_K_ORDER_TICKET, KAS_K_ORDER_WIDE, KAS_K_ORDER_ROUND,
  KAS_K_FAMILIES
};
// A kernel instance: the family and the template arguments that select it (those a family does not have stay 0).
struct KasKernelId {
  int32_t family = KAS_K_FILL;
  int32_t W = 0;                // width class
  int32_t NW = 0;               // fill: wavefronts per scenario
  int32_t G = 0;                // ticket form: scenarios per wavefront
  int32_t packed = 0;           // ticket form: 3 x 10-bit counter rows
  int32_t tiles = 0;            // relaxation form: 0 = tiles of 64 rows, 1 = double tiles, 2 = quad tiles
  int32_t ctx = 0, verify = 0;  // relaxation form: Context instance, sampled verification
  int32_t c16 = 0, idl = 0;     // relaxation form: 16-bit cells, broker ids in the LDS
  int32_t m32 = 0;              // dword mid rows (slim fill, kas_p4_kernel, relaxation form)
};
static inline bool operator==(const KasKernelId& x, const KasKernelId& y) {
  return x.family == y.family && x.W == y.W && x.NW == y.NW && x.G == y.G && x.packed == y.packed && x.tiles == y.tiles && x.ctx == y.ctx &&
         x.verify == y.verify && x.c16 == y.c16 && x.idl == y.idl && x.m32 == y.m32;
}

// what a stage is there for (its kernel says how)
enum KasStageRole {
  KAS_STAGE_SPREAD,             // the spread fill's four kernels
  KAS_STAGE_SLIM,               // the slim fill for every scenario
  KAS_STAGE_FILL,               // kas_fill_kernel: every scenario, or (ONLY_FLAGGED) what the spread / slim fill handed back
  KAS_STAGE_P4,                 // first fit in a kernel of its own
  KAS_STAGE_PERMUTATION,        // ticket form: scenarios by descending chain length
  KAS_STAGE_ORDER,              // P5: exactly one per solve
  KAS_STAGE_REFILL,             // wide form with checked count fields: fill again what it flagged ...
  KAS_STAGE_ROUND_FLAGGED       // ... and the round form for what an order kernel flagged
};
enum KasFlagSource { KAS_SP_FLAG_NONE, KAS_SP_FLAG_PLAN, KAS_SP_FLAG_ORD };
struct KasStage {
  KasKernelId k;
  int32_t role = KAS_STAGE_FILL;
  uint32_t grid_x = 1, grid_y = 1, block = 64;
  uint32_t lds = 0;             // dynamic LDS bytes of the launch
  uint32_t flags = 0;           // KasLaunch::flags of this launch
  int32_t sp_flag = KAS_SP_FLAG_NONE;   // KasLaunch::sp_flag: none, the plan's hand-back flags, the order kernels' ord_flag
  int32_t spread = 0;           // the spread fill's scratch (sp_hist .. sp_oc, sp_chunks) is wired in
  int32_t handback = 0;         // KasLaunch::handback: this launch leaves the number of flagged scenarios
  int32_t perm = 0;             // KasLaunch::perm is wired in
};
#define KAS_MAX_STAGES 10
struct KasResolvedLaunch {
  uint32_t flags = 0;           // KasLaunch::flags of the solve (the stages' words differ from it in the launcher's own bits only)
  int32_t spread_chunks = 0;
  int32_t cells16 = 0;
  int32_t order_form = 0;       // 1 ticket form, 2 wide ticket form, 3 relaxation form, 4 relaxation form for wide lists, 0 round form
  int32_t relax_off = 0;        // the relaxation form applies to the shape and was not asked away, yet is not launched:
                                // 1 self-test FAILED, 2 switched off, 3 could not run
  int32_t n_stages = 0;
  KasStage stages[KAS_MAX_STAGES];
  const KasStage* find(int32_t role) const {
    for (int32_t i = 0; i < n_stages; ++i) if (stages[i].role == role) return &stages[i];
    return nullptr;
  }
};

// kernel families a build may leave out (KAS_MINIMAL_INSTANCES builds of the library; everything in a full build and in the emulator)
#define KAS_BUILT_RELAX 1u
#define KAS_BUILT_RELAXW 2u
#define KAS_BUILT_WIDE 4u
#define KAS_BUILT_SLIM 8u
#define KAS_BUILT_P4_ORDER 16u
#define KAS_BUILT_SPREAD 32u
#define KAS_BUILT_ALL 63u

// everything the launch decisions read
struct KasLaunchIn {
  const KasShape* shape = nullptr;
  int32_t n_scenarios = 0, single_topic = 0, cells16 = 0;
  // the plan's state after kas_plan_set_flags (kas_user_flags)
  uint32_t flags = 0, index_rows_bits = 0, mid32_bits = 0, full_fill = 0;
  int32_t NW = 1, G = 1, fused = 0;
  int32_t lds_total = 0, lds_fused_total = 0;
  int32_t lane_order_ok = 1;    // the context's LDS lane-order self-test passed
  int32_t lane_order_state = 1; // ... its state, for the describe text only
  int32_t have_p4s = 1;         // the first-fit hand-over scratch exists
  int32_t have_back_flags = 1;  // the hand-back flag buffer exists
  int32_t last_handback = 0;    // scenarios the slim fill handed back in the plan's last solve
  int32_t relax_gather = 0;     // the relaxation form gathers the broker ids from the node table whatever the broker count
  uint32_t built = KAS_BUILT_ALL;
};
static inline void kas_launch_in_shape(KasLaunchIn* in, const KasShape* s) {
  in->shape = s;
  in->NW = s->NW; in->G = s->G; in->fused = s->fused_ok;
  in->lds_total = s->lds.total; in->lds_fused_total = s->lds_fused.total;
}

// A caller's flag word (kas_plan_set_flags, the emulator) as the plan keeps it: the bits that share a position with one of the
// launcher's own are kept beside `flags`; scenarios per wavefront only mean something to the ticket form.
struct KasUserFlags { uint32_t flags, index_rows_bits, mid32_bits, full_fill; };
static inline KasUserFlags kas_user_flags(uint32_t word) {
  KasUserFlags u;
  u.index_rows_bits = word & (KAS_PLAN_NO_INDEX_ROWS_BIT | KAS_PLAN_INDEX_ROWS_BIT);
  u.mid32_bits = word & (KAS_PLAN_NO_MID32_BIT | KAS_PLAN_MID32_BIT);
  u.full_fill = word & KAS_PLAN_FULL_FILL_BIT;
  u.flags = (word & (0xff0000ffu | KAS_FLAG_TICKET_ORDER | KAS_FLAG_RELAX_TILES_64 | KAS_FLAG_RELAX_TILES_128 | KAS_FLAG_NO_RTN_QUOTA |
                     KAS_FLAG_FILL_WITH_P4 | KAS_FLAG_SPLIT_P4) & ~(KAS_FLAG_FUSED_HIST | KAS_FLAG_ONLY_FLAGGED | KAS_FLAG_ORDER_FLAGGED)) |
            (((word >> 12) & 0xfu) != 0u ? KAS_FLAG_TICKET_ORDER : 0u);
  return u;
}
static inline void kas_launch_in_user_flags(KasLaunchIn* in, uint32_t word) {
  const KasUserFlags u = kas_user_flags(word);
  in->flags = u.flags; in->index_rows_bits = u.index_rows_bits; in->mid32_bits = u.mid32_bits; in->full_fill = u.full_fill;
}

// the relaxation form's instances for this plan keep the broker ids in the LDS (int32 cells; kas_relax_lds_ids)
static inline int32_t kas_relax_idl(const KasShape& s, bool c16, bool relax_gather) {
  return !c16 && !relax_gather && kas_relax_lds_ids(s.n_max, s.any_ctx) ? 1 : 0;
}

// 16-bit cells (kas_plan_create16, kas_solve_host16 without widening): the kernels with that I/O are the fill kernel (+ kas_p4_kernel),
// the relaxation form and the round form — lists up to 3 wide, and one of the two order forms must take the batch HERE
static inline bool kas_cells16_ok(const KasShape& s, int32_t lane_order_ok, uint32_t built) {
  return s.Wc <= 3 && ((s.relax_ok && lane_order_ok && (built & KAS_BUILT_RELAX)) || s.round_fits);
}

// A flag word the plan cannot honour (kas_plan_set_flags refuses it, and leaves the plan as it was): the reason, or NULL
static inline const char* kas_flags_refusal(const KasShape& s, bool c16, uint32_t word, bool relax_gather) {
  if ((word & KAS_FLAG_ROUND_ORDER) && !s.round_fits)
    return "KAS_PLAN_ROUND_ORDER: the round form's LDS exceeds 160 KiB at this broker count x width";
  if ((word >> 24) != 0u && s.relax_ok && !c16 && !kas_relax_idl(s, c16, relax_gather))
    return "KAS_PLAN_VERIFY_SAMPLE: not instantiated for the instances that gather the broker ids from the node table (this many brokers)";
  if (c16 && kas_flags_want_tickets(word) && !s.round_fits)
    return "16-bit cells: no ticket form; the round form it would take does not fit at this broker count";
  return nullptr;
}

// Workgroups of the kas_fill_kernel launch behind the slim kernel: KAS_FILL_BACK_GRID — each needs a 35 KB / 4 x 128-VGPR slot before it
// can see that there is nothing to do — unless the plan's last solve handed more scenarios back than that: then one workgroup per
// such scenario and a quarter more (a batch whose rows are not rack-diverse hands EVERY scenario back, and the general fill of a
// scenario is one long chain: 1000 of them on 256 workgroups took 53 ms, on 1000 they take 20).  A rebuilt plan starts small again.
static inline uint32_t kas_back_grid(int32_t last_handback, uint32_t fill_grid) {
  uint32_t g = KAS_FILL_BACK_GRID;
  const uint32_t last = last_handback > 0 ? (uint32_t)last_handback : 0u;
  if (last + last / 4u > g) g = ((last + last / 4u + KAS_FILL_BACK_GRID_STEP - 1u) / KAS_FILL_BACK_GRID_STEP) * KAS_FILL_BACK_GRID_STEP;
  return g < fill_grid ? g : fill_grid;
}

static inline KasResolvedLaunch kas_resolve_launch(const KasLaunchIn& in) {
  const KasShape& s = *in.shape;
  const int32_t Wc = s.Wc, S = in.n_scenarios;
  const bool c16 = in.cells16 != 0;
  const uint32_t uf = in.flags;
  KasResolvedLaunch L;
  L.cells16 = in.cells16;
  // per-chunk histograms: what the shape allows unless switched off (or the general fill is forced)
  const bool fused = in.fused && !(uf & (KAS_FLAG_TWO_PASS_HIST | KAS_FLAG_GENERIC_FILL));
  const bool rtn_quota = in.lane_order_ok && !(uf & KAS_FLAG_NO_RTN_QUOTA);   // the fill draws its quota with the atomic-with-return
  const int32_t idl = kas_relax_idl(s, c16, in.relax_gather != 0);
  // index rows (KAS_FLAG_INDEX_ROWS; the kernel still decides per topic: rows of the batch's width, a direct id table): int32
  // cells, lists up to 3 wide, per-chunk histograms, the quota drawn with the atomic-with-return
  const bool index_rows = !c16 && kas_index_rows_wanted(in.index_rows_bits) && Wc <= 3 && fused && rtn_quota && s.n_max < 0x3fff &&
                          s.idmap_entries > 0;
  // chunks per scenario of the spread fill, or 0 (one-workgroup fill kernel): its kernels read int32 cells, exist for lists 3 to 5
  // wide, and the quota kernel puts scenarios on grid.y and nodes on grid.x
  int32_t chunks = 0;
  if (!c16 && in.NW == 4 && Wc >= 3 && Wc <= 5 && (in.built & KAS_BUILT_SPREAD) && !(uf & KAS_FLAG_GENERIC_FILL) && s.n_max > 0 && S <= 65535 &&
      kas_fill_lds_layout(s.n_max, Wc, 4, s.idmap_entries, s.need_bsearch, 1).total <= KAS_LDS_LIMIT)
    chunks = kas_spread_chunks(s, S, in.single_topic != 0, (uf & KAS_FLAG_SPREAD_FILL) != 0);
  L.spread_chunks = chunks;
  // the order form
  const bool relax = s.relax_ok && in.lane_order_ok && (in.built & KAS_BUILT_RELAX) && !(uf & KAS_FLAG_ROUND_ORDER) &&
                     !(kas_flags_want_tickets(uf) && s.tickets_ok);
  const bool tickets = !relax && s.tickets_ok && !(uf & KAS_FLAG_ROUND_ORDER) && !c16;   // (no ticket form with 16-bit cells: the round form)
  const int32_t packed = s.packed_ok && !(uf & KAS_FLAG_WIDE_COUNTERS) ? 1 : 0;
  const bool pairing = tickets && in.G > 1 && S > in.G;
  const bool relaxw = !relax && !c16 && s.relaxw_ok && in.lane_order_ok && (in.built & KAS_BUILT_RELAXW) && kas_relaxw_wanted(uf);
  const bool wide = !tickets && !relaxw && !c16 && s.wide_ok && !(uf & KAS_FLAG_ROUND_ORDER) && (in.built & KAS_BUILT_WIDE);
  L.order_form = relax ? 3 : (relaxw ? 4 : (tickets ? 1 : (wide ? 2 : 0)));
  if (s.relax_ok && !relax && !(uf & KAS_FLAG_ROUND_ORDER) && !kas_flags_want_tickets(uf))
    L.relax_off = in.lane_order_state == 0 ? 1 : (in.lane_order_state == -2 ? 2 : 3);
  const uint32_t generic = s.with_x ? 0u : KAS_FLAG_GENERIC_FILL;
  L.flags = (uf & ~(KAS_FLAG_FUSED_HIST | KAS_FLAG_ORDER_FLAGGED | KAS_FLAG_WIDE_CHECK)) | generic | (fused ? KAS_FLAG_FUSED_HIST : 0u) |
            (kas_relax_double_tiles(uf, S) ? KAS_FLAG_RELAX_DUAL : 0u) | (rtn_quota ? KAS_FLAG_LANE_ORDER : 0u) |
            (c16 ? KAS_FLAG_CELLS16 : 0u) | (index_rows ? KAS_FLAG_INDEX_ROWS : 0u);
  // dword mid rows: every kernel of this solve moves mid rows as one dword each
  const bool m32 = kas_mid32_launch(s, c16, in.mid32_bits, relax, uf, idl, index_rows, chunks);
  if (m32) L.flags |= KAS_FLAG_MID32;
  // relaxation form: tile size, and first fit as a second wavefront of its workgroup?
  int32_t tiles = 0;
  bool p4_order = false;
  if (relax) {
    tiles = Wc == 3 && kas_relax_double_tiles(uf, S);
    if (tiles && m32 && kas_relax_quad_tiles(uf, S) && kas_order_relax_lds(s.n_max, 2, 0, 1) <= KAS_LDS_LIMIT) tiles = 2;   // (the instances on dword mid rows)
    const bool relax_plain = !s.any_ctx && (uf >> 24) == 0u && (c16 || idl) && (in.built & KAS_BUILT_P4_ORDER) && in.have_p4s;
    p4_order = kas_p4_with_order(s, in.NW, uf | generic, chunks, S, relax_plain, tiles, idl);
  }
  // the fill kernel hands first fit over: to kas_p4_kernel, or to kas_p4_order_kernel
  const bool split_p4 = p4_order || (in.have_p4s && kas_split_p4(s, in.NW, uf | generic, chunks, S));
  L.flags = split_p4 ? (L.flags | KAS_FLAG_SPLIT_P4) : (L.flags & ~KAS_FLAG_SPLIT_P4);   // (the kernels' bit: this launch's form)
  // the slim fill kernel in front (with kas_fill_kernel behind it for the scenarios it hands back): int32 cells, lists up to 3 wide,
  // per-chunk histograms on 4 wavefronts, the quota drawn with the atomic-with-return, a direct id table for every scenario, no
  // index rows, first fit handed over, no spread fill
  const bool slim = KAS_SLIM_FILL_DEFAULT && !in.full_fill && !c16 && Wc <= 3 && in.NW == 4 && (in.built & KAS_BUILT_SLIM) && fused && s.with_x &&
                    rtn_quota && !index_rows && split_p4 && chunks == 0 && s.idmap_entries > 0 && !s.need_bsearch && in.have_back_flags;

  auto add = [&L](int32_t role, int32_t family, uint32_t gx, uint32_t gy, uint32_t block, int64_t lds, uint32_t flags) -> KasStage& {
    KasStage& st = L.stages[L.n_stages++];
    st.role = role; st.k.family = family;
    st.grid_x = gx; st.grid_y = gy; st.block = block; st.lds = (uint32_t)lds; st.flags = flags;
    return st;
  };
  const uint32_t uS = (uint32_t)S;
  int32_t sp_flag = KAS_SP_FLAG_NONE;
  if (chunks > 0) {
    sp_flag = KAS_SP_FLAG_PLAN;
    const int32_t fam[4] = {KAS_K_SPREAD_A, KAS_K_SPREAD_Q, KAS_K_SPREAD_B, KAS_K_SPREAD_P4};
    for (int32_t i = 0; i < 4; ++i) {
      const int32_t mode = i == 0 ? 1 : (i == 2 ? 2 : 3);
      const int64_t lds = i == 1 ? 0 : kas_spread_scan_lds(s.n_max, Wc, s.idmap_entries, s.need_bsearch, mode).total;
      KasStage& st = i == 1 ? add(KAS_STAGE_SPREAD, fam[i], (uint32_t)((s.n_max + 255) / 256), uS, 256u, lds, L.flags)
                   : i == 3 ? add(KAS_STAGE_SPREAD, fam[i], uS, 1u, 64u * KAS_SPREAD_P4_WAVES, lds, L.flags)
                            : add(KAS_STAGE_SPREAD, fam[i], (uint32_t)chunks, uS, 64u, lds, L.flags);
      st.k.W = Wc; st.sp_flag = sp_flag; st.spread = 1;
    }
  }
  const uint32_t fill_block = 64u * (uint32_t)in.NW;
  if (slim) {
    // the slim kernel takes every scenario (and writes each one's hand-back flag, 0 or 1); the full kernel behind it takes the
    // flagged ones on a small grid
    sp_flag = KAS_SP_FLAG_PLAN;
    KasStage& st = add(KAS_STAGE_SLIM, KAS_K_FILL_SLIM, uS, 1u, fill_block,
                       (int64_t)kas_fill_slim_lds(s.n_max, Wc, s.idmap_entries).total + KAS_TUNE_SLIM_LDS_PAD, L.flags);
    st.k.W = Wc; st.k.m32 = m32; st.sp_flag = sp_flag;
  }
  const int64_t fill_lds = (int64_t)(fused ? in.lds_fused_total : in.lds_total) + KAS_TUNE_FILL_LDS_PAD;
  {
    // (what is left behind the spread / slim fill: the scenarios handed back)
    KasStage& st = add(KAS_STAGE_FILL, KAS_K_FILL, slim ? kas_back_grid(in.last_handback, uS) : uS, 1u, fill_block, fill_lds,
                       L.flags | (sp_flag != KAS_SP_FLAG_NONE ? KAS_FLAG_ONLY_FLAGGED : 0u));
    st.k.W = Wc; st.k.NW = in.NW; st.sp_flag = sp_flag; st.spread = chunks > 0; st.handback = slim;
  }
  if (split_p4 && !p4_order) {
    KasStage& st = add(KAS_STAGE_P4, KAS_K_P4, uS, 1u, 64u * KAS_P4_KERNEL_WAVES, kas_p4_lds_layout(s.n_max).total, L.flags);
    st.k.W = Wc; st.k.m32 = m32; st.sp_flag = sp_flag; st.spread = chunks > 0;
  }
  // lists 4-5 wide and a node that may hold 1023 .. 2039 rows: the wide form checks its 10-bit count fields when the last row has
  // retired and flags a scenario that outgrew them.  Its rows are finished (on wrong counts) by then and its mid rows gone, so it
  // is solved again from `cur`: fill kernel, then round form, both taking only the flagged scenarios.
  const bool wide_recheck = wide && s.wide_checked;
  // a Context handed in: the order kernels flag the scenarios whose counters do not fit their count fields, and the round form
  // (launched behind them, taking only those) serves them
  const bool round_flagged = (s.any_ctx && (tickets || wide || relax)) || wide_recheck;
  const uint32_t oflags = L.flags | (wide_recheck ? KAS_FLAG_WIDE_CHECK : 0u);
  if (pairing) {
    // scenarios that share a solver wavefront should have P5 chains of similar length
    KasStage& st = add(KAS_STAGE_PERMUTATION, KAS_K_PERMUTATION, 1u, 1u, 64u * KAS_PERM_WAVES, (int64_t)sizeof(int32_t) * (KAS_PERM_BINS + 8), oflags);
    st.sp_flag = sp_flag; st.spread = chunks > 0; st.perm = 1;
  }
  {
    KasStage* st;
    if (relax && p4_order) {
      st = &add(KAS_STAGE_ORDER, KAS_K_P4_ORDER, uS, 1u, 128u, kas_p4_order_lds(s.n_max, tiles, idl), oflags);
      st->k.tiles = tiles; st->k.c16 = c16; st->k.idl = idl; st->k.m32 = m32;
    } else if (relax) {
      st = &add(KAS_STAGE_ORDER, KAS_K_ORDER_RELAX, uS, 1u, 64u, kas_order_relax_lds(s.n_max, tiles, s.any_ctx, idl), oflags);
      st->k.tiles = tiles; st->k.ctx = s.any_ctx; st->k.verify = (uf >> 24) != 0u; st->k.c16 = c16; st->k.idl = idl; st->k.m32 = m32;
    } else if (relaxw) {
      st = &add(KAS_STAGE_ORDER, KAS_K_ORDER_RELAX_WIDE, uS, 1u, 64u, kas_order_relaxw_lds(s.n_max, Wc), oflags);
    } else if (tickets) {
      st = &add(KAS_STAGE_ORDER, KAS_K_ORDER_TICKET, (uint32_t)((S + in.G - 1) / in.G), 1u, 192u,
                (int64_t)kas_order_ticket_lds(s.n_max, in.G, packed) + KAS_TUNE_ORDER_LDS_PAD, oflags);
      st->k.G = in.G; st->k.packed = packed;
    } else if (wide) {
      st = &add(KAS_STAGE_ORDER, KAS_K_ORDER_WIDE, uS, 1u, (uint32_t)KAS_ORDER_WIDE_BLOCK, kas_order_wide_lds(s.n_max), oflags);
    } else {
      st = &add(KAS_STAGE_ORDER, KAS_K_ORDER_ROUND, uS, 1u, 64u, kas_order_round_lds(s.n_max, Wc), oflags);
    }
    st->k.W = Wc; st->sp_flag = sp_flag; st->spread = chunks > 0; st->perm = pairing;
  }
  if (wide_recheck) {
    // (this fill does its own first fit; ord_flag has sp_flag's meaning: != 0, this kernel takes the scenario)
    KasStage& st = add(KAS_STAGE_REFILL, KAS_K_FILL, uS, 1u, fill_block, fill_lds, (L.flags | KAS_FLAG_ONLY_FLAGGED) & ~KAS_FLAG_SPLIT_P4);
    st.k.W = Wc; st.k.NW = in.NW; st.sp_flag = KAS_SP_FLAG_ORD; st.spread = chunks > 0;
  }
  if (round_flagged) {
    KasStage& st = add(KAS_STAGE_ROUND_FLAGGED, KAS_K_ORDER_ROUND, uS, 1u, 64u, kas_order_round_lds(s.n_max, Wc), oflags | KAS_FLAG_ORDER_FLAGGED);
    st.k.W = Wc; st.sp_flag = sp_flag; st.spread = chunks > 0;
  }
  return L;
}

// The kernel identities a plan in this state may launch, whatever kas_plan_set_flags is told next and whatever the context's
// self-test says later: fn(stage) for every stage of the resolver over the switches that select an instance or an LDS size — order
// form, packed counters, tile size, sampled verification, where first fit runs, mid rows, per-chunk histograms, the spread fill.
// (The other switches — index rows, full fill, general fill, quota draw — only take stages away.)
template <typename Fn>
static inline void kas_enumerate_launches(KasLaunchIn in, Fn fn) {
  static const uint32_t order_sw[] = {0u, KAS_FLAG_ROUND_ORDER, KAS_FLAG_TICKET_ORDER, KAS_FLAG_TICKET_ORDER | KAS_FLAG_WIDE_COUNTERS};
  static const uint32_t tile_sw[] = {KAS_FLAG_RELAX_TILES_64, KAS_FLAG_RELAX_TILES_128, KAS_FLAG_RELAX_TILES_64 | KAS_FLAG_RELAX_TILES_128};
  static const uint32_t p4_sw[] = {KAS_FLAG_SPLIT_P4, KAS_FLAG_FILL_WITH_P4, KAS_FLAG_P4_WITH_ORDER};
  static const uint32_t mid_sw[] = {KAS_PLAN_NO_MID32_BIT, KAS_PLAN_MID32_BIT};
  const int32_t lane_now = in.lane_order_ok;
  for (int32_t lane = lane_now ? 1 : 0; lane >= 0; --lane)      // (a context's self-test may still fail: the forms without lane order)
    for (uint32_t o : order_sw) for (uint32_t t : tile_sw) for (uint32_t p4 : p4_sw) for (uint32_t mid : mid_sw)
      for (uint32_t verify = 0; verify < 2u; ++verify) for (uint32_t hist = 0; hist < 2u; ++hist) for (uint32_t spread = 0; spread < 2u; ++spread) {
        const uint32_t word = o | t | p4 | mid | (verify << 24) | (hist ? KAS_FLAG_TWO_PASS_HIST : 0u) | (spread ? KAS_FLAG_SPREAD_FILL : 0u) |
                              KAS_PLAN_NO_INDEX_ROWS_BIT;
        if (kas_flags_refusal(*in.shape, in.cells16 != 0, word, in.relax_gather != 0)) continue;
        in.lane_order_ok = lane;
        kas_launch_in_user_flags(&in, word);
        const KasResolvedLaunch L = kas_resolve_launch(in);
        for (int32_t i = 0; i < L.n_stages; ++i) fn(L.stages[i]);
      }
}

static inline std::string kas_kernel_name(const KasKernelId& k) {
  char b[160];
  const char* mids = k.idl ? (k.m32 ? ", ids in LDS, dword mid rows" : ", ids in LDS") : "";
  switch (k.family) {
    case KAS_K_FILL_SLIM: snprintf(b, sizeof(b), "kas_fill_slim_kernel<%d>", k.W); break;
    case KAS_K_FILL: snprintf(b, sizeof(b), "kas_fill_kernel<%d,%d>", k.W, k.NW); break;
    case KAS_K_P4: snprintf(b, sizeof(b), "kas_p4_kernel<%d>", k.W); break;
    case KAS_K_PERMUTATION: snprintf(b, sizeof(b), "kas_order_permutation_kernel"); break;
    case KAS_K_ORDER_RELAX:
      snprintf(b, sizeof(b), "kas_order_relax_kernel<%d>[tiles of %d rows%s%s]", k.W, 64 << k.tiles, mids, k.verify ? ", sampled verification" : "");
      break;
    case KAS_K_P4_ORDER:
      snprintf(b, sizeof(b), "kas_p4_order_kernel<%d>[first fit beside kas_order_relax_kernel<%d>[tiles of %d rows%s] in one workgroup]", k.W, k.W,
               64 << k.tiles, mids);
      break;
    case KAS_K_ORDER_RELAX_WIDE: snprintf(b, sizeof(b), "kas_order_relax_wide_kernel<%d>[tiles of 64 rows, ids in LDS]", k.W); break;
    case KAS_K_ORDER_TICKET: snprintf(b, sizeof(b), "kas_order_ticket_kernel<%d,%d,%s>", k.W, k.G, k.packed ? "true" : "false"); break;
    case KAS_K_ORDER_WIDE: snprintf(b, sizeof(b), "kas_order_wide_kernel<%d>", k.W); break;
    case KAS_K_ORDER_ROUND: snprintf(b, sizeof(b), "kas_order_round_kernel<%d>", k.W); break;
    default: snprintf(b, sizeof(b), "kas_spread_{a,q,b,p4}_kernel<%d>", k.W); break;
  }
  return b;
}

// the text of kas_plan_describe: rendered from the stages that are launched
static inline std::string kas_describe_launch(const KasResolvedLaunch& L) {
  auto launch = [](const KasStage& st, const char* attr) {
    char b[96];
    snprintf(b, sizeof(b), "%s grid=%ux%u lds=%u", attr, st.grid_x, st.block, st.lds);
    return kas_kernel_name(st.k) + b;
  };
  const KasStage* fill = L.find(KAS_STAGE_FILL);
  const KasStage* order = L.find(KAS_STAGE_ORDER);
  const char* attr = (L.flags & KAS_FLAG_GENERIC_FILL) ? "[sweeps]"
                     : !(L.flags & KAS_FLAG_FUSED_HIST) ? "[quota]"
                     : ((L.flags & KAS_FLAG_INDEX_ROWS) && L.spread_chunks == 0) ? "[quota, chunk histograms, index rows]" : "[quota, chunk histograms]";
  std::string out;
  if (const KasStage* sp = L.find(KAS_STAGE_SPREAD)) {
    char b[96];
    snprintf(b, sizeof(b), " %d chunks x %u scenarios (rows not rack-diverse: ", L.spread_chunks, sp->grid_y);
    out = kas_kernel_name(sp->k) + b + launch(*fill, attr) + ")";
  } else if (const KasStage* slim = L.find(KAS_STAGE_SLIM)) {
    out = launch(*slim, attr) + " (+ " + launch(*fill, attr) + " for scenarios it hands back)";
  } else {
    out = launch(*fill, attr);
  }
  if (const KasStage* p4 = L.find(KAS_STAGE_P4)) out += " + " + launch(*p4, "");   // first fit (P4) is a launch of its own between the two
  out += " + ";
  if (L.find(KAS_STAGE_PERMUTATION)) out += "kas_order_permutation_kernel + ";
  out += launch(*order, "");
  if (L.find(KAS_STAGE_REFILL)) out += " [count fields checked at the end; kas_fill_kernel + kas_order_round_kernel for scenarios it flags]";
  else if (L.find(KAS_STAGE_ROUND_FLAGGED)) out += " [Context in/out; kas_order_round_kernel for scenarios it flags]";
  if (L.relax_off)                                             // the form the shape allows is not the one launched: say why
    out += std::string(" [relaxation form off: LDS lane-order self-test ") +
           (L.relax_off == 1 ? "FAILED" : (L.relax_off == 2 ? "switched off (KAS_NO_LANE_ORDER)" : "could not run")) + "]";
  if (L.cells16) out += " [16-bit cells]";
  return out;
}
