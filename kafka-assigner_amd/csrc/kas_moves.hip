// kas_moves.hip — gfx950 kernels of the moves pass (kas_moves_device / kas_solve_host_moves / kas_solve_host_choose_moves in
// kas_hip.hip).  Tables and launch arguments: kas_moves.h; device code: kas_moves_body.h.  A translation unit of its own, so
// that nothing here changes how the kernels of kas_hip.hip, kas_impact.hip and kas_choose.hip are compiled.
#include <hip/hip_runtime.h>

#include "kas_moves_body.h"

// one workgroup per (listed scenario, item); W = cells a row may hold (the plan's width class), C16 = 16-bit source cells
template <int W, bool C16>
__global__ __launch_bounds__(KAS_MOVES_BLOCK) void kas_moves_count_kernel(KasMovesLaunch a) {
  __shared__ int32_t red[2 * kasm::WAVES];
  kasm::count_item<W, C16>(a, (int32_t)blockIdx.x, red);
}

// the one workgroup that scans the (listed scenario, item) table
__global__ __launch_bounds__(KAS_MOVES_BLOCK) void kas_moves_scan_kernel(KasMovesLaunch a) {
  __shared__ int32_t red[2 * kasm::WAVES];
  kasm::scan_all(a, red);
}

template <int W, bool C16>
__global__ __launch_bounds__(KAS_MOVES_BLOCK) void kas_moves_emit_kernel(KasMovesLaunch a) {
  __shared__ int32_t sub[2 * kasm::GROUPS];
  kasm::emit_item<W, C16>(a, (int32_t)blockIdx.x, sub);
}

typedef void (*kas_moves_fn)(KasMovesLaunch);

template <bool C16>
static kas_moves_fn kas_moves_count_for(int32_t wc) {
  return wc <= 3 ? kas_moves_count_kernel<3, C16> : (wc <= 5 ? kas_moves_count_kernel<5, C16> : kas_moves_count_kernel<8, C16>);
}
template <bool C16>
static kas_moves_fn kas_moves_emit_for(int32_t wc) {
  return wc <= 3 ? kas_moves_emit_kernel<3, C16> : (wc <= 5 ? kas_moves_emit_kernel<5, C16> : kas_moves_emit_kernel<8, C16>);
}

int kas_moves_launch(const KasMovesLaunch* a, int32_t wc, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t grid = (int64_t)a->n * a->stride;
  if (a->n < 0 || a->stride < 1 || grid > INT32_MAX) return (int)hipErrorInvalidConfiguration;
  hipError_t e;
  if (grid > 0) {
    hipLaunchKernelGGL(a->src16 ? kas_moves_count_for<true>(wc) : kas_moves_count_for<false>(wc), dim3((unsigned)grid), dim3(KAS_MOVES_BLOCK), 0, st, *a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kas_moves_scan_kernel, dim3(1), dim3(KAS_MOVES_BLOCK), 0, st, *a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (grid > 0 && (a->moves_cap > 0 || a->cells_cap > 0)) {
    hipLaunchKernelGGL(a->src16 ? kas_moves_emit_for<true>(wc) : kas_moves_emit_for<false>(wc), dim3((unsigned)grid), dim3(KAS_MOVES_BLOCK), 0, st, *a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  return (int)hipSuccess;
}
