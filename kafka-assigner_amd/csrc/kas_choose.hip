// kas_choose.hip — gfx950 kernels that choose the best scenarios of a solve (kas_rank_device / kas_choose_device /
// kas_solve_host_choose in kas_hip.hip).  Tables and launch arguments: kas_choose.h; device code: kas_choose_body.h.  A
// translation unit of its own, so that nothing here changes how the kernels of kas_hip.hip and kas_impact.hip are compiled.
#include <hip/hip_runtime.h>

#include "kas_choose_body.h"

// one lane per scenario (and one more): every workgroup streams all S keys through its LDS tile
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_rank_kernel(KasChooseLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasc::rank_block(a, (int32_t)blockIdx.x, tile);
}

// one workgroup per (chosen scenario, chunk of its packed rows and node block)
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_gather_kernel(KasChooseLaunch a) {
  kasc::gather_item(a, (int64_t)blockIdx.x);
}

int kas_rank_launch(const KasChooseLaunch* a, void* hip_stream) {
  const unsigned grid = (unsigned)(((int64_t)a->S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK);
  hipLaunchKernelGGL(kas_rank_kernel, dim3(grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_gather_launch(const KasChooseLaunch* a, void* hip_stream) {
  const int64_t grid = (int64_t)a->k * a->chunks;
  if (grid <= 0) return (int)hipSuccess;
  if (grid > INT32_MAX) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(kas_gather_kernel, dim3((unsigned)grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}
