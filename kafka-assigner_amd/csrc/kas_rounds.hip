// kas_rounds.hip — the gfx950 kernel of the rounds pass (kas_rounds_device / kas_solve_host_rounds / 16 in kas_hip.hip).
// Launch arguments and LDS layout: kas_rounds.h; device code: kas_rounds_body.h.  A translation unit of its own, so that
// nothing here changes how the kernels of the other translation units are compiled.
#include <hip/hip_runtime.h>

#include "kas_rounds_body.h"

// one workgroup per listed scenario; W = cells a row may hold (the plan's width class), C16 = 16-bit source cells
template <int W, bool C16>
__global__ __launch_bounds__(KAS_ROUND_BLOCK) void kas_rounds_kernel(KasRoundsLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_rounds_lds_bytes[];
  kasr::rounds_scenario<W, C16>(a, (int32_t)blockIdx.x, kas_rounds_lds_bytes);
}

typedef void (*kas_rounds_fn)(KasRoundsLaunch);

template <bool C16>
static kas_rounds_fn kas_rounds_for(int32_t wc) {
  return wc <= 3 ? kas_rounds_kernel<3, C16> : (wc <= 5 ? kas_rounds_kernel<5, C16> : kas_rounds_kernel<8, C16>);
}

int kas_rounds_launch(const KasRoundsLaunch* a, int32_t wc, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  if (a->n < 0 || a->lds.total <= 0 || a->lds.total > KAS_ROUND_LDS_LIMIT) return (int)hipErrorInvalidConfiguration;
  if (a->n == 0) return (int)hipSuccess;
  const kas_rounds_fn fn = a->src16 ? kas_rounds_for<true>(wc) : kas_rounds_for<false>(wc);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, a->lds.total);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(fn, dim3((unsigned)a->n), dim3(KAS_ROUND_BLOCK), (size_t)a->lds.total, st, *a);
  return (int)hipGetLastError();
}
