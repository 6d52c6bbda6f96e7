// kas_batches.hip — the gfx950 kernel of the batches pass (kas_batches_device / kas_solve_host_batches / 16 in kas_hip.hip).
// Launch arguments and LDS layout: kas_batches.h; device code: kas_batches_body.h.  A translation unit of its own, so that
// nothing here changes how the kernels of the other translation units are compiled.
#include <hip/hip_runtime.h>

#include "kas_batches_body.h"

// one workgroup per listed scenario; W = cells a row may hold (the plan's width class), C16 = 16-bit source cells
template <int W, bool C16>
__global__ __launch_bounds__(KAS_BATCH_BLOCK) void kas_batches_kernel(KasBatchesLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_batches_lds_bytes[];
  kasb::batches_scenario<W, C16>(a, (int32_t)blockIdx.x, kas_batches_lds_bytes);
}

typedef void (*kas_batches_fn)(KasBatchesLaunch);

template <bool C16>
static kas_batches_fn kas_batches_for(int32_t wc) {
  return wc <= 3 ? kas_batches_kernel<3, C16> : (wc <= 5 ? kas_batches_kernel<5, C16> : kas_batches_kernel<8, C16>);
}

int kas_batches_launch(const KasBatchesLaunch* a, int32_t wc, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  if (a->n < 0 || a->lds.total <= 0 || a->lds.total > KAS_BATCH_LDS_LIMIT) return (int)hipErrorInvalidConfiguration;
  if (a->n == 0) return (int)hipSuccess;
  const kas_batches_fn fn = a->src16 ? kas_batches_for<true>(wc) : kas_batches_for<false>(wc);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, a->lds.total);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(fn, dim3((unsigned)a->n), dim3(KAS_BATCH_BLOCK), (size_t)a->lds.total, st, *a);
  return (int)hipGetLastError();
}
