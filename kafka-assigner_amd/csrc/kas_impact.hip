// kas_impact.hip — gfx950 kernels of the impact pass (ABI v6: kas_impact_device / kas_solve_host_impact in kas_hip.hip).
// Work list and launch arguments: kas_impact.h; device code: kas_impact_body.h.  A translation unit of its own, so that
// nothing here changes how the solve kernels of kas_hip.hip are compiled.
#include <hip/hip_runtime.h>

#include "kas_impact_body.h"

// one workgroup per item; W = cells a row may hold (the plan's width class), C16 = 16-bit node-index cells
template <int W, bool C16>
__global__ __launch_bounds__(KAS_IMPACT_BLOCK) void kas_impact_kernel(KasImpactLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_impact_lds[];
  kasi::impact_item<W, C16>(a, (int32_t)blockIdx.x, kas_impact_lds);
}

// one workgroup per scenario with its counters in global scratch
__global__ __launch_bounds__(KAS_IMPACT_BLOCK) void kas_impact_merge_kernel(KasImpactLaunch a) {
  __shared__ int32_t red[KAS_IMPACT_FIELDS * (KAS_IMPACT_BLOCK / 64)];
  kasi::impact_merge(a, (int32_t)blockIdx.x, red);
}

typedef void (*kas_impact_fn)(KasImpactLaunch);

template <bool C16>
static kas_impact_fn kas_impact_for(int32_t wc) {
  return wc <= 3 ? kas_impact_kernel<3, C16> : (wc <= 5 ? kas_impact_kernel<5, C16> : kas_impact_kernel<8, C16>);
}

int kas_impact_launch(const KasImpactLaunch* a, int32_t wc, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  if (a->n_items > 0) {
    const kas_impact_fn fn = a->cells16 ? kas_impact_for<true>(wc) : kas_impact_for<false>(wc);
    hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, a->lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3((unsigned)a->n_items), dim3(KAS_IMPACT_BLOCK), (size_t)a->lds_bytes, st, *a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  if (a->n_merge > 0) {
    hipLaunchKernelGGL(kas_impact_merge_kernel, dim3((unsigned)a->n_merge), dim3(KAS_IMPACT_BLOCK), 0, st, *a);
    return (int)hipGetLastError();
  }
  return (int)hipSuccess;
}
