// kas_racks.hip — gfx950 kernels of the rack pass (kas_rack_impact_device / kas_solve_host_rack_impact in kas_hip.hip).
// Launch arguments and host tables: kas_racks.h; device code: kas_racks_body.h.  A translation unit of its own, so that
// nothing here changes how the kernels of kas_hip.hip and kas_impact.hip are compiled.
#include <hip/hip_runtime.h>

#include "kas_racks_body.h"

// one workgroup per item of the impact pass's work list; W = cells a row may hold (the plan's width class), C16 = 16-bit cells
template <int W, bool C16>
__global__ __launch_bounds__(KAS_RACK_BLOCK) void kas_rack_rows_kernel(KasRackLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_rack_rows_lds[];
  kasr::rack_item<W, C16>(a, (int32_t)blockIdx.x, kas_rack_rows_lds);
}

// one workgroup per scenario
__global__ __launch_bounds__(KAS_RACK_BLOCK) void kas_rack_reduce_kernel(KasRackLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_rack_reduce_lds[];
  kasr::rack_reduce(a, (int32_t)blockIdx.x, kas_rack_reduce_lds);
}

typedef void (*kas_rack_fn)(KasRackLaunch);

template <bool C16>
static kas_rack_fn kas_rack_rows_for(int32_t wc) {
  return wc <= 3 ? kas_rack_rows_kernel<3, C16> : (wc <= 5 ? kas_rack_rows_kernel<5, C16> : kas_rack_rows_kernel<8, C16>);
}

int kas_rack_launch(const KasRackLaunch* a, int32_t wc, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  hipError_t e;
  if (a->lds_bytes > KAS_RACK_LDS_LIMIT || a->reduce_lds_bytes > KAS_RACK_LDS_LIMIT) return (int)hipErrorInvalidValue;
  if (a->n_items > 0) {
    const kas_rack_fn fn = a->cells16 ? kas_rack_rows_for<true>(wc) : kas_rack_rows_for<false>(wc);
    if ((e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, a->lds_bytes)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3((unsigned)a->n_items), dim3(KAS_RACK_BLOCK), (size_t)a->lds_bytes, st, *a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  if (a->n_scenarios > 0) {
    if ((e = hipFuncSetAttribute((const void*)kas_rack_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, a->reduce_lds_bytes)) != hipSuccess)
      return (int)e;
    hipLaunchKernelGGL(kas_rack_reduce_kernel, dim3((unsigned)a->n_scenarios), dim3(KAS_RACK_BLOCK), (size_t)a->reduce_lds_bytes, st, *a);
    return (int)hipGetLastError();
  }
  return (int)hipSuccess;
}
