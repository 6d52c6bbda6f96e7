// kas_topics.hip — gfx950 kernels of the topic pass (kas_topic_impact_device / kas_solve_host_topic_impact in kas_hip.hip).
// Launch arguments and work list: kas_topics.h; device code: kas_topics_body.h.  A translation unit of its own, so that nothing
// here changes how the kernels of kas_hip.hip, kas_impact.hip and kas_racks.hip are compiled.
#include <hip/hip_runtime.h>

#include "kas_topics_body.h"

// one workgroup per item; W = cells a row may hold (the plan's width class), C16 = 16-bit node-index cells
template <int W, bool C16>
__global__ __launch_bounds__(KAS_TOPIC_BLOCK) void kas_topic_item_kernel(KasTopicLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kas_topic_lds[];
  kast::topic_item<W, C16>(a, (int32_t)blockIdx.x, kas_topic_lds);
}

// one workgroup per topic with its counters in global scratch
__global__ __launch_bounds__(KAS_TOPIC_BLOCK) void kas_topic_merge_kernel(KasTopicLaunch a) {
  __shared__ int32_t red[KAS_TOPIC_RED * (KAS_TOPIC_BLOCK / 64)];
  kast::topic_merge(a, (int32_t)blockIdx.x, red);
}

// one workgroup per scenario, behind the two above
__global__ __launch_bounds__(KAS_TOPIC_BLOCK) void kas_topic_summary_kernel(KasTopicLaunch a) {
  __shared__ int32_t red[KAS_TOPIC_WORDS * (KAS_TOPIC_BLOCK / 64)];
  kast::topic_summary(a, (int32_t)blockIdx.x, red);
}

typedef void (*kas_topic_fn)(KasTopicLaunch);

template <bool C16>
static kas_topic_fn kas_topic_item_for(int32_t wc) {
  return wc <= 3 ? kas_topic_item_kernel<3, C16> : (wc <= 5 ? kas_topic_item_kernel<5, C16> : kas_topic_item_kernel<8, C16>);
}

int kas_topic_launch(const KasTopicLaunch* a, int32_t wc, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  hipError_t e;
  if (a->lds_bytes > KAS_TOPIC_LDS_LIMIT) return (int)hipErrorInvalidValue;
  if (a->n_items > 0) {
    const kas_topic_fn fn = a->cells16 ? kas_topic_item_for<true>(wc) : kas_topic_item_for<false>(wc);
    if ((e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, a->lds_bytes)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3((unsigned)a->n_items), dim3(KAS_TOPIC_BLOCK), (size_t)a->lds_bytes, st, *a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  if (a->n_merge > 0) {
    hipLaunchKernelGGL(kas_topic_merge_kernel, dim3((unsigned)a->n_merge), dim3(KAS_TOPIC_BLOCK), 0, st, *a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  if (a->n_scenarios > 0) {
    hipLaunchKernelGGL(kas_topic_summary_kernel, dim3((unsigned)a->n_scenarios), dim3(KAS_TOPIC_BLOCK), 0, st, *a);
    return (int)hipGetLastError();
  }
  return (int)hipSuccess;
}
