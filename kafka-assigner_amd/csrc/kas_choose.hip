// kas_choose.hip — gfx950 kernels that choose the best scenarios of a solve (kas_rank_device / kas_choose_device /
// kas_solve_host_choose in kas_hip.hip) or mark and rank their Pareto front (kas_front_rank_device / kas_front_device /
// kas_solve_host_front), and the instances of the rank, mark and front rank kernels that read the scenario rack records too
// (the *_racks entries) or those and the scenario topic records (the *_topics entries).  Tables and launch arguments:
// kas_choose.h, kas_front.h; device code: kas_choose_body.h, kas_front_body.h.  A translation unit of its own, so that nothing
// here changes how the kernels of kas_hip.hip and kas_impact.hip are compiled.
#include <hip/hip_runtime.h>

#include "kas_choose_body.h"
#include "kas_front_body.h"

// one lane per scenario (and one more): every workgroup streams all S keys through its LDS tile
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_rank_kernel(KasChooseLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasc::rank_block(a, (int32_t)blockIdx.x, tile);
}

// one workgroup per (chosen scenario, chunk of its packed rows and node block)
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_gather_kernel(KasChooseLaunch a) {
  kasc::gather_item(a, (int64_t)blockIdx.x);
}

// one lane per scenario: every workgroup streams all S scenarios through its LDS tile and tests each against its lanes' own
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_front_mark_kernel(KasFrontLaunch a) {
  __shared__ kasf::Entry tile[KAS_CHOOSE_TILE];
  kasf::mark_block(a, (int32_t)blockIdx.x, tile);
}

// the rank kernel's loop over the members of the front (the classes kas_front_mark_kernel left)
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_front_rank_kernel(KasFrontLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasf::rank_block(a, (int32_t)blockIdx.x, tile);
}

// The instances that also read the scenario rack records (rack criteria, KAS_KEY_RACK_BASE): same grids, same tiles.
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_rank_racks_kernel(KasRackChooseLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasc::rank_block(a.c, (int32_t)blockIdx.x, tile, kasc::ByStatus(), kasc::RackRecords{a.srk});
}

__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_front_mark_racks_kernel(KasRackFrontLaunch a) {
  __shared__ kasf::Entry tile[KAS_CHOOSE_TILE];
  kasf::mark_block(a.f, (int32_t)blockIdx.x, tile, kasc::RackRecords{a.srk});
}

__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_front_rank_racks_kernel(KasRackFrontLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasf::rank_block(a.f, (int32_t)blockIdx.x, tile, kasc::RackRecords{a.srk});
}

// The instances that read the scenario rack records and the scenario topic records (topic criteria, KAS_KEY_TOPIC_BASE): same
// grids, same tiles; they differ in the loads of entry_of alone.
__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_rank_topics_kernel(KasTopicChooseLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasc::rank_block(a.c, (int32_t)blockIdx.x, tile, kasc::ByStatus(), kasc::TopicRecords{a.srk, a.stp});
}

__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_front_mark_topics_kernel(KasTopicFrontLaunch a) {
  __shared__ kasf::Entry tile[KAS_CHOOSE_TILE];
  kasf::mark_block(a.f, (int32_t)blockIdx.x, tile, kasc::TopicRecords{a.srk, a.stp});
}

__global__ __launch_bounds__(KAS_CHOOSE_BLOCK) void kas_front_rank_topics_kernel(KasTopicFrontLaunch a) {
  __shared__ kasc::Entry tile[KAS_CHOOSE_TILE];
  kasf::rank_block(a.f, (int32_t)blockIdx.x, tile, kasc::TopicRecords{a.srk, a.stp});
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

int kas_front_mark_launch(const KasFrontLaunch* a, void* hip_stream) {
  hipLaunchKernelGGL(kas_front_mark_kernel, dim3((unsigned)kas_front_mark_grid(a->c.S)), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_front_rank_launch(const KasFrontLaunch* a, void* hip_stream) {
  const unsigned grid = (unsigned)(((int64_t)a->c.S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK);
  hipLaunchKernelGGL(kas_front_rank_kernel, dim3(grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_rank_racks_launch(const KasRackChooseLaunch* a, void* hip_stream) {
  const unsigned grid = (unsigned)(((int64_t)a->c.S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK);
  hipLaunchKernelGGL(kas_rank_racks_kernel, dim3(grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_front_mark_racks_launch(const KasRackFrontLaunch* a, void* hip_stream) {
  hipLaunchKernelGGL(kas_front_mark_racks_kernel, dim3((unsigned)kas_front_mark_grid(a->f.c.S)), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_front_rank_racks_launch(const KasRackFrontLaunch* a, void* hip_stream) {
  const unsigned grid = (unsigned)(((int64_t)a->f.c.S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK);
  hipLaunchKernelGGL(kas_front_rank_racks_kernel, dim3(grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_rank_topics_launch(const KasTopicChooseLaunch* a, void* hip_stream) {
  const unsigned grid = (unsigned)(((int64_t)a->c.S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK);
  hipLaunchKernelGGL(kas_rank_topics_kernel, dim3(grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_front_mark_topics_launch(const KasTopicFrontLaunch* a, void* hip_stream) {
  hipLaunchKernelGGL(kas_front_mark_topics_kernel, dim3((unsigned)kas_front_mark_grid(a->f.c.S)), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}

int kas_front_rank_topics_launch(const KasTopicFrontLaunch* a, void* hip_stream) {
  const unsigned grid = (unsigned)(((int64_t)a->f.c.S + 1 + KAS_CHOOSE_BLOCK - 1) / KAS_CHOOSE_BLOCK);
  hipLaunchKernelGGL(kas_front_rank_topics_kernel, dim3(grid), dim3(KAS_CHOOSE_BLOCK), 0, (hipStream_t)hip_stream, *a);
  return (int)hipGetLastError();
}
