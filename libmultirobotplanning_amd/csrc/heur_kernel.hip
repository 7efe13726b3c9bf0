// Shortest-path heuristic tables on the device (mrp_ll_compute_heuristics, mrp_ll_heuristic_lookup): the wave program of
// heur_bfs.h with one wavefront (= one 64-thread workgroup) per table, and the gather that hands single entries back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_dev.h"
#include "heur_bfs.h"
#include "ll_launch.h"  // HeurParams, LookupParams, the launchers' prototypes

namespace mrp {

// No static LDS: the dynamic window starts at LDS address 0 (wave_dev.h windowBase).  Its size is the largest
// hb::ldsBytes of the launch's tables.
extern "C" __global__ void __launch_bounds__(64) mrp_ll_heur_bfs_kernel(HeurParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem != 0u) __builtin_trap();
  if (blockIdx.x >= P.n) return;
  const hb::HeurJob job = P.jobs[blockIdx.x];
  hb::heurBfs(wv::windowBase(nullptr), P.maps, job);
}

extern "C" __global__ void __launch_bounds__(256) mrp_ll_heur_lookup_kernel(LookupParams P) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= P.n) return;
  const hb::LookupJob j = P.jobs[k];
  const uint32_t v = reinterpret_cast<const uint16_t*>(P.maps + j.tabOff)[j.half];
  P.out[k] = v == 0xFFFFu ? INT32_MAX : (int32_t)v;
}

}  // namespace mrp

extern "C" hipError_t mrp_ll_launch_heur_bfs(const mrp::HeurParams* P, uint32_t ldsBytes, hipStream_t stream) {
  hipLaunchKernelGGL(mrp::mrp_ll_heur_bfs_kernel, dim3(P->n), dim3(64), ldsBytes, stream, *P);
  return hipGetLastError();
}
extern "C" hipError_t mrp_ll_launch_heur_lookup(const mrp::LookupParams* P, hipStream_t stream) {
  hipLaunchKernelGGL(mrp::mrp_ll_heur_lookup_kernel, dim3((P->n + 255u) / 256u), dim3(256), 0, stream, *P);
  return hipGetLastError();
}
