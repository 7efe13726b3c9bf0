// Min-cost task assignment on the device (mrp_ll_assign_batch, mrp_ll_assign_series_*): the wave program of
// assign_wave.h (up to 64 x 64) and of assign_wave_wide.h (up to 256 x 256, mrp_ll_assign_batch_w) with one wavefront
// (= one 64-thread workgroup) per problem.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_dev.h"
#include "assign_wave.h"
#include "assign_wave_wide.h"
#include "ll_launch.h"  // AssignParams, the launcher's prototype

namespace mrp {

// No static LDS: the dynamic window starts at LDS address 0 (wave_dev.h windowBase).  Its size is the largest
// as::ldsBytes of the launch's problems.
extern "C" __global__ void __launch_bounds__(64) mrp_ll_assign_kernel(AssignParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem != 0u) __builtin_trap();
  if (blockIdx.x >= P.n) return;
  const as::AssignJob job = P.jobs[blockIdx.x];
  as::assignSolve(wv::windowBase(nullptr), P.maps, P.data, P.out, job);
}

// The wide form: the window holds the problem's LDS rows (none with memory rows); the program is instantiated per
// C = AssignJobWide::words, so that its per-lane arrays are indexed by constants only.
extern "C" __global__ void __launch_bounds__(64) mrp_ll_assign_wide_kernel(AssignWideParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem != 0u) __builtin_trap();
  if (blockIdx.x >= P.n) return;
  const as::AssignJobWide job = P.jobs[blockIdx.x];
  as::assignSolveWideAny(wv::windowBase(nullptr), P.maps, P.data, P.out, job);
}

}  // namespace mrp

extern "C" hipError_t mrp_ll_launch_assign_wide(const mrp::AssignWideParams* P, uint32_t ldsBytes, hipStream_t stream) {
  hipLaunchKernelGGL(mrp::mrp_ll_assign_wide_kernel, dim3(P->n), dim3(64), ldsBytes, stream, *P);
  return hipGetLastError();
}

extern "C" hipError_t mrp_ll_launch_assign(const mrp::AssignParams* P, uint32_t ldsBytes, hipStream_t stream) {
  hipLaunchKernelGGL(mrp::mrp_ll_assign_kernel, dim3(P->n), dim3(64), ldsBytes, stream, *P);
  return hipGetLastError();
}
