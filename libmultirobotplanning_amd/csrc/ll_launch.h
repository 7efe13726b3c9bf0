// Everything the host side of the engine launches: the parameter records of the conflict-scan, heuristic and assignment
// kernels and the prototypes of every host-callable function the .hip files define.  Included by ll_kernel.hip,
// conflict_kernel.hip, heur_kernel.hip, assign_kernel.hip (which define them) and by mrp_ll_host.cpp (which calls them):
// one declaration, checked on both sides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrp_ll.h"
#include "assign_layout.h"
#include "heur_layout.h"
#include "ll_device.h"

namespace mrp {

struct ConflictOut {  // mirrors mrp_ll_conflict of include/mrp_ll.h (10 x int32)
  int32_t found, time, agent1, agent2, type, x1, y1, x2, y2, count;
};
static_assert(sizeof(mrp_ll_conflict) == sizeof(ConflictOut), "mrp_ll_conflict layout");

struct ConflictParams {
  const uint32_t* setFirstAgent;   // [nSets + 1]
  const uint32_t* pathFirstState;  // [totalAgents + 1]
  const uint16_t* states;          // [totalStates]  x | y << 8
  ConflictOut* out;                // [nSets]
  uint32_t nSets;
};

struct HeurParams {
  uint32_t* maps;           // the maps buffer: bitmaps are read, tables written
  const hb::HeurJob* jobs;  // [n]
  uint32_t n;
};
struct LookupParams {
  const uint32_t* maps;
  const hb::LookupJob* jobs;  // [n]
  int32_t* out;               // [n]: the entry, INT32_MAX where the table says 0xFFFF
  uint32_t n;
};
struct AssignParams {
  const uint32_t* maps;       // the maps buffer: the gather form reads the tasks' heuristic tables
  const as::AssignJob* jobs;  // [n]
  const uint32_t* data;       // the staged words the jobs' offsets count in
  uint32_t* out;              // the result records
  uint32_t n;
};
struct AssignWideParams {
  const uint32_t* maps;
  const as::AssignJobWide* jobs;  // [n]
  const uint32_t* data;
  uint32_t* out;                  // the result records, then the scratch regions of the gather problems with memory rows
  uint32_t n;
};

}  // namespace mrp

extern "C" {
// ll_kernel.hip.  kind: 0 = mixed, 1 = A*-epsilon jobs only, 2 = A* jobs only
uint32_t mrp_ll_lds_bytes(int kind, uint32_t capNodes, uint32_t rows, uint32_t rowWords, uint32_t pathBytes);
hipError_t mrp_ll_launch(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int kind, hipStream_t stream);
hipError_t mrp_ll_launch_persistent(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int kind, hipStream_t stream);
int mrp_ll_persistent_occupancy(int kind, uint32_t ldsBytes);
uint32_t mrp_ll_heavy_lds_bytes(void);
hipError_t mrp_ll_launch_front_heavy(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int heavy, hipStream_t stream);
int mrp_ll_front_heavy_occupancy(int heavy, uint32_t ldsBytes);
hipError_t mrp_ll_launch_ta_root(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int eps, int wide, hipStream_t stream);
hipError_t mrp_ll_launch_sipp(const mrp::LaunchParams* P, uint32_t grid, hipStream_t stream);
hipError_t mrp_ll_launch_sipp_persistent(const mrp::LaunchParams* P, uint32_t grid, hipStream_t stream);
int mrp_ll_sipp_persistent_occupancy(void);
// conflict_kernel.hip
hipError_t mrp_ll_launch_conflict(const mrp::ConflictParams* P, hipStream_t stream);
// heur_kernel.hip
hipError_t mrp_ll_launch_heur_bfs(const mrp::HeurParams* P, uint32_t ldsBytes, hipStream_t stream);
hipError_t mrp_ll_launch_heur_lookup(const mrp::LookupParams* P, hipStream_t stream);
// assign_kernel.hip
hipError_t mrp_ll_launch_assign(const mrp::AssignParams* P, uint32_t ldsBytes, hipStream_t stream);
hipError_t mrp_ll_launch_assign_wide(const mrp::AssignWideParams* P, uint32_t ldsBytes, hipStream_t stream);
}
