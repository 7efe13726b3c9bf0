// TEST INFRASTRUCTURE — the next-best assignment series of a CBS-TA instance on the CPU, for the restatement
// (cbs_ta_tree_check.cpp) and the stand-in engine (mock_ll_ta.cpp): the host-side series of csrc/host/assign_series.h, its
// constrained problems solved by the assignment wave program (csrc/assign_wave.h, the code the gfx950 kernel runs) on the
// host interpretation of its wave vocabulary, as tests/support/emu_assign.cpp does.  Problems are in the matrix form: a
// gather-form problem is turned into its cost rows first — cost(a, t) = table t at agent a's start (cbs_ta.cpp:272-279), no
// edge where the table says unreachable or the agent may not take the task (mrp_ll.h) — which is what the kernel gathers.
#pragma once
#include <stdint.h>

#include <climits>
#include <vector>

#include "wave_emu_assign.h"
#include "../../libmultirobotplanning_amd/csrc/assign_wave.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_pack.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_series.h"

namespace ta_emu {

inline int solveBatch(int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results) {
  static const mrp::host::PackEnv noEnv;
  static const std::vector<uint32_t> noMaps(1, 0);
  mrp::host::AssignStaging st;
  mrp::host::packAssignBatch(noEnv, n, problems, results, st);
  std::vector<uint32_t> out(st.outWords, 0xA5A5A5A5u);
  for (const mrp::as::AssignJob& job : st.jobs) {
    std::vector<uint8_t> mem(st.ldsBytes, 0xCD);
    wv::LdsWindow win{mem.data(), mrp::as::ldsBytes(job.nA), 0, 0};
    mrp::as::assignSolve(&win, noMaps.data(), st.data.data(), out.data(), job);
  }
  mrp::host::unpackAssignBatch(st, out.data(), results);
  return MRP_LL_SUCCESS;
}
inline mrp::host::AssignSolveFn solver() {
  return [](int32_t n, const mrp_ll_assign_problem* ps, mrp_ll_assign_result* rs) { return solveBatch(n, ps, rs); };
}

// dist(start of a, task t) -> the matrix entry
inline int32_t edge(int dist, bool allowed) { return (!allowed || dist == INT_MAX || dist > 0xFFFE) ? MRP_LL_ASSIGN_NO_EDGE : dist; }

}  // namespace ta_emu
