// TEST INFRASTRUCTURE — ta_series_emu.h for instances beyond 64 x 64: the wide series of csrc/host/assign_series.h
// (assignSeriesCreateWide), its constrained problems solved by the WIDE assignment wave program (csrc/assign_wave_wide.h,
// the code the gfx950 kernel runs) on the host interpretation of its wave vocabulary, as tests/support/emu_assign_wide.cpp
// does.  For the wide restatements (cbs_ta_tree_wide_check.cpp, ecbs_ta_tree_wide_check.cpp) and the wide stand-in engine
// (mock_ll_ta_wide.cpp).  Problems are in the matrix form.
#pragma once
#include "ta_series_emu.h"
#include "../../libmultirobotplanning_amd/csrc/assign_wave_wide.h"

namespace ta_emu {

inline int solveBatchWide(int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_result* results) {
  static const mrp::host::PackEnv noEnv;
  static const std::vector<uint32_t> noMaps(1, 0);
  const uint32_t budget = mrp::as::kLdsBudgetWide;
  mrp::host::AssignStagingWide st;
  mrp::host::packAssignBatchWide(noEnv, n, problems, results, budget, st);
  std::vector<uint32_t> out(st.outWords + st.scratchWords, 0xA5A5A5A5u);
  for (const mrp::as::AssignJobWide& job : st.jobs) {
    const uint32_t bytes = mrp::as::ldsBytesWide(job.nA, job.nT, budget);
    if (bytes > st.ldsBytes) return MRP_LL_E_INVALID;
    std::vector<uint8_t> mem(bytes, 0xCD);
    wv::LdsWindow win{mem.data(), bytes, 0, 0};
    mrp::as::assignSolveWideAny(&win, noMaps.data(), st.data.data(), out.data(), job);
  }
  mrp::host::unpackAssignBatchWide(st, out.data(), results);
  return MRP_LL_SUCCESS;
}
inline mrp::host::AssignSolveWideFn solverWide() {
  return [](int32_t n, const mrp_ll_assign_problem_w* ps, mrp_ll_assign_result* rs) { return solveBatchWide(n, ps, rs); };
}

// bit t of agent a's mask of `words` words (mrp_ll_assign_problem_w's layout)
inline bool maskBit(const uint64_t* masks, int words, int a, int t) { return (masks[static_cast<size_t>(a) * words + t / 64] >> (t % 64)) & 1; }

}  // namespace ta_emu
