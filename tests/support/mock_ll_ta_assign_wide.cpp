// TEST INFRASTRUCTURE ONLY — the wide assignment half of mock_ll_ta_wide.cpp (a translation unit of its own, as
// mock_ll_ta_assign.cpp is): the engine's host-side wide series (csrc/host/assign_series.h) with the wide assignment wave
// program on the CPU as its solver, and one step over narrow and wide series together (ta_series_emu_wide.h).
#include "ta_series_emu_wide.h"

extern "C" int mock_ta_series_create_w(const void* owner, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_series** out) {
  return mrp::host::assignSeriesCreateWide(owner, n, problems, out, ta_emu::solverWide());
}
extern "C" int mock_ta_series_next_mixed(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results) {
  return mrp::host::assignSeriesNext(n, series, results, ta_emu::solver(), ta_emu::solverWide());
}
