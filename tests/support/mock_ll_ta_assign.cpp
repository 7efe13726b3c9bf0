// TEST INFRASTRUCTURE ONLY — the assignment half of mock_ll_ta.cpp: the engine's host-side next-best series
// (csrc/host/assign_series.h) with the assignment wave program on the CPU as its solver (ta_series_emu.h).
#include "ta_series_emu.h"

extern "C" int mock_ta_solve_batch(int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results) {
  return ta_emu::solveBatch(n, problems, results);
}
extern "C" int mock_ta_series_create(const void* owner, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_series** out) {
  return mrp::host::assignSeriesCreate(owner, n, problems, out, ta_emu::solver());
}
extern "C" int mock_ta_series_next(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results) {
  return mrp::host::assignSeriesNext(n, series, results, ta_emu::solver());
}
extern "C" void mock_ta_series_destroy(mrp_ll_assign_series* s) { delete s; }
