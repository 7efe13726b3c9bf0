// TEST INFRASTRUCTURE ONLY — mock_ll_ta_eps.cpp as it is, with one thing in front of it: the flags of every
// MRP_LL_ASTAR_EPS_TA job the driver sends through mrp_ll_search_batch are appended to the file MRP_SPY_TA_EPS_FLAGS names
// (one number per job).  The test links with -Wl,--wrap=mrp_ll_search_batch as test_ecbs_ta_driver_cpu.py does; the
// stand-in's own entry point gets another name here so that this file's can stand in front of it.
#define __wrap_mrp_ll_search_batch mock_ta_eps_search_batch
#include "mock_ll_ta_eps.cpp"
#undef __wrap_mrp_ll_search_batch

extern "C" int __wrap_mrp_ll_search_batch(mrp_ll_ctx* c, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res) {
  if (const char* file = std::getenv("MRP_SPY_TA_EPS_FLAGS"))
    if (FILE* f = std::fopen(file, "a")) {
      for (int i = 0; i < n; ++i)
        if (jobs[i].algo == MRP_LL_ASTAR_EPS_TA) std::fprintf(f, "%d\n", jobs[i].flags);
      std::fclose(f);
    }
  return mock_ta_eps_search_batch(c, n, jobs, res);
}
