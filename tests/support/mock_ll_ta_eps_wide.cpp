// TEST INFRASTRUCTURE ONLY — mock_ll_ta_eps.cpp plus the engine's wide entry points (mock_ll_ta_wide.cpp over it) and the wide
// ECBS-TA root call: mock_ll_ta_eps.cpp's mrp_ll_ta_eps_root_batch has no agent limit of its own, so
// mrp_ll_ta_eps_root_batch_w runs it.  Linked like mock_ll_ta_eps.cpp, with -Wl,--wrap=mrp_ll_search_batch.
// MRP_MOCK_TA_CALLS: the wide root call appends "ta_eps_root_batch_w" alone.
// -DMOCK_TA_WIDE_BASE='"mock_ll_ta_eps_store.cpp"': the same over the stand-in with a path store (MRP_HL_TA_DEVICE_PATHS).
#ifndef MOCK_TA_WIDE_BASE
#define MOCK_TA_WIDE_BASE "mock_ll_ta_eps.cpp"
#endif
#include "mock_ll_ta_wide.cpp"

#ifndef MOCK_NO_WIDE_ROOT
extern "C" int mrp_ll_ta_eps_root_batch_w(mrp_ll_ctx* c, float w, int32_t nRoots, const mrp_ll_ta_root* roots, mrp_ll_conflict* conflicts,
                                          int32_t* planned) {
  taCall("ta_eps_root_batch_w");
  for (int r = 0; r < nRoots; ++r)
    if (roots[r].n_agents <= 64) taCall("narrow_root_in_wide_call");
  return quietly([&] { return mrp_ll_ta_eps_root_batch(c, w, nRoots, roots, conflicts, planned); });
}
#endif
