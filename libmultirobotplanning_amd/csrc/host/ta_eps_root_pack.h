// The packer of mrp_ll_ta_eps_root_batch: ta_root_pack.h's with algo MRP_LL_ASTAR_EPS_TA and the weight in the root's
// record, and on the way back one more case: a root whose table outgrew the slot's path area before every agent was
// planned, which the host finishes (ll_ta_root_host.h).  Pure host logic: compiles with plain g++ -std=c++17
// (tests/support/ta_eps_root_pack_check.cpp).
#pragma once
#include "ta_root_pack.h"

namespace mrp {
namespace host {

// storeIds (mrp_ll_ta_eps_root_batch_stored): where each agent's path also goes in the path store; nullptr: nowhere.
static inline void packTaEpsRoots(const PackEnv& env, float w, int32_t n, const mrp_ll_ta_root* roots, uint32_t wordBase, TaRootStaging& st,
                                  const int32_t* const* storeIds = nullptr, uint32_t maxAgents = kTaRootMaxAgents) {
  packTaRootsAs(env, MRP_LL_ASTAR_EPS_TA, w, n, roots, wordBase, st, storeIds, maxAgents);
}

// After the launch: unpackTaRoots, plus needRest: the roots the kernel left in front of agent planned[k] < n_agents with
// every planned agent MRP_LL_OK (ll_ta_root.h, ECBS-TA: the table did not fit).  needScan: all agents planned, scan left to the host.
static inline void unpackTaEpsRoots(mrp_ll_stats& stats, const TaRootStaging& st, int32_t n, const mrp_ll_ta_root* roots,
                                    const DevResult* devResults, const uint16_t* outPaths, uint32_t outStride, int32_t* planned,
                                    mrp_ll_conflict* conflicts, std::vector<int32_t>& needScan, std::vector<int32_t>& needRest) {
  unpackTaRoots(stats, st, n, roots, devResults, outPaths, outStride, planned, conflicts, needScan);
  needRest.clear();
  if (!devResults) return;
  for (int32_t k = 0; k < n; ++k) {
    if (st.devRootOf[k] < 0 || planned[k] >= roots[k].n_agents) continue;
    if (taRootAnswer(outPaths, outStride, st.firstResult[k])[0] != kTaRootScanSkipped) continue;
    bool allOk = true;
    for (int a = 0; a < planned[k]; ++a) allOk = allOk && devResults[st.firstResult[k] + a].status == ST_OK;
    if (allOk) needRest.push_back(k);
  }
}

}  // namespace host
}  // namespace mrp
