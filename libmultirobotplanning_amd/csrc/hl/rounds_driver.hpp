// The round-based CBS / ECBS driver (mrp_hl_options.mode 1): every round a thread gathers the ready searches of its
// instances into one mrp_ll_search_batch.  Nothing stays resident on the device between rounds.
#pragma once
#include <memory>
#include <vector>

#include "ct_session.hpp"

namespace mrp_hl {

// Drives instances idx[...] (map ids mapBase + idx[...]) to completion on one engine, one mrp_ll_search_batch per round
// of ready searches.
// heurIds (mrp_hl_solve_batch_table_h; nullptr: the Manhattan searches): every search goes out with MRP_LL_JOB_TABLE_H and the
// table of its agent's goal on this engine, heurIds[agentFirst[instance] + agent].
inline void runGroup(mrp_ll_ctx* ctx, const mrp_hl_options& opt, const mrp_hl_instance* instIn, mrp_hl_solution* sols,
              const std::vector<int32_t>& idx, int32_t mapBase, int32_t horizon, GroupResult& out,
              const int32_t* heurIds = nullptr, const int64_t* agentFirst = nullptr) {
  const size_t n = idx.size();
  std::vector<std::unique_ptr<Instance>> inst(n);
  for (size_t k = 0; k < n; ++k) inst[k].reset(new Instance(instIn[idx[k]], mapBase + idx[k], opt));
  std::vector<std::vector<LLRequest>> req(n), nextReq(n);
  for (size_t k = 0; k < n; ++k) inst[k]->start(req[k]);

  JobBatch batch;
  std::vector<mrp_ll_job>& jobs = batch.jobs;
  std::vector<mrp_ll_result> results;
  std::vector<int32_t> statesPool;
  std::vector<LLAnswer> ans;
  int64_t ranExpansions = 0;

  for (;;) {
    auto tA = clockNow();
    batch.clear();
    for (size_t k = 0; k < n; ++k)
      for (const LLRequest& r : req[k]) {
        mrp_ll_job& j = batch.add(*inst[k], r);
        if (heurIds) {
          j.flags |= MRP_LL_JOB_TABLE_H;
          j.heuristic_id = heurIds[agentFirst[idx[k]] + r.agent];
        }
      }
    if (jobs.empty()) break;
    batch.patch();
    results.assign(jobs.size(), mrp_ll_result());
    bindResults(results.data(), jobs.size(), statesPool, horizon);
    auto tB = clockNow();
    int rc = mrp_ll_search_batch(ctx, static_cast<int32_t>(jobs.size()), jobs.data(), results.data());
    auto tC = clockNow();
    if (rc != MRP_LL_SUCCESS) {
      out.err = llError("mrp_ll_search_batch", ctx);
      return;
    }
    out.rounds += 1;
    out.searches += static_cast<int64_t>(jobs.size());
    // answers go back group by group (the requests of one group are consecutive), in request order
    size_t q = 0;
    for (size_t k = 0; k < n; ++k) {
      nextReq[k].clear();
      const std::vector<LLRequest>& rq = req[k];
      for (size_t a = 0; a < rq.size();) {
        size_t b = a;
        ans.clear();
        while (b < rq.size() && rq[b].group == rq[a].group) {
          ranExpansions += results[q].expanded;
          ans.push_back(answerOf(results[q]));
          ++q;
          ++b;
        }
        inst[k]->deliver(rq[a].group, ans, nextReq[k]);
        a = b;
      }
      if (inst[k]->done()) nextReq[k].clear();  // requests of a finished instance point into freed CT nodes
      req[k].swap(nextReq[k]);
    }
    auto tD = clockNow();
    out.buildS += secondsBetween(tA, tB);
    out.llS += secondsBetween(tB, tC);
    out.consumeS += secondsBetween(tC, tD);
  }
  for (size_t k = 0; k < n; ++k) {
    writeSolution(*inst[k], sols[idx[k]]);
    out.expansions += inst[k]->llExpanded();
    out.specSearches += inst[k]->specSearches();
  }
  out.specWasted += ranExpansions - out.expansions;
}

}  // namespace mrp_hl
