// mrp_hl_solve_cbs_ta_batch (include/mrp_hl.h): CBS with task assignment for a batch of instances, in the rounds of
// hl/ta_rounds.hpp over hl/cbs_ta_tree.hpp's state machines (speculation width 1).  What is CBS-TA's own in a round:
//   the root call      mrp_ll_ta_root_batch for the new roots of at most 64 agents, mrp_ll_ta_root_batch_w for the others; the
//                      tree takes the call's conflict scan
//   a root as jobs     its n independent MRP_LL_ASTAR_TA searches in ONE round, and the tree scans itself
//   the children       two MRP_LL_ASTAR_TA searches
// A translation unit of its own: csrc/hl/mrp_hl.cpp neither includes nor calls it, so the drivers there still link against
// engines that have no table, assignment or root calls.
#include "../../../include/mrp_hl.h"
#include "cbs_ta_tree.hpp"
#include "ta_rounds.hpp"

namespace {

using mrp_hl::ta::Conflict;
using mrp_hl::ta::Engine;
using mrp_hl::ta::fillJob;
using mrp_hl::ta::PathP;

struct CbsTa {
  typedef mrp_hl::ta::Tree Tree;
  static bool wideRootCall() { return &mrp_ll_ta_root_batch_w != nullptr; }
  int setUp(Engine&, const std::vector<std::unique_ptr<Tree>>&) { return MRP_LL_SUCCESS; }
  void beginRound(const mrp_ll_result*, size_t) {}
  void endRound() {}
  int rootCall(mrp_ll_ctx* ctx, bool wide, int32_t m, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* scan) {
    return wide ? mrp_ll_ta_root_batch_w(ctx, m, roots, planned, scan) : mrp_ll_ta_root_batch(ctx, m, roots, planned, scan);
  }
  size_t rootJobsOf(const Tree& t) { return static_cast<size_t>(t.nAgents); }
  void rootJobs(const Tree& t, int64_t budget, size_t, std::vector<mrp_ll_job>& jobs) {
    for (int a = 0; a < t.nAgents; ++a) {
      jobs.emplace_back();
      fillJob(jobs.back(), t, MRP_LL_ASTAR_TA, 1.0f, a, t.rootTasks[a], nullptr, budget);
    }
  }
  void childJobs(const Tree& t, int64_t budget, size_t, std::vector<mrp_ll_job>& jobs) {
    for (int c = 0; c < 2; ++c) {
      jobs.emplace_back();
      fillJob(jobs.back(), t, MRP_LL_ASTAR_TA, 1.0f, t.childAgent[c], t.nodes[t.popped].taskOf[t.childAgent[c]], t.childCons[c].get(), budget);
    }
  }
  PathP path(const mrp_ll_result& r, size_t) { return mrp_hl::ta::pathOf(r); }
  // (a call that planned fewer than n searches without a failed one: the tree sees a root that is not whole)
  void gotRoot(Tree& t, bool viaCall, const std::vector<PathP>& paths, const mrp_ll_result*, int done, bool all, const mrp_ll_conflict& scan) {
    Conflict c;
    if (all && done == t.nAgents) c = viaCall ? mrp_hl::ta::conflictFromScan(scan, paths) : mrp_hl::ta::firstConflict(paths);
    t.gotRoot(paths, done, c);
  }
  void gotChildren(Tree& t, const PathP path[2], const mrp_ll_result*) { t.gotChildren(path); }
};

}  // namespace

extern "C" int mrp_hl_solve_cbs_ta_batch(int32_t device, const mrp_hl_ta_options* opt, int32_t n, const mrp_hl_ta_instance* inst,
                                         mrp_hl_ta_solution* sols, mrp_hl_batch_stats* stats) {
  CbsTa algo;
  return mrp_hl::ta::solveTaBatch(algo, device, opt, n, inst, sols, stats);
}
