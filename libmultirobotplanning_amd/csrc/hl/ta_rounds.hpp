// The round loop of the two task-assignment solvers, mrp_hl_solve_cbs_ta_batch (csrc/hl/mrp_hl_ta.cpp) and
// mrp_hl_solve_ecbs_ta_batch (csrc/hl/mrp_hl_ecbs_ta.cpp).  The trees are resumable state machines over hl/ta_tree_base.hpp;
// a round makes at most four engine calls over ALL instances, in this order:
//   1. mrp_ll_assign_series_next  for the trees that ask for their next assignment
//   2. the algorithm's root call  for the new roots of at most 64 agents, one workgroup each, and its _w form for the others
//                                 (use_root_kernel = 0, or a wide root with an engine that has no wide root call: the root's
//                                 searches are jobs of call 3)
//   3. mrp_ll_search_batch        the roots planned as jobs in front of the two child searches of every expanded node
// then the trees take their answers, roots before children (a new root is pushed BEFORE the two children, cbs_ta.hpp:165-168
// in front of :179-210), and every live tree runs up to its next request.
// What differs between the algorithms is said by `Algo`, an object that lives for one call (no virtual dispatch):
//   typedef ... Tree;                              ta::Tree or ecbs_ta::Tree
//   static bool wideRootCall();                    the engine has the _w form of the root call
//   int setUp(Engine&, trees);                     after setUpBatch; anything but MRP_LL_SUCCESS ends the call
//   void beginRound(const mrp_ll_result* res, size_t nResults);
//   int rootCall(ctx, bool wide, m, roots, int32_t* planned, mrp_ll_conflict* scan);
//   size_t rootJobsOf(const Tree&);                the searches that a root planned as jobs issues in ONE round
//   void rootJobs(const Tree&, budget, first, jobs);   appends them; their results stand at `first` on
//   void childJobs(const Tree&, budget, first, jobs);  appends the two searches of the popped node's children
//   PathP path(const mrp_ll_result&, size_t q);    result q, a search that left a path, as the tree's path
//   void gotRoot(Tree&, bool viaCall, paths, const mrp_ll_result* r, int done, bool all, const mrp_ll_conflict& scan);
//                                                  the root's results r[0 .. done), read up to the first without a path
//                                                  (all: none), paths[k] of r[k]; `scan` is the root call's
//   void gotChildren(Tree&, const PathP path[2], const mrp_ll_result* r);
//   void endRound();
// This header names no entry point of one algorithm's: csrc/hl/mrp_hl_ta.cpp still links against an engine without ECBS-TA's.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../include/mrp_hl.h"
#include "ta_batch_setup.hpp"

namespace mrp_hl {
namespace ta {

// What a search's status means to its tree: 0 a path, 1 no path (the reference's `success == false`), else the tree ends.
inline int verdict(TreeBase& t, const mrp_ll_result& r) {
  if (r.status == MRP_LL_OK && r.n_states >= 1 && r.n_states <= kPathCap) return 0;
  if (r.status == MRP_LL_NO_SOLUTION) return 1;
  t.end(r.status == MRP_LL_CAP_EXPANSIONS ? MRP_HL_CAP : MRP_HL_LL_ERROR);
  return 2;
}

// One search of `agent` for `task` (-1: none, MRP_LL_JOB_NO_GOAL) under `cons` (null: none): everything but the algorithm's
// own fields.
inline void fillJob(mrp_ll_job& j, const TreeBase& t, int32_t algo, float w, int agent, int32_t task, const Cons* cons, int64_t budget) {
  std::memset(&j, 0, sizeof(j));
  j.map_id = t.mapId;
  j.algo = algo;
  j.w = w;
  j.start_x = t.starts[2 * agent];
  j.start_y = t.starts[2 * agent + 1];
  j.result_path_id = -1;
  j.max_expansions = budget;
  if (task >= 0) {
    j.goal_x = t.taskXY[2 * task];
    j.goal_y = t.taskXY[2 * task + 1];
    j.heuristic_id = t.taskHeur[task];
  } else {
    j.flags = MRP_LL_JOB_NO_GOAL;
    j.heuristic_id = -1;
  }
  if (cons) {
    j.n_vertex_constraints = static_cast<int32_t>(cons->vc.size() / 3);
    j.vertex_constraints = cons->vc.data();
    j.n_edge_constraints = static_cast<int32_t>(cons->ec.size() / 5);
    j.edge_constraints = cons->ec.data();
  }
}

template <class Algo>
int solveTaBatch(Algo& algo, int32_t device, const mrp_hl_ta_options* optIn, int32_t n, const mrp_hl_ta_instance* inst,
                 mrp_hl_ta_solution* sols, mrp_hl_batch_stats* stats) {
  typedef typename Algo::Tree Tree;
  if (n < 0 || (n > 0 && (!inst || !sols))) return MRP_LL_E_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return MRP_LL_SUCCESS;
  mrp_hl_ta_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.max_task_assignments = 1 << 30;
  opt.use_root_kernel = 0;  // (measured slower in the driver at the reference shape: DESIGN.md section 5)
  opt.max_hl_expansions = opt.max_ll_expansions = -1;
  if (optIn) opt = *optIn;

  Engine eng;
  mrp_ll_options lo;
  std::memset(&lo, 0, sizeof(lo));
  lo.device = device;
  lo.n_tickets = 1;
  int rc = mrp_ll_create(&lo, &eng.ctx);
  if (rc != MRP_LL_SUCCESS) return rc;

  // ---- the instances: maps, tasks, one launch for all tables, one for all optima
  std::vector<std::unique_ptr<Tree>> trees;
  rc = setUpBatch(eng, n, inst, trees);
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = algo.setUp(eng, trees);
  if (rc != MRP_LL_SUCCESS) return rc;

  // ---- the rounds
  const auto t0 = std::chrono::steady_clock::now();
  ResultPool pool;
  int64_t rounds = 0;
  for (;;) {
    std::vector<int32_t> live;
    for (int32_t k = 0; k < n; ++k)
      if (trees[k]->running()) live.push_back(k);
    if (live.empty()) break;
    rounds += 1;
    // 1. the next assignment of every tree that asks for one
    {
      std::vector<mrp_ll_assign_series*> ask;
      std::vector<int32_t> who;
      for (int32_t k : live) {
        Tree& t = *trees[k];
        if (!t.wantAssignment) continue;
        if (!t.assignmentAllowed(opt.max_task_assignments)) {
          t.gotAssignment(nullptr);
          continue;
        }
        ask.push_back(eng.series[k]);
        who.push_back(k);
      }
      if (!ask.empty()) {
        std::vector<mrp_ll_assign_result> res;
        const std::vector<int32_t> taskOf = taskOfBuffers(ask.size(), res);
        rc = mrp_ll_assign_series_next(eng.ctx, static_cast<int32_t>(ask.size()), ask.data(), res.data());
        if (rc != MRP_LL_SUCCESS) return rc;
        for (size_t q = 0; q < ask.size(); ++q)
          trees[who[q]]->gotAssignment(res[q].status == MRP_LL_OK && res[q].matched > 0 ? res[q].task_of : nullptr);
      }
    }
    // what every search of this round may spend
    auto budgetOf = [&](const Tree& t) -> int64_t {
      if (opt.max_ll_expansions < 0) return -1;
      return opt.max_ll_expansions > t.llExpanded ? opt.max_ll_expansions - t.llExpanded : 0;
    };
    // trees with a pending root — first those whose root goes through a root call, then those planned as jobs, so that the
    // jobs' results stand in one run with the children's — and trees with pending children
    std::vector<int32_t> rootOf, rootAsJobs, childOf;
    for (int32_t k : live) {
      const Tree& t = *trees[k];
      if (!t.running()) continue;
      if (t.wantRoot) {
        const bool call = opt.use_root_kernel && (t.nAgents <= kNarrowLimit || Algo::wideRootCall());
        (call ? rootOf : rootAsJobs).push_back(k);
      }
      if (t.wantChildren) childOf.push_back(k);
    }
    const size_t nKernelRoots = rootOf.size();
    rootOf.insert(rootOf.end(), rootAsJobs.begin(), rootAsJobs.end());
    // the results of the round: the roots' (n each through a root call, Algo's count as jobs), then two per pair of children
    std::vector<size_t> rootFirst(rootOf.size() + 1, 0);
    for (size_t q = 0; q < rootOf.size(); ++q) {
      const Tree& t = *trees[rootOf[q]];
      rootFirst[q + 1] = rootFirst[q] + (q < nKernelRoots ? static_cast<size_t>(t.nAgents) : algo.rootJobsOf(t));
    }
    const size_t firstJob = rootFirst[nKernelRoots], nRootResults = rootFirst[rootOf.size()];
    const size_t nResults = nRootResults + 2 * childOf.size();
    pool.reserve(nResults);
    std::vector<mrp_ll_result> res(nResults + 1);
    for (size_t q = 0; q < nResults; ++q) pool.attach(res[q], q);
    algo.beginRound(res.data(), nResults);
    std::vector<int32_t> planned(rootOf.size() + 1, 0);
    std::vector<mrp_ll_conflict> rootScan(rootOf.size() + 1);
    std::vector<std::vector<int32_t>> rootGoals(nKernelRoots), rootHeur(nKernelRoots);
    if (nKernelRoots > 0) {
      // 2. the new roots, one workgroup each: the narrow ones in one call, the wide ones in another
      std::vector<mrp_ll_ta_root> roots[2];
      std::vector<size_t> rootIs[2];
      for (size_t q = 0; q < nKernelRoots; ++q) {
        const Tree& t = *trees[rootOf[q]];
        rootGoals[q].assign(static_cast<size_t>(2 * t.nAgents), 0);
        rootHeur[q].assign(static_cast<size_t>(t.nAgents), -1);
        for (int a = 0; a < t.nAgents; ++a)
          if (t.rootTasks[a] >= 0) {
            rootGoals[q][2 * a] = t.taskXY[2 * t.rootTasks[a]];
            rootGoals[q][2 * a + 1] = t.taskXY[2 * t.rootTasks[a] + 1];
            rootHeur[q][a] = t.taskHeur[t.rootTasks[a]];
          }
        mrp_ll_ta_root r;
        std::memset(&r, 0, sizeof(r));
        r.map_id = t.mapId;
        r.n_agents = t.nAgents;
        r.starts_xy = t.starts.data();
        r.goals_xy = rootGoals[q].data();
        r.heuristic_ids = rootHeur[q].data();
        r.max_expansions = budgetOf(t);
        r.results = res.data() + rootFirst[q];
        const int wide = t.nAgents > kNarrowLimit ? 1 : 0;
        roots[wide].push_back(r);
        rootIs[wide].push_back(q);
      }
      for (int wide = 0; wide < 2; ++wide) {
        if (roots[wide].empty()) continue;
        std::vector<int32_t> plannedOf(roots[wide].size(), 0);
        std::vector<mrp_ll_conflict> scanOf(roots[wide].size());
        rc = algo.rootCall(eng.ctx, wide != 0, static_cast<int32_t>(roots[wide].size()), roots[wide].data(), plannedOf.data(),
                           scanOf.data());
        if (rc != MRP_LL_SUCCESS) return rc;
        for (size_t i = 0; i < rootIs[wide].size(); ++i) {
          planned[rootIs[wide][i]] = plannedOf[i];
          rootScan[rootIs[wide][i]] = scanOf[i];
        }
      }
    }
    // 3. the child searches, and in front of them the searches of the roots that go through no root call
    std::vector<mrp_ll_job> jobs;
    jobs.reserve(nResults - firstJob);
    for (size_t q = nKernelRoots; q < rootOf.size(); ++q) {
      const Tree& t = *trees[rootOf[q]];
      algo.rootJobs(t, budgetOf(t), rootFirst[q], jobs);
    }
    for (size_t q = 0; q < childOf.size(); ++q) {
      const Tree& t = *trees[childOf[q]];
      algo.childJobs(t, budgetOf(t), nRootResults + 2 * q, jobs);
    }
    if (!jobs.empty()) {
      rc = mrp_ll_search_batch(eng.ctx, static_cast<int32_t>(jobs.size()), jobs.data(), res.data() + firstJob);
      if (rc != MRP_LL_SUCCESS) return rc;
    }
    // a tree's share of one result; true: the search left a path
    auto took = [&](Tree& t, const mrp_ll_result& r, bool ofRoot) {
      t.nSearches += 1;
      t.nRootSearches += ofRoot ? 1 : 0;
      t.llExpanded += r.expanded;  // (the expansions of a failed search count)
      return verdict(t, r) == 0;
    };
    // the roots first; a root ends behind its first agent without a path (cbs_ta.hpp:159-162, ecbs_ta.hpp:323-326): later
    // answers, if any, are not looked at
    for (size_t q = 0; q < rootOf.size(); ++q) {
      Tree& t = *trees[rootOf[q]];
      const bool viaCall = q < nKernelRoots;
      const int nRead = viaCall ? std::min(planned[q], t.nAgents) : static_cast<int>(rootFirst[q + 1] - rootFirst[q]);
      std::vector<PathP> paths(static_cast<size_t>(t.nAgents));
      int done = 0;
      bool all = true;
      while (done < nRead && all && t.running()) {
        const size_t at = rootFirst[q] + static_cast<size_t>(done);
        if (took(t, res[at], true))
          paths[done] = algo.path(res[at], at);
        else
          all = false;
        done += 1;
      }
      if (t.running()) algo.gotRoot(t, viaCall, paths, res.data() + rootFirst[q], done, all, rootScan[q]);
    }
    for (size_t q = 0; q < childOf.size(); ++q) {
      Tree& t = *trees[childOf[q]];
      const size_t at = nRootResults + 2 * q;
      PathP path[2];
      for (int c = 0; c < 2 && t.running(); ++c)
        if (took(t, res[at + c], false)) path[c] = algo.path(res[at + c], at + c);
      if (t.running()) algo.gotChildren(t, path, res.data() + at);
    }
    algo.endRound();
    for (int32_t k : live) {
      Tree& t = *trees[k];
      if (t.running() && opt.max_ll_expansions >= 0 && t.llExpanded > opt.max_ll_expansions) t.end(MRP_HL_CAP);
      t.advance(opt.max_hl_expansions);
    }
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (int32_t k = 0; k < n; ++k) {
    trees[k]->write(sols[k]);
    if (stats) {
      stats->ll_searches += trees[k]->nSearches;
      stats->ll_expansions += trees[k]->llExpanded;
      stats->solved += trees[k]->status == MRP_HL_SOLVED ? 1 : 0;
      stats->root_solved += trees[k]->status == MRP_HL_SOLVED && trees[k]->hlExpanded == 1 ? 1 : 0;
    }
  }
  if (stats) {
    stats->wall_seconds = wall;
    stats->rounds = rounds;
  }
  return MRP_LL_SUCCESS;
}

}  // namespace ta
}  // namespace mrp_hl
