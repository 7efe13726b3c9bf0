// mrp_hl_solve_cbs_ta_batch (include/mrp_hl.h): CBS with task assignment for a batch of instances, round-based.  The trees are
// hl/cbs_ta_tree.hpp's state machines (speculation width 1); a round makes three engine calls over ALL instances:
//   1. mrp_ll_assign_series_next  for the trees that need a root (one launch for all their series' children)
//   2. mrp_ll_ta_root_batch       for the new roots of at most 64 agents and mrp_ll_ta_root_batch_w for the others: at most
//                                 two root calls (use_root_kernel = 0, or a wide root with an engine that has no wide root
//                                 call: their n searches join call 3, the tree scans itself)
//   3. mrp_ll_search_batch        for the child searches
// and then lets every tree run up to its next request.  A translation unit of its own: csrc/hl/mrp_hl.cpp neither includes nor
// calls it, so the drivers there still link against engines that have no table, assignment or root calls.
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../include/mrp_hl.h"
#include "cbs_ta_tree.hpp"
#include "ta_batch_setup.hpp"

namespace {

using mrp_hl::ta::Conflict;
using mrp_hl::ta::Engine;
using mrp_hl::ta::kPathCap;
using mrp_hl::ta::Path;
using mrp_hl::ta::PathP;
using mrp_hl::ta::pathOf;
using mrp_hl::ta::ResultPool;
using mrp_hl::ta::Tree;

// What a search's status means to its tree: 0 a path, 1 no path (the reference's `success == false`), else the tree ends.
int verdict(Tree& t, const mrp_ll_result& r) {
  if (r.status == MRP_LL_OK && r.n_states >= 1 && r.n_states <= kPathCap) return 0;
  if (r.status == MRP_LL_NO_SOLUTION) return 1;
  t.end(r.status == MRP_LL_CAP_EXPANSIONS ? MRP_HL_CAP : MRP_HL_LL_ERROR);
  return 2;
}

void taskJob(mrp_ll_job& j, const Tree& t, int agent, int32_t task, const mrp_hl::ta::Cons* cons, int64_t budget) {
  std::memset(&j, 0, sizeof(j));
  j.map_id = t.mapId;
  j.algo = MRP_LL_ASTAR_TA;
  j.w = 1.0f;
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

}  // namespace

extern "C" int mrp_hl_solve_cbs_ta_batch(int32_t device, const mrp_hl_ta_options* optIn, int32_t n, const mrp_hl_ta_instance* inst,
                                         mrp_hl_ta_solution* sols, mrp_hl_batch_stats* stats) {
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
  rc = mrp_hl::ta::setUpBatch(eng, n, inst, trees);
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
    // 1. the next assignment of every tree that needs a root
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
        const std::vector<int32_t> taskOf = mrp_hl::ta::taskOfBuffers(ask.size(), res);
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
    // trees with a pending root — first those whose root goes through a root call, then those planned as ordinary jobs, so
    // that the jobs' results stand in one run with the children's — and trees with pending children
    std::vector<int32_t> rootOf, rootAsJobs, childOf;
    size_t nRootSearches = 0, nKernelSearches = 0;
    for (int32_t k : live) {
      Tree& t = *trees[k];
      if (!t.running()) continue;
      if (t.wantRoot) {
        const bool call = opt.use_root_kernel && (t.nAgents <= mrp_hl::ta::kNarrowLimit || &mrp_ll_ta_root_batch_w != nullptr);
        (call ? rootOf : rootAsJobs).push_back(k);
        nRootSearches += static_cast<size_t>(t.nAgents);
        if (call) nKernelSearches += static_cast<size_t>(t.nAgents);
      }
      if (t.wantChildren) childOf.push_back(k);
    }
    const size_t nKernelRoots = rootOf.size();
    rootOf.insert(rootOf.end(), rootAsJobs.begin(), rootAsJobs.end());
    const size_t nResults = nRootSearches + 2 * childOf.size();
    pool.reserve(nResults);
    std::vector<mrp_ll_result> res(nResults + 1);
    for (size_t q = 0; q < nResults; ++q) pool.attach(res[q], q);
    std::vector<size_t> rootFirst(rootOf.size());
    {
      size_t at = 0;
      for (size_t q = 0; q < rootOf.size(); ++q) {
        rootFirst[q] = at;
        at += static_cast<size_t>(trees[rootOf[q]]->nAgents);
      }
    }
    std::vector<int32_t> planned(rootOf.size() + 1, 0);
    std::vector<mrp_ll_conflict> rootConf(rootOf.size() + 1);
    std::vector<mrp_ll_job> jobs;
    std::vector<std::vector<int32_t>> rootGoals(rootOf.size()), rootHeur(rootOf.size());
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
        const int wide = t.nAgents > mrp_hl::ta::kNarrowLimit ? 1 : 0;
        roots[wide].push_back(r);
        rootIs[wide].push_back(q);
      }
      for (int wide = 0; wide < 2; ++wide) {
        if (roots[wide].empty()) continue;
        const int32_t m = static_cast<int32_t>(roots[wide].size());
        std::vector<int32_t> plannedOf(roots[wide].size(), 0);
        std::vector<mrp_ll_conflict> confOf(roots[wide].size());
        rc = wide ? mrp_ll_ta_root_batch_w(eng.ctx, m, roots[wide].data(), plannedOf.data(), confOf.data())
                  : mrp_ll_ta_root_batch(eng.ctx, m, roots[wide].data(), plannedOf.data(), confOf.data());
        if (rc != MRP_LL_SUCCESS) return rc;
        for (size_t i = 0; i < rootIs[wide].size(); ++i) {
          planned[rootIs[wide][i]] = plannedOf[i];
          rootConf[rootIs[wide][i]] = confOf[i];
        }
      }
    }
    for (size_t q = nKernelRoots; q < rootOf.size(); ++q) {
      const Tree& t = *trees[rootOf[q]];
      for (int a = 0; a < t.nAgents; ++a) {
        jobs.emplace_back();
        taskJob(jobs.back(), t, a, t.rootTasks[a], nullptr, budgetOf(t));
      }
    }
    // 3. the child searches (and, without the root kernel, the roots' searches in front of them)
    for (int32_t k : childOf) {
      const Tree& t = *trees[k];
      for (int c = 0; c < 2; ++c) {
        jobs.emplace_back();
        taskJob(jobs.back(), t, t.childAgent[c], t.nodes[t.popped].taskOf[t.childAgent[c]], t.childCons[c].get(), budgetOf(t));
      }
    }
    if (!jobs.empty()) {
      rc = mrp_ll_search_batch(eng.ctx, static_cast<int32_t>(jobs.size()), jobs.data(), res.data() + nKernelSearches);
      if (rc != MRP_LL_SUCCESS) return rc;
    }
    // the roots first: a new root is pushed BEFORE the two children (cbs_ta.hpp:165-168 in front of :179-210)
    for (size_t q = 0; q < rootOf.size(); ++q) {
      Tree& t = *trees[rootOf[q]];
      std::vector<PathP> paths(static_cast<size_t>(t.nAgents));
      const bool viaCall = q < nKernelRoots;
      int done = 0;
      bool all = true;
      for (int a = 0; a < t.nAgents && t.running(); ++a) {
        const mrp_ll_result& r = res[rootFirst[q] + a];
        if (viaCall && a >= planned[q]) break;
        done += 1;
        t.nSearches += 1;
        t.nRootSearches += 1;
        t.llExpanded += r.expanded;  // (the expansions of a failed root count)
        const int v = verdict(t, r);
        if (v == 0) paths[a] = pathOf(r);
        if (v != 0) {
          all = false;
          break;  // the root ends behind this agent (cbs_ta.hpp:159-162): later answers, if any, are not looked at
        }
      }
      if (!t.running()) continue;
      Conflict c;
      if (all && done == t.nAgents)
        c = viaCall ? mrp_hl::ta::conflictFromScan(rootConf[q], paths) : mrp_hl::ta::firstConflict(paths);
      t.gotRoot(paths, done, c);
    }
    for (size_t q = 0; q < childOf.size(); ++q) {
      Tree& t = *trees[childOf[q]];
      if (!t.running()) continue;
      PathP path[2];
      for (int c = 0; c < 2 && t.running(); ++c) {
        const mrp_ll_result& r = res[nRootSearches + 2 * q + c];
        t.nSearches += 1;
        t.llExpanded += r.expanded;
        if (verdict(t, r) == 0) path[c] = pathOf(r);
      }
      if (t.running()) t.gotChildren(path);
    }
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
