// mrp_hl_solve_ecbs_ta_batch (include/mrp_hl.h): ECBS with task assignment for a batch of instances, round-based.  The trees
// are hl/ecbs_ta_tree.hpp's state machines; a round makes at most three engine calls over ALL instances:
//   1. mrp_ll_assign_series_next   for the trees whose new-root test (or start) asks for an assignment
//   2. mrp_ll_ta_eps_root_batch    for the new roots of at most 64 agents, one workgroup each, and mrp_ll_ta_eps_root_batch_w
//                                  for the others: at most two root calls (use_root_kernel = 0, or a wide root with an engine
//                                  that has no wide root call: a root is n dependent jobs of call 3, one agent per round, each
//                                  with the paths of the agents before it as its shipped focal context, and the tree scans
//                                  and counts itself)
//   3. mrp_ll_search_batch         MRP_LL_ASTAR_EPS_TA jobs: for every tree with an expanded node, its two child searches with
//                                  the node's paths as the context
// and then lets every tree run up to its next request.  The trees scan and count their children's conflicts themselves.
// MRP_HL_TA_DEVICE_PATHS=1 (ta_batch_setup.hpp TaKnobs; off by default, same results): the engine's path store is reserved,
// every search is told to leave its path in a slot of it (a root through mrp_ll_ta_eps_root_batch_stored), and a job whose
// node has every other agent's path there goes out with path_ids instead of a shipped table.  Instances of more than 64
// agents ignore the knob: their contexts ship, their searches store nothing and their roots go through the unstored call.
// MRP_HL_TA_EPS_LDS=1 (solve_knobs.hpp TaEpsKnobs; off by default, same results): the jobs of call 3 carry MRP_LL_JOB_TRY_LDS.
// A translation unit of its own, like csrc/hl/mrp_hl_ta.cpp.
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../include/mrp_hl.h"
#include "ecbs_ta_tree.hpp"
#include "solve_knobs.hpp"
#include "ta_batch_setup.hpp"

// The engine's entry point for roots that leave their paths in the store.  A weak reference: an engine library without it
// still loads, and MRP_HL_TA_DEVICE_PATHS then sends its roots through the plain call, their paths unstored.
extern "C" int mrp_ll_ta_eps_root_batch_stored(mrp_ll_ctx*, float, int32_t, const mrp_ll_ta_root*, mrp_ll_conflict*, int32_t*,
                                               const int32_t* const*) __attribute__((weak));

namespace {

using mrp_hl::ecbs_ta::Tree;
using mrp_hl::ta::Cons;
using mrp_hl::ta::Engine;
using mrp_hl::ta::kPathCap;
using mrp_hl::ta::PathP;
using mrp_hl::ta::pathOf;
using mrp_hl::ta::PathSlots;
using mrp_hl::ta::PathSlotsP;
using mrp_hl::ta::ResultPool;

// What a search's status means to its tree: 0 a path, 1 no path (the reference's `success == false`), else the tree ends.
int verdict(Tree& t, const mrp_ll_result& r) {
  if (r.status == MRP_LL_OK && r.n_states >= 1 && r.n_states <= kPathCap) return 0;
  if (r.status == MRP_LL_NO_SOLUTION) return 1;
  t.end(r.status == MRP_LL_CAP_EXPANSIONS ? MRP_HL_CAP : MRP_HL_LL_ERROR);
  return 2;
}

// The focal context of one job: the solution vector the search sees (its own entry is ignored, an empty path is skipped).
struct Context {
  std::vector<int32_t> len, ids;  // ids: the paths' slots in the path store, -1: not there (or no path)
  std::vector<const int32_t*> xy;
  void of(const std::vector<PathP>& sol) {
    static const int32_t none[2] = {0, 0};
    len.assign(sol.size(), 0);
    ids.assign(sol.size(), -1);
    xy.assign(sol.size(), none);
    for (size_t a = 0; a < sol.size(); ++a)
      if (sol[a]) {
        len[a] = sol[a]->len();
        ids[a] = sol[a]->slot;
        xy[a] = sol[a]->xy.data();
      }
  }
  // The context of `agent`'s search can go by slot: some other agent has a path, and each of those paths is in the store.
  // (Asked for trees of at most 64 agents only — the table the workgroup then builds fits: 64 agents x kPathCap 512 states
  // x 2 bytes = 64 KiB of the default engine's 128 KiB path area.  256 agents x 512 states do not, so wider trees ship.)
  bool byId(int agent) const {
    bool any = false;
    for (size_t a = 0; a < len.size(); ++a) {
      if (static_cast<int>(a) == agent || len[a] <= 0) continue;
      if (ids[a] < 0) return false;
      any = true;
    }
    return any;
  }
};

// slot >= 0: the search also leaves its path there; byId: the context goes by slot, nothing is shipped.
void epsJob(mrp_ll_job& j, const Tree& t, int agent, int32_t task, const Cons* cons, const Context& ctx, int64_t budget,
            int32_t slot = -1, bool byId = false) {
  std::memset(&j, 0, sizeof(j));
  j.map_id = t.mapId;
  j.algo = MRP_LL_ASTAR_EPS_TA;
  j.w = t.w;
  j.agent_idx = agent;
  j.start_x = t.starts[2 * agent];
  j.start_y = t.starts[2 * agent + 1];
  j.result_path_id = -1;
  j.max_expansions = budget;
  j.n_agents = static_cast<int32_t>(ctx.len.size());
  j.path_len = ctx.len.data();
  j.path_xy = ctx.xy.data();
  if (byId) {
    j.path_ids = ctx.ids.data();
    j.path_xy = nullptr;
  }
  if (slot >= 0) {
    j.result_path_id = slot;
    j.flags |= MRP_LL_JOB_STORE_RESULT;
  }
  if (task >= 0) {
    j.goal_x = t.taskXY[2 * task];
    j.goal_y = t.taskXY[2 * task + 1];
    j.heuristic_id = t.taskHeur[task];
  } else {
    j.flags |= MRP_LL_JOB_NO_GOAL;
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

extern "C" int mrp_hl_solve_ecbs_ta_batch(int32_t device, float w, const mrp_hl_ta_options* optIn, int32_t n,
                                          const mrp_hl_ta_instance* inst, mrp_hl_ta_solution* sols, mrp_hl_batch_stats* stats) {
  if (n < 0 || (n > 0 && (!inst || !sols)) || !(w >= 1.0f)) return MRP_LL_E_INVALID;
  mrp_hl_ta_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.max_task_assignments = 1 << 30;
  opt.max_hl_expansions = opt.max_ll_expansions = -1;
  opt.use_root_kernel = 0;  // (measured slower in the driver at the reference shape: DESIGN.md section 5)
  if (optIn) opt = *optIn;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return MRP_LL_SUCCESS;

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
  for (int32_t k = 0; k < n; ++k) trees[k]->w = w;
  // ---- MRP_HL_TA_DEVICE_PATHS: the store and its free list (null: the knob is off, and nothing below differs from before)
  const mrp_hl::ta::TaKnobs knobs = mrp_hl::ta::TaKnobs::read();
  const bool tryLds = mrp_hl::TaEpsKnobs::read().tryLds;  // MRP_HL_TA_EPS_LDS: the jobs below start in the LDS tier
  PathSlotsP slots;
  if (knobs.devicePaths) {
    int64_t agents = 0;
    for (int32_t k = 0; k < n; ++k) agents += trees[k]->running() && trees[k]->nAgents <= mrp_hl::ta::kNarrowLimit ? trees[k]->nAgents : 0;
    const int32_t nSlots = knobs.slotsFor(agents);
    rc = mrp_ll_path_store_reserve(eng.ctx, nSlots);
    if (rc != MRP_LL_SUCCESS) return rc;
    slots = std::make_shared<PathSlots>();
    slots->reset(nSlots);
  }

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
    // trees with a pending root — first those whose root goes through a root call, then those planned as jobs, so that the
    // jobs' results stand in one run with the children's — and trees with pending children
    std::vector<int32_t> rootOf, rootAsJobs, childOf;
    for (int32_t k : live) {
      const Tree& t = *trees[k];
      if (!t.running()) continue;
      if (t.wantRoot) {
        const bool call = opt.use_root_kernel && (t.nAgents <= mrp_hl::ta::kNarrowLimit || &mrp_ll_ta_eps_root_batch_w != nullptr);
        (call ? rootOf : rootAsJobs).push_back(k);
      }
      if (t.wantChildren) childOf.push_back(k);
    }
    const size_t nKernelRoots = rootOf.size();
    rootOf.insert(rootOf.end(), rootAsJobs.begin(), rootAsJobs.end());
    // the results of the round: the roots' (n each through a root call, one each as jobs), then two per pair of children
    std::vector<size_t> rootFirst(rootOf.size() + 1, 0);
    for (size_t q = 0; q < rootOf.size(); ++q)
      rootFirst[q + 1] = rootFirst[q] + (q < nKernelRoots ? static_cast<size_t>(trees[rootOf[q]]->nAgents) : 1u);
    const size_t nRootResults = rootFirst[rootOf.size()], nRootJobs = rootOf.size() - nKernelRoots;
    const size_t nResults = nRootResults + 2 * childOf.size(), nJobs = nRootJobs + 2 * childOf.size();
    pool.reserve(nResults);
    std::vector<mrp_ll_result> res(nResults + 1);
    for (size_t q = 0; q < nResults; ++q) pool.attach(res[q], q);
    // the slot result q's search was told to leave its path in (-1: none); whoever turns the result into a path takes it.
    // Only trees of at most 64 agents keep paths in the store (Context::byId).
    std::vector<int32_t> outSlot(nResults + 1, -1);
    auto stores = [&](const Tree& t) { return slots && t.nAgents <= mrp_hl::ta::kNarrowLimit; };
    auto takeSlot = [&](const Tree& t, size_t q) {
      if (stores(t)) outSlot[q] = slots->take();
      return outSlot[q];
    };
    auto pathFrom = [&](size_t q) {
      int32_t s = outSlot[q];
      outSlot[q] = -1;
      if (s >= 0 && res[q].n_states >= kPathCap) {  // as long as a slot: the device did not store it (mrp_ll.h)
        slots->give(s);
        s = -1;
      }
      return pathOf(res[q], s, slots);
    };
    std::vector<Context> ctx(rootOf.size() + childOf.size());
    std::vector<mrp_ll_job> jobs(nJobs);
    std::vector<int32_t> planned(rootOf.size() + 1, 0);
    std::vector<mrp_ll_conflict> rootScan(rootOf.size() + 1);
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
        std::vector<mrp_ll_conflict> scanOf(roots[wide].size());
        if (wide) {
          rc = mrp_ll_ta_eps_root_batch_w(eng.ctx, w, m, roots[wide].data(), scanOf.data(), plannedOf.data());
        } else if (slots && &mrp_ll_ta_eps_root_batch_stored != nullptr) {
          std::vector<std::vector<int32_t>> ids(roots[wide].size());
          std::vector<const int32_t*> idsOf(roots[wide].size());
          for (size_t i = 0; i < rootIs[wide].size(); ++i) {
            const size_t q = rootIs[wide][i];
            for (size_t a = 0; a < rootFirst[q + 1] - rootFirst[q]; ++a) ids[i].push_back(takeSlot(*trees[rootOf[q]], rootFirst[q] + a));
            idsOf[i] = ids[i].data();
          }
          rc = mrp_ll_ta_eps_root_batch_stored(eng.ctx, w, m, roots[wide].data(), scanOf.data(), plannedOf.data(), idsOf.data());
        } else {
          rc = mrp_ll_ta_eps_root_batch(eng.ctx, w, m, roots[wide].data(), scanOf.data(), plannedOf.data());
        }
        if (rc != MRP_LL_SUCCESS) return rc;
        for (size_t i = 0; i < rootIs[wide].size(); ++i) {
          planned[rootIs[wide][i]] = plannedOf[i];
          rootScan[rootIs[wide][i]] = scanOf[i];
        }
      }
    }
    for (size_t q = nKernelRoots; q < rootOf.size(); ++q) {
      const Tree& t = *trees[rootOf[q]];
      ctx[q].of(t.rootPaths);
      epsJob(jobs[q - nKernelRoots], t, t.rootAgent, t.rootTasks[t.rootAgent], nullptr, ctx[q], budgetOf(t), takeSlot(t, rootFirst[q]),
             stores(t) && ctx[q].byId(t.rootAgent));
    }
    // 3. the child searches (and, without the root call, the roots' next searches in front of them)
    for (size_t q = 0; q < childOf.size(); ++q) {
      const Tree& t = *trees[childOf[q]];
      Context& c = ctx[rootOf.size() + q];
      c.of(t.nodes[t.popped].sol);
      for (int s = 0; s < 2; ++s)
        epsJob(jobs[nRootJobs + 2 * q + s], t, t.childAgent[s], t.nodes[t.popped].taskOf[t.childAgent[s]], t.childCons[s].get(), c,
               budgetOf(t), takeSlot(t, nRootResults + 2 * q + s), stores(t) && c.byId(t.childAgent[s]));
    }
    if (tryLds)
      for (mrp_ll_job& j : jobs) j.flags |= MRP_LL_JOB_TRY_LDS;
    if (!jobs.empty()) {
      rc = mrp_ll_search_batch(eng.ctx, static_cast<int32_t>(jobs.size()), jobs.data(), res.data() + (nRootResults - nRootJobs));
      if (rc != MRP_LL_SUCCESS) return rc;
    }
    for (size_t q = 0; q < rootOf.size(); ++q) {
      Tree& t = *trees[rootOf[q]];
      if (q >= nKernelRoots) {
        const mrp_ll_result& r = res[rootFirst[q]];
        t.nSearches += 1;
        t.nRootSearches += 1;
        t.llExpanded += r.expanded;  // (the expansions of a failed root count)
        const int v = verdict(t, r);
        if (v != 2) t.gotRootSearch(v == 0 ? pathFrom(rootFirst[q]) : nullptr, r.fmin);
        continue;
      }
      std::vector<PathP> paths(static_cast<size_t>(t.nAgents));
      std::vector<int32_t> fmin(static_cast<size_t>(t.nAgents), 0);
      int done = 0;
      bool all = true;
      for (int a = 0; a < t.nAgents && a < planned[q] && all && t.running(); ++a) {
        const mrp_ll_result& r = res[rootFirst[q] + a];
        done += 1;
        t.nSearches += 1;
        t.nRootSearches += 1;
        t.llExpanded += r.expanded;
        const int v = verdict(t, r);
        if (v == 0) {
          paths[a] = pathFrom(rootFirst[q] + a);
          fmin[a] = r.fmin;
        } else {
          all = false;  // the root ends behind this agent (ecbs_ta.hpp:323-326)
        }
      }
      if (!t.running()) continue;
      if (all && done != t.nAgents)
        t.end(MRP_HL_LL_ERROR);  // (the call completes every root it accepts: a refused one)
      else
        t.gotRoot(paths, fmin, done, rootScan[q]);
    }
    for (size_t q = 0; q < childOf.size(); ++q) {
      Tree& t = *trees[childOf[q]];
      PathP path[2];
      int32_t fmin[2] = {0, 0};
      for (int s = 0; s < 2 && t.running(); ++s) {
        const mrp_ll_result& r = res[nRootResults + 2 * q + s];
        t.nSearches += 1;
        t.llExpanded += r.expanded;
        if (verdict(t, r) == 0) {
          path[s] = pathFrom(nRootResults + 2 * q + s);
          fmin[s] = r.fmin;
        }
      }
      if (t.running()) t.gotChildren(path, fmin);
    }
    for (int32_t s : outSlot)  // a search that left no path, or whose tree had ended: its slot is free again
      if (s >= 0) slots->give(s);
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
