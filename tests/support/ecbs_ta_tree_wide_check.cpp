// TEST INFRASTRUCTURE — ecbs_ta_tree_check.cpp for instances of up to 256 agents and 256 tasks: the same sequential algorithm,
// line for line, with the agents' masks in max(1, ceil(tasks / 64)) words (mrp_ll_assign_problem_w's layout) and the series
// of csrc/host/assign_series.h over the WIDE assignment wave program on the CPU (ta_series_emu_wide.h) — on an instance
// within 64 x 64 it returns field for field what ecbs_ta_tree_check.cpp returns (tests/test_ta_wide_restatement_cpu.py).
// What follows is that file's description.
// A sequential restatement of ECBS with task assignment, whole: ECBSTA::search (ecbs_ta.hpp:94-352, as
// example/ecbs_ta.cpp compiles it: REBUILT_FOCAL_LIST and STYLE_MINROOT, Cost = int) with the assignment bookkeeping of its
// Environment (example/ecbs_ta.cpp:254-281 constructor, :513-527 nextTaskAssignment), over the checker's low level
// (ecbs_ta_check.cpp: AStarEpsilon over the task-assignment Environment, included here as it stands), the oracle's conflict
// scan and count and its restated d_ary_heap.  Tasks and the next-best series are the product's, as in cbs_ta_tree_check.cpp.
// The three spots the reference leaves undefined are defined as include/mrp_hl.h documents them:
//   :302  open.top() on an empty open list     counts as "ask for a new root"
//   :344  open.top() on a still empty list     the loop ends, no solution
//   :238  focal.top() on an empty focal list   the instance ends with status 3 (MRP_HL_LL_ERROR)
// One instance per call, one search after the other: what csrc/hl/mrp_hl_ecbs_ta.cpp's rounds must equal.
// Holds no program text of the reference: every step names the lines it follows.
#include "ecbs_ta_check.cpp"
#include "ta_series_emu_wide.h"

namespace {

struct TreeNode {  // ecbs_ta.hpp:372-391
  std::vector<Plan> solution;
  std::vector<Constraints> constraints;
  std::vector<int32_t> taskOf;  // `tasks`: -1 = no entry
  int cost = 0, LB = 0, focalHeuristic = 0, id = 0;
  bool isRoot = false;
};
struct TreeWorse {
  bool operator()(const TreeNode& a, const TreeNode& b) const { return a.cost > b.cost; }  // operator<, :387-391
};
typedef ORACLE_HEAP<TreeNode, TreeWorse> TreeOpen;
struct TreeFocalWorse {  // :420-428
  const TreeOpen* open;
  bool operator()(const TreeOpen::handle_type& h1, const TreeOpen::handle_type& h2) const {
    const TreeNode& a = (*open)[h1];
    const TreeNode& b = (*open)[h2];
    if (a.focalHeuristic != b.focalHeuristic) return a.focalHeuristic > b.focalHeuristic;
    return a.cost > b.cost;
  }
};

}  // namespace

// out[0..9] as cbs_ta_tree_solve: status (0 solved, 1 no solution, 2 cap, 3 empty focal list), cost, makespan,
// highLevelExpanded, lowLevelExpanded, numTaskAssignments, roots pushed, popped root-flagged nodes with a conflict, schedule
// digest, searches.  out[10..14] say what the run reached: expanded nodes that had a conflict, roots that failed behind at least
// one planned agent, child searches that failed, 1 if the FIRST assignment was empty, new-root attempts (:302 taken).
// taskXY [nAgents][2] (-1: none), endXYT [nAgents][3]: the last state of every path with the t the reference writes;
// pathLen [nAgents] and pathsXY [nAgents][pathCap][2] (may be NULL): the returned paths, for a check from outside.
extern "C" int ecbs_ta_tree_wide_solve(int dimx, int dimy, int nObst, const int32_t* obstXY, int nAgents, const int32_t* startsXY,
                                  const int32_t* goalFirst, const int32_t* goalsXY, float w, int64_t maxTaskAssignments,
                                  int64_t maxHl, int64_t* out, int32_t* taskXY, int32_t* endXYT, int32_t* pathLen, int32_t* pathsXY,
                                  int pathCap) {
  const auto obst = obstacleSet(nObst, obstXY);
  std::vector<State> starts;
  for (int a = 0; a < nAgents; ++a) starts.push_back(State(0, startsXY[2 * a], startsXY[2 * a + 1]));
  // ---- Environment constructor (ecbs_ta.cpp:271-280): the tasks, the cost of every (agent, own potential goal), the optimum
  std::vector<Cell> tasks;
  std::vector<std::vector<int>> tasksOf(nAgents);
  for (int a = 0; a < nAgents; ++a)
    for (int q = goalFirst[a]; q < goalFirst[a + 1]; ++q) {
      const Cell g{goalsXY[2 * q], goalsXY[2 * q + 1]};
      if (g.x < 0 || g.x >= dimx || g.y < 0 || g.y >= dimy) continue;
      size_t t = 0;
      while (t < tasks.size() && !(tasks[t].x == g.x && tasks[t].y == g.y)) ++t;
      if (t == tasks.size()) tasks.push_back(g);
      tasksOf[a].push_back(static_cast<int>(t));
    }
  const int nT = static_cast<int>(tasks.size());
  if (nAgents > 256 || nT > 256) return -1;
  const int maskWords = nT > 64 ? (nT + 63) / 64 : 1;
  std::vector<uint64_t> allowed(static_cast<size_t>(nAgents) * maskWords, 0);
  for (int a = 0; a < nAgents; ++a)
    for (int t : tasksOf[a]) allowed[static_cast<size_t>(a) * maskWords + t / 64] |= 1ull << (t % 64);
  std::vector<int32_t> cost(static_cast<size_t>(nAgents) * nT + 1, 0);
  for (int t = 0; t < nT; ++t) {
    const std::vector<int> table = ta::shortestPathTable(dimx, dimy, obst, tasks[t]);
    for (int a = 0; a < nAgents; ++a)
      cost[static_cast<size_t>(a) * nT + t] = ta_emu::edge(table[starts[a].x + dimx * starts[a].y], ta_emu::maskBit(allowed.data(), maskWords, a, t));
  }
  mrp_ll_assign_problem_w prob{nAgents, nT, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, maskWords};
  mrp_ll_assign_series* series = nullptr;
  const mrp::host::AssignSolveFn solve = ta_emu::solver();
  const mrp::host::AssignSolveWideFn solveWide = ta_emu::solverWide();
  if (mrp::host::assignSeriesCreateWide(nullptr, 1, &prob, &series, solveWide) != MRP_LL_SUCCESS) return -1;
  int64_t numTaskAssignments = 0, hlExpanded = 0, searches = 0, rootsPushed = 0, rootConflicts = 0;
  int64_t conflictNodes = 0, rootsFailedPartWay = 0, childFailures = 0, firstEmpty = 0, rootAttempts = 0;
  auto nextTaskAssignment = [&](std::vector<int32_t>& taskOf) {  // ecbs_ta.cpp:513-527; false: `tasks` stays empty
    taskOf.assign(nAgents, -1);
    if (numTaskAssignments > maxTaskAssignments) return false;
    mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
    if (mrp::host::assignSeriesNext(1, &series, &r, solve, solveWide) != MRP_LL_SUCCESS || r.status != MRP_LL_OK || r.matched <= 0) {
      taskOf.assign(nAgents, -1);
      return false;
    }
    bool any = false;
    for (int a = 0; a < nAgents; ++a) any = any || taskOf[a] >= 0;
    if (any) ++numTaskAssignments;
    return any;
  };
  ta::Environment env(dimx, dimy, obst);
  const mapf::Environment counting(dimx, dimy, {}, {});  // focalHeuristic ecbs_ta.cpp:347-382 == ecbs.cpp:315-350
  auto search = [&](int a, const Constraints& c, int32_t task, const std::vector<Plan>& context, Plan& plan) {
    ++searches;
    Counters cnt;
    return lowLevel(env, dimx, dimy, obst, static_cast<std::size_t>(a), c, task >= 0 ? &tasks[task] : nullptr, context, w, starts[a],
                    plan, -1, cnt);
  };
  auto finish = [&](int status, const TreeNode* sol) {
    delete series;
    for (int q = 0; q < 15; ++q) out[q] = 0;
    out[0] = status;
    out[3] = hlExpanded;
    out[4] = env.lowLevelExpanded();
    out[5] = numTaskAssignments;
    out[6] = rootsPushed;
    out[7] = rootConflicts;
    out[9] = searches;
    out[10] = conflictNodes;
    out[11] = rootsFailedPartWay;
    out[12] = childFailures;
    out[13] = firstEmpty;
    out[14] = rootAttempts;
    for (int a = 0; a < nAgents; ++a) {
      taskXY[2 * a] = taskXY[2 * a + 1] = -1;
      endXYT[3 * a] = endXYT[3 * a + 1] = endXYT[3 * a + 2] = -1;
      if (pathLen) pathLen[a] = 0;
    }
    if (!sol) return 0;
    uint64_t h = 14695981039346656037ull;
    auto byte = [&](uint32_t b) { h = (h ^ (b & 0xFFu)) * 1099511628211ull; };
    for (int a = 0; a < nAgents; ++a) {
      const Plan& p = sol->solution[a];
      out[1] += p.cost;                                    // ecbs_ta.cpp main: statistics.cost, makespan
      out[2] = p.cost > out[2] ? p.cost : out[2];
      int k = 0;
      for (const auto& s : p.states) {
        byte(static_cast<uint32_t>(s.first.x));
        byte(static_cast<uint32_t>(s.first.y));
        if (pathsXY && k < pathCap) {
          pathsXY[(static_cast<size_t>(a) * pathCap + k) * 2] = s.first.x;
          pathsXY[(static_cast<size_t>(a) * pathCap + k) * 2 + 1] = s.first.y;
        }
        ++k;
      }
      if (pathLen) pathLen[a] = k;
      byte(0xFFu);
      endXYT[3 * a] = p.states.back().first.x;
      endXYT[3 * a + 1] = p.states.back().first.y;
      endXYT[3 * a + 2] = p.states.back().second;          // `t` is the state's cost so far
      if (sol->taskOf[a] >= 0) {
        taskXY[2 * a] = tasks[sol->taskOf[a]].x;
        taskXY[2 * a + 1] = tasks[sol->taskOf[a]].y;
      }
    }
    out[8] = static_cast<int64_t>(h);
    return 0;
  };
  // a root, :117-138 and :306-343: every agent against the paths of the agents before it; false: the search of agent
  // `failedAt` found no path
  auto planRoot = [&](TreeNode& n, int& failedAt) {
    n.solution.assign(nAgents, Plan());
    n.constraints.assign(nAgents, Constraints());
    n.cost = n.LB = 0;
    n.isRoot = true;
    for (int i = 0; i < nAgents; ++i) {
      if (!search(i, n.constraints[i], n.taskOf[i], n.solution, n.solution[i])) {
        failedAt = i;
        return false;
      }
      n.cost += n.solution[i].cost;
      n.LB += n.solution[i].fmin;
    }
    n.focalHeuristic = counting.focalHeuristic(n.solution);
    return true;
  };
  // ---- ECBSTA::search
  TreeNode start;                                          // ecbs_ta.hpp:96-104
  start.id = 0;
  if (!nextTaskAssignment(start.taskOf)) firstEmpty = 1;   // (an empty first assignment is planned all the same: no :105-113 here)
  int failedAt = 0;
  if (!planRoot(start, failedAt)) {                        // :129-131
    if (failedAt > 0) ++rootsFailedPartWay;
    return finish(1, nullptr);
  }
  int nextRootNodeCost = static_cast<int>(static_cast<float>(start.LB) * w);  // :142, binary32 product, truncated
  TreeOpen open;
  open.push(start);                                        // :149
  ++rootsPushed;
  int id = 1;
  while (!open.empty()) {                                  // :157
    if (maxHl >= 0 && hlExpanded + 1 > maxHl) return finish(2, nullptr);
    ORACLE_HEAP<TreeOpen::handle_type, TreeFocalWorse> focal(TreeFocalWorse{&open});  // :160 clear()
    open.orderedWalk([&](TreeOpen::handle_type h) {        // :163-179
      const float val = static_cast<float>(open[h].cost);
      if (!(val <= static_cast<float>(nextRootNodeCost))) return false;
      focal.push(h);
      return true;
    });
    if (focal.empty()) return finish(3, nullptr);          // :238 undefined in the reference
    const TreeOpen::handle_type h = focal.top();
    TreeNode P = open[h];
    ++hlExpanded;                                          // :240
    focal.pop();
    open.erase(h);                                         // :243-244
    Conflict conflict;
    if (!env.getFirstConflict(P.solution, conflict)) return finish(0, &P);  // :246-251
    ++conflictNodes;
    if (P.isRoot) ++rootConflicts;
    std::map<std::size_t, Constraints> cons;               // :258-297
    env.createConstraintsFromConflict(conflict, cons);
    for (const auto& c : cons) {
      const std::size_t i = c.first;
      TreeNode child = P;
      child.id = id;
      child.constraints[i].add(c.second);
      child.cost -= child.solution[i].cost;
      child.LB -= child.solution[i].fmin;
      const bool ok = search(static_cast<int>(i), child.constraints[i], child.taskOf[i], child.solution, child.solution[i]);
      if (ok) {
        child.cost += child.solution[i].cost;
        child.LB += child.solution[i].fmin;
        child.focalHeuristic = counting.focalHeuristic(child.solution);
        open.push(child);
      } else {
        ++childFailures;
      }
      ++id;
    }
    if (open.empty() || open.top().cost > nextRootNodeCost) {  // :302 (empty: defined as "ask")
      ++rootAttempts;
      TreeNode n;
      if (nextTaskAssignment(n.taskOf)) {                  // :307-309
        n.id = id;
        if (planRoot(n, failedAt)) {                       // :317-343
          open.push(n);
          ++id;
          ++rootsPushed;
        } else if (failedAt > 0) {
          ++rootsFailedPartWay;
        }
      }
      if (open.empty()) return finish(1, nullptr);         // :344 undefined in the reference
      nextRootNodeCost = static_cast<int>(static_cast<float>(open.top().LB) * w);  // :344-345
    }
  }
  return finish(1, nullptr);
}
