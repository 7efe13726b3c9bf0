// TEST INFRASTRUCTURE — cbs_ta_tree_check.cpp for instances of up to 256 agents and 256 tasks: the same sequential algorithm,
// line for line, with the agents' masks in max(1, ceil(tasks / 64)) words (mrp_ll_assign_problem_w's layout) and the series
// of csrc/host/assign_series.h over the WIDE assignment wave program on the CPU (ta_series_emu_wide.h) — on an instance
// within 64 x 64 it returns field for field what cbs_ta_tree_check.cpp returns (tests/test_ta_wide_restatement_cpu.py).
// What follows is that file's description.
// A sequential restatement of CBS with task assignment, whole: CBSTA::search (cbs_ta.hpp:87-214) with
// the assignment bookkeeping of its Environment (example/cbs_ta.cpp:255-281 constructor, :442-456 nextTaskAssignment), over
// the oracle's low level and conflict scan (oracle/ta_restated.hpp: AStar over the cbs_ta.cpp Environment, getFirstConflict
// :369-420) and its restated d_ary_heap.  The two things the reference leaves to accident are fixed as the product documents
// them (include/mrp_hl.h, include/mrp_ll.h): tasks are the distinct potential goals in order of first appearance, and the
// next-best series is csrc/host/assign_series.h's (cost, then creation number), solved by the assignment wave program on the
// CPU (ta_series_emu.h).  One instance per call, one search after the other: what csrc/hl/mrp_hl_ta.cpp's rounds must equal.
// Holds no program text of the reference: every step names the lines it follows.
#include <cstdint>
#include <map>
#include <unordered_set>
#include <vector>

#include "search_restated.hpp"
#include "ta_restated.hpp"
#include "ta_series_emu_wide.h"

using namespace oracle;
using oracle::mapf::Cell;
using oracle::mapf::CellHash;
using oracle::mapf::Conflict;
using oracle::mapf::Constraints;
using oracle::mapf::Plan;
using oracle::mapf::State;

namespace {

struct Node {  // cbs_ta.hpp:217-235
  std::vector<Plan> solution;
  std::vector<Constraints> constraints;
  std::vector<int32_t> taskOf;  // `tasks`: -1 = no entry
  int cost = 0;
  int id = 0;
  bool isRoot = false;
};
struct Worse {
  bool operator()(const Node& a, const Node& b) const { return a.cost > b.cost; }  // operator<, :231-235
};

}  // namespace

// out: status (0 solved, 1 no solution, 2 cap), cost, makespan, highLevelExpanded, lowLevelExpanded, numTaskAssignments,
// roots pushed, popped root-flagged nodes with a conflict, schedule digest (FNV-1a as mrp_hl_solution), searches.
// taskXY [nAgents][2] (-1: none), endXYT [nAgents][3]: the last state of every path with the t the reference writes (cost so far).
extern "C" int cbs_ta_tree_wide_solve(int dimx, int dimy, int nObst, const int32_t* obstXY, int nAgents, const int32_t* startsXY,
                                 const int32_t* goalFirst, const int32_t* goalsXY, int64_t maxTaskAssignments, int64_t maxHl,
                                 int64_t* out, int32_t* taskXY, int32_t* endXYT) {
  std::unordered_set<Cell, CellHash> obst;
  for (int i = 0; i < nObst; ++i) obst.insert(Cell{obstXY[2 * i], obstXY[2 * i + 1]});
  std::vector<State> starts;
  for (int a = 0; a < nAgents; ++a) starts.push_back(State(0, startsXY[2 * a], startsXY[2 * a + 1]));
  // ---- Environment constructor (cbs_ta.cpp:271-280): the tasks, the cost of every (agent, own potential goal), the optimum
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
  auto nextTaskAssignment = [&](std::vector<int32_t>& taskOf) {  // cbs_ta.cpp:442-456; false: `tasks` stays empty
    taskOf.assign(nAgents, -1);
    if (numTaskAssignments > maxTaskAssignments) return false;
    mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
    if (mrp::host::assignSeriesNext(1, &series, &r, solve, solveWide) != MRP_LL_SUCCESS) return false;
    bool any = false;
    for (int a = 0; a < nAgents; ++a) any = any || taskOf[a] >= 0;
    if (any) ++numTaskAssignments;
    return any;
  };
  ta::Environment env(dimx, dimy, obst);
  auto search = [&](int a, const Constraints& c, int32_t task, Plan& plan) {
    ++searches;
    return ta::lowLevelSearch(env, a, c, task >= 0 ? &tasks[task] : nullptr, obst, dimx, dimy, starts[a], plan);
  };
  auto finish = [&](int status, const Node* sol) {
    delete series;
    for (int q = 0; q < 10; ++q) out[q] = 0;
    out[0] = status;
    out[3] = hlExpanded;
    out[4] = env.lowLevelExpanded();
    out[5] = numTaskAssignments;
    out[6] = rootsPushed;
    out[7] = rootConflicts;
    out[9] = searches;
    for (int a = 0; a < nAgents; ++a) {
      taskXY[2 * a] = taskXY[2 * a + 1] = -1;
      endXYT[3 * a] = endXYT[3 * a + 1] = endXYT[3 * a + 2] = -1;
    }
    if (!sol) return 0;
    uint64_t h = 14695981039346656037ull;
    auto byte = [&](uint32_t b) { h = (h ^ (b & 0xFFu)) * 1099511628211ull; };
    for (int a = 0; a < nAgents; ++a) {
      const Plan& p = sol->solution[a];
      out[1] += p.cost;                                    // cbs_ta.cpp:582-587
      out[2] = p.cost > out[2] ? p.cost : out[2];
      for (const auto& s : p.states) {
        byte(static_cast<uint32_t>(s.first.x));
        byte(static_cast<uint32_t>(s.first.y));
      }
      byte(0xFFu);
      endXYT[3 * a] = p.states.back().first.x;
      endXYT[3 * a + 1] = p.states.back().first.y;
      endXYT[3 * a + 2] = p.states.back().second;          // :606-610: `t` is the state's cost so far
      if (sol->taskOf[a] >= 0) {
        taskXY[2 * a] = tasks[sol->taskOf[a]].x;
        taskXY[2 * a + 1] = tasks[sol->taskOf[a]].y;
      }
    }
    out[8] = static_cast<int64_t>(h);
    return 0;
  };
  // ---- CBSTA::search
  Node start;                                              // cbs_ta.hpp:89-96
  start.solution.resize(nAgents);
  start.constraints.resize(nAgents);
  start.isRoot = true;
  const bool haveTasks = nextTaskAssignment(start.taskOf);
  for (int i = 0; i < nAgents; ++i) {                      // :98-116
    bool success = false;
    if (haveTasks) success = search(i, start.constraints[i], start.taskOf[i], start.solution[i]);
    if (!success) return finish(1, nullptr);
    start.cost += start.solution[i].cost;
  }
  ORACLE_HEAP<Node, Worse> open;
  open.push(start);                                        // :123
  ++rootsPushed;
  int id = 1;
  while (!open.empty()) {                                  // :128
    if (maxHl >= 0 && hlExpanded + 1 > maxHl) return finish(2, nullptr);
    Node P = open.top();
    ++hlExpanded;                                          // :130
    open.pop();
    Conflict conflict;
    if (!env.getFirstConflict(P.solution, conflict)) return finish(0, &P);  // :136-140
    if (P.isRoot) {                                        // :142-172 (a child is a copy of its parent, flag included: :185)
      ++rootConflicts;
      Node n;
      if (nextTaskAssignment(n.taskOf)) {
        n.solution.resize(nAgents);
        n.constraints.resize(nAgents);
        n.id = id;
        n.isRoot = true;
        bool all = true;
        for (int i = 0; i < nAgents; ++i) {
          if (!search(i, n.constraints[i], n.taskOf[i], n.solution[i])) {
            all = false;
            break;
          }
          n.cost += n.solution[i].cost;
        }
        if (all) {
          open.push(n);
          ++id;
          ++rootsPushed;
        }
      }
    }
    std::map<std::size_t, Constraints> cons;               // :179-210
    env.createConstraintsFromConflict(conflict, cons);
    for (const auto& c : cons) {
      const std::size_t i = c.first;
      Node child = P;
      child.id = id;
      child.constraints[i].add(c.second);
      child.cost -= child.solution[i].cost;
      const bool ok = search(static_cast<int>(i), child.constraints[i], child.taskOf[i], child.solution[i]);
      child.cost += child.solution[i].cost;
      if (ok) open.push(child);
      ++id;
    }
  }
  return finish(1, nullptr);
}
