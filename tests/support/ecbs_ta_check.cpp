// TEST INFRASTRUCTURE ONLY: the CPU checker of MRP_LL_ASTAR_EPS_TA, assembled from the oracle's headers (build:
// g++ -std=c++17 -O2 -I oracle, tests/ecbs_ta_checker.py).
//
// The low level of ECBS with task assignment is AStarEpsilon (a_star_epsilon.hpp:86-285, restated in
// oracle/search_restated.hpp) over the task-assignment Environment (example/ecbs_ta.cpp:283-445).  That Environment's
// low-level side equals example/cbs_ta.cpp's (restated in oracle/ta_restated.hpp: setLowLevelContext, admissibleHeuristic,
// isSolution, getNeighbors) plus the two focal heuristics, which are example/ecbs.cpp's taken at the states' TIMES:
//   focalStateHeuristic       ecbs_ta.cpp:314-327
//   focalTransitionHeuristic  ecbs_ta.cpp:330-344
//   getState                  paths are clamped to their last state; empty paths and the agent itself are skipped
// LowLevelEnvironment (ecbs_ta.hpp:441-493) is the adapter below, with the harness's expansion cap and three counters the
// tests need: decrease-key events (a_star_epsilon.hpp:254-269 taken), nodes created, largest time discovered.
// The conflict tree is ecbs_ta.hpp:94-297 for ONE fixed assignment: the root searches run against the partial solution,
// cost / LB / focalHeuristic, open + focal, children; the assignment solvers (nextTaskAssignment, the new-root branch
// :299-348) stay out.
#include <cstdint>
#include <map>
#include <unordered_set>
#include <vector>

#include "search_restated.hpp"
#include "ta_restated.hpp"

namespace {

using namespace oracle;
using mapf::Action;
using mapf::Cell;
using mapf::CellHash;
using mapf::Conflict;
using mapf::Constraints;
using mapf::EdgeConstraint;
using mapf::Plan;
using mapf::State;
using mapf::StateHash;
using mapf::VertexConstraint;

State stateAt(std::size_t i, const std::vector<Plan>& sol, int t) {  // getState
  if (static_cast<std::size_t>(t) < sol[i].states.size()) return sol[i].states[t].first;
  return sol[i].states.back().first;
}

struct LLEnv {  // ecbs_ta.hpp:441-493
  ta::Environment& env;
  std::size_t agent;
  const std::vector<Plan>& sol;
  long cap;  // < 0: unlimited
  long decreaseKeys = 0, nodes = 1;
  int maxTime = 0;
  std::unordered_set<State, StateHash> seen;

  int admissibleHeuristic(const State& s) { return env.admissibleHeuristic(s); }
  int focalStateHeuristic(const State& s, int) {  // ecbs_ta.cpp:314-327
    int n = 0;
    for (std::size_t i = 0; i < sol.size(); ++i)
      if (i != agent && !sol[i].states.empty() && s.sameCell(stateAt(i, sol, s.time))) ++n;
    return n;
  }
  int focalTransitionHeuristic(const State& a, const State& b, int, int) {  // ecbs_ta.cpp:330-344
    int n = 0;
    for (std::size_t i = 0; i < sol.size(); ++i)
      if (i != agent && !sol[i].states.empty()) {
        const State oa = stateAt(i, sol, a.time), ob = stateAt(i, sol, b.time);
        if (a.sameCell(ob) && b.sameCell(oa)) ++n;
      }
    return n;
  }
  bool isSolution(const State& s) { return env.isSolution(s); }
  void getNeighbors(const State& s, std::vector<Neighbor<State, Action, int>>& n) { env.getNeighbors(s, n); }
  void onExpandNode(const State& s, int f, int g) {
    env.onExpandLowLevelNode(s, f, g);
    if (cap >= 0 && env.m_llExpandedThisSearch > cap) throw mapf::CapExceeded();
  }
  void onDiscover(const State& s, int, int) {  // a second discovery of a state is the decrease-key branch
    if (seen.insert(s).second)
      ++nodes;
    else
      ++decreaseKeys;
    if (s.time > maxTime) maxTime = s.time;
  }
};

struct Counters {
  long expanded = 0, decreaseKeys = 0, nodes = 0;
  int maxTime = 0;
};

// One low-level search (ecbs_ta.hpp:125-128, :276-279).  Throws mapf::CapExceeded.
bool lowLevel(ta::Environment& env, int dimx, int dimy, const std::unordered_set<Cell, CellHash>& obst, std::size_t agent,
              const Constraints& c, const Cell* task, const std::vector<Plan>& sol, float w, const State& start, Plan& out,
              long cap, Counters& cnt) {
  std::vector<int> table;
  if (task) table = ta::shortestPathTable(dimx, dimy, obst, *task);
  env.setLowLevelContext(agent, &c, task, task ? &table : nullptr);
  env.m_llExpandedThisSearch = 0;
  LLEnv ll{env, agent, sol, cap};
  AStarEpsilon<State, Action, int, LLEnv, StateHash> search(ll, w);
  bool ok = false;
  try {
    ok = search.search(start, out);
  } catch (const mapf::CapExceeded&) {
    cnt = Counters{env.m_llExpandedThisSearch, ll.decreaseKeys, ll.nodes, ll.maxTime};
    throw;
  }
  cnt = Counters{env.m_llExpandedThisSearch, ll.decreaseKeys, ll.nodes, ll.maxTime};
  return ok;
}

struct Call {  // recorder entry
  std::size_t agent;
  bool hasTask;
  Cell task;
  Constraints constraints;
  std::vector<Plan> context;
  bool ok;
  Plan plan;
  Counters cnt;
};

int actionCode(Action a) { return static_cast<int>(a); }

std::unordered_set<Cell, CellHash> obstacleSet(int n, const int32_t* xy) {
  std::unordered_set<Cell, CellHash> o;
  for (int i = 0; i < n; ++i) o.insert(Cell{xy[2 * i], xy[2 * i + 1]});
  return o;
}

}  // namespace

extern "C" {

// One AStarEpsilon::search over the task-assignment Environment.  hasGoal = 0: the agent has no task.  The focal context:
// nAgents paths, pathLen[a] states each ([x, y] pairs, concatenated in pathXY); agentIdx's own entry is skipped.
// out[0..6] = success, cost, fmin, n_states, decrease-key events, nodes created, largest time discovered.
// Returns 0, or -1 when the expansion cap was exceeded.
int ecbs_ta_ll_search(int dimx, int dimy, int nObst, const int32_t* obstXY, int startX, int startY, int hasGoal, int goalX,
                      int goalY, int nVC, const int32_t* vc, int nEC, const int32_t* ec, float w, int agentIdx, int nAgents,
                      const int32_t* pathLen, const int32_t* pathXY, int64_t capExpansions, int32_t* out, int64_t* expanded,
                      int32_t* statesTXY, int32_t* actions, int32_t* actionCosts, int cap) {
  const auto obst = obstacleSet(nObst, obstXY);
  Constraints cons;
  for (int i = 0; i < nVC; ++i) cons.vertex.insert(VertexConstraint{vc[3 * i], vc[3 * i + 1], vc[3 * i + 2]});
  for (int i = 0; i < nEC; ++i)
    cons.edge.insert(EdgeConstraint{ec[5 * i], ec[5 * i + 1], ec[5 * i + 2], ec[5 * i + 3], ec[5 * i + 4]});
  std::vector<Plan> sol(nAgents);
  {
    const int32_t* p = pathXY;
    for (int a = 0; a < nAgents; ++a)
      for (int t = 0; t < pathLen[a]; ++t, p += 2) sol[a].states.push_back(std::make_pair(State(t, p[0], p[1]), t));
  }
  ta::Environment env(dimx, dimy, obst);
  const Cell goal{goalX, goalY};
  Plan plan;
  Counters cnt;
  bool ok = false;
  int rc = 0;
  try {
    ok = lowLevel(env, dimx, dimy, obst, static_cast<std::size_t>(agentIdx), cons, hasGoal ? &goal : nullptr, sol, w,
                  State(0, startX, startY), plan, capExpansions, cnt);
  } catch (const mapf::CapExceeded&) {
    rc = -1;
  }
  *expanded = cnt.expanded;
  const int n = ok ? static_cast<int>(plan.states.size()) : 0;
  out[0] = ok ? 1 : 0;
  out[1] = ok ? plan.cost : 0;
  out[2] = ok ? plan.fmin : 0;
  out[3] = n;
  out[4] = static_cast<int32_t>(cnt.decreaseKeys);
  out[5] = static_cast<int32_t>(cnt.nodes);
  out[6] = cnt.maxTime;
  for (int k = 0; k < n && k < cap; ++k) {
    statesTXY[3 * k + 0] = plan.states[k].first.time;
    statesTXY[3 * k + 1] = plan.states[k].first.x;
    statesTXY[3 * k + 2] = plan.states[k].first.y;
    if (k + 1 < n) {
      actions[k] = actionCode(plan.actions[k].first);
      actionCosts[k] = plan.actions[k].second;
    }
  }
  return rc;
}

// ecbs_ta.hpp:94-297 for ONE fixed assignment; tasksXY[i] = (-1, -1): agent i has no task.
// stats[0..2] = solved, cost, high-level nodes expanded; endTXY [nAgents][3] = last state of every path.
// Every low-level call is serialised into buf (int32 words) as
//   agent, hasTask, taskX, taskY, success, cost, fmin, expanded, decrease-key events, nVC, nEC, nStates, nCtx,
//   vc[nVC][3], ec[nEC][5], statesTXY[nStates][3], actions[nStates - 1], actionCosts[nStates - 1],
//   nCtx x { len, xy[len][2] }        (the solution vector the search saw, its own entry included)
// Returns the words needed (call again with a bigger buffer if > bufWords); *nCalls = number of calls.
int64_t ecbs_ta_fixed(int dimx, int dimy, int nObst, const int32_t* obstXY, int nAgents, const int32_t* startsXY,
                      const int32_t* tasksXY, float w, int64_t maxHighLevel, int64_t* stats, int32_t* endTXY, int32_t* buf,
                      int64_t bufWords, int32_t* nCalls) {
  const auto obst = obstacleSet(nObst, obstXY);
  const std::size_t n = static_cast<std::size_t>(nAgents);
  std::vector<State> starts;
  std::vector<Cell> taskCells(n);
  std::vector<const Cell*> tasks(n, nullptr);
  for (std::size_t i = 0; i < n; ++i) {
    starts.push_back(State(0, startsXY[2 * i], startsXY[2 * i + 1]));
    if (tasksXY[2 * i] >= 0) {
      taskCells[i] = Cell{tasksXY[2 * i], tasksXY[2 * i + 1]};
      tasks[i] = &taskCells[i];
    }
  }
  ta::Environment env(dimx, dimy, obst);
  const mapf::Environment counting(dimx, dimy, {}, {});  // focalHeuristic ecbs_ta.cpp:347-382 == ecbs.cpp:315-350
  std::vector<Call> rec;
  auto search = [&](std::size_t i, const Constraints& c, const std::vector<Plan>& context, Plan& out) {
    const std::vector<Plan> seen = context;
    Counters cnt;
    const bool ok = lowLevel(env, dimx, dimy, obst, i, c, tasks[i], context, w, starts[i], out, -1, cnt);
    rec.push_back(Call{i, tasks[i] != nullptr, tasks[i] ? *tasks[i] : Cell{0, 0}, c, seen, ok, out, cnt});
    return ok;
  };

  struct Node {  // ecbs_ta.hpp:372-418
    std::vector<Plan> solution;
    std::vector<Constraints> constraints;
    int cost = 0, LB = 0, focalHeuristic = 0, id = 0;
  };
  struct Worse {  // :387-391
    bool operator()(const Node& a, const Node& b) const { return a.cost > b.cost; }
  };
  typedef ORACLE_HEAP<Node, Worse> Open;
  typedef Open::handle_type Handle;
  struct FocalWorse {  // :420-428
    const Open* open;
    bool operator()(const Handle& h1, const Handle& h2) const {
      const Node& a = (*open)[h1];
      const Node& b = (*open)[h2];
      if (a.focalHeuristic != b.focalHeuristic) return a.focalHeuristic > b.focalHeuristic;
      return a.cost > b.cost;
    }
  };

  bool solved = false;
  int cost = 0;
  int64_t hlExpanded = 0;
  std::vector<Plan> solution;
  [&]() {
    Node start;  // :96-138
    start.solution.resize(n);
    start.constraints.resize(n);
    for (std::size_t i = 0; i < n; ++i) {
      if (!search(i, start.constraints[i], start.solution, start.solution[i])) return;
      start.cost += start.solution[i].cost;
      start.LB += start.solution[i].fmin;
    }
    start.focalHeuristic = counting.focalHeuristic(start.solution);
    Open open;
    ORACLE_HEAP<Handle, FocalWorse> focal(FocalWorse{&open});
    const Handle h0 = open.push(start);
    focal.push(h0);
    int bestCost = open[h0].cost;
    int id = 1;
    while (!open.empty()) {
      {  // :181-201, int * float products
        const int oldBest = bestCost;
        bestCost = open.top().cost;
        if (bestCost > oldBest) {
          open.orderedWalk([&](Handle h) {
            const int val = open[h].cost;
            if (val > oldBest * w && val <= bestCost * w) focal.push(h);
            if (val > bestCost * w) return false;
            return true;
          });
        }
      }
      const Handle h = focal.top();  // :238-244
      Node P = open[h];
      if (++hlExpanded > maxHighLevel) return;
      focal.pop();
      open.erase(h);
      Conflict conflict;
      if (!env.getFirstConflict(P.solution, conflict)) {  // :246-251
        solution = P.solution;
        cost = P.cost;
        solved = true;
        return;
      }
      std::map<std::size_t, Constraints> split;
      env.createConstraintsFromConflict(conflict, split);
      for (const auto& c : split) {  // :260-297
        const std::size_t i = c.first;
        Node child = P;
        child.id = id;
        child.constraints[i].add(c.second);
        child.cost -= child.solution[i].cost;
        child.LB -= child.solution[i].fmin;
        const bool ok = search(i, child.constraints[i], child.solution, child.solution[i]);
        child.cost += child.solution[i].cost;
        child.LB += child.solution[i].fmin;
        child.focalHeuristic = counting.focalHeuristic(child.solution);
        if (ok) {
          const Handle hc = open.push(child);
          if (child.cost <= bestCost * w) focal.push(hc);
        }
        ++id;
      }
    }
  }();

  stats[0] = solved ? 1 : 0;
  stats[1] = solved ? cost : 0;
  stats[2] = hlExpanded;
  if (solved)
    for (std::size_t i = 0; i < n; ++i) {
      const State& s = solution[i].states.back().first;
      endTXY[3 * i] = s.time;
      endTXY[3 * i + 1] = s.x;
      endTXY[3 * i + 2] = s.y;
    }
  int64_t wd = 0;
  auto put = [&](int32_t v) {
    if (wd < bufWords) buf[wd] = v;
    ++wd;
  };
  for (const auto& c : rec) {
    const int nst = c.ok ? static_cast<int>(c.plan.states.size()) : 0;
    put(static_cast<int32_t>(c.agent)); put(c.hasTask ? 1 : 0); put(c.task.x); put(c.task.y); put(c.ok ? 1 : 0);
    put(c.ok ? c.plan.cost : 0); put(c.ok ? c.plan.fmin : 0); put(static_cast<int32_t>(c.cnt.expanded));
    put(static_cast<int32_t>(c.cnt.decreaseKeys));
    put(static_cast<int32_t>(c.constraints.vertex.size())); put(static_cast<int32_t>(c.constraints.edge.size())); put(nst);
    put(static_cast<int32_t>(c.context.size()));
    for (const auto& v : c.constraints.vertex) { put(v.time); put(v.x); put(v.y); }
    for (const auto& e : c.constraints.edge) { put(e.time); put(e.x1); put(e.y1); put(e.x2); put(e.y2); }
    for (int k = 0; k < nst; ++k) { put(c.plan.states[k].first.time); put(c.plan.states[k].first.x); put(c.plan.states[k].first.y); }
    for (int k = 0; k + 1 < nst; ++k) put(actionCode(c.plan.actions[k].first));
    for (int k = 0; k + 1 < nst; ++k) put(c.plan.actions[k].second);
    for (const auto& p : c.context) {
      put(static_cast<int32_t>(p.states.size()));
      for (const auto& s : p.states) { put(s.first.x); put(s.first.y); }
    }
  }
  *nCalls = static_cast<int32_t>(rec.size());
  return wd;
}

}  // extern "C"
