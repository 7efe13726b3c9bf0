// One CBS-TA conflict tree as a resumable state machine (cbs_ta.hpp:87-214 over the Environment of example/cbs_ta.cpp), cut at
// the three things a tree asks of the engine: the next task assignment, the searches of a new root, the two searches of a
// popped node's children.  Pure host logic: no engine call, no HIP; csrc/hl/mrp_hl_ta.cpp drives many of these in rounds.
//   open list          boost d_ary_heap ordered by cost alone (cbs_ta.hpp:231-235), replayed by hl/exact_heap.hpp
//   getFirstConflict   example/cbs_ta.cpp:369-420: t = 0 .. (longest path's STATE COUNT) - 1 — one step more than example/cbs.cpp
//                      and mrp_ll_conflict_scan look at —, vertex pairs before edge pairs, pairs (i, j), i < j
//   constraints        createConstraintsFromConflict :422-440, children in agent order (std::map), ids as cbs_ta.hpp:179-210
//   nextTaskAssignment :442-456, its `>` test and the count that rises only for a non-empty assignment
#pragma once
#include <stdint.h>

#include <memory>
#include <vector>

#include "../../../include/mrp_hl.h"
#include "exact_heap.hpp"

namespace mrp_hl {
namespace ta {

struct Path {
  std::vector<int32_t> xy;  // x, y at time 0, 1, ...
  std::vector<int32_t> g;   // the path's cost up to that state (what the reference writes as t, cbs_ta.cpp:606-610)
  int32_t cost = 0;
  int32_t slot = -1;        // the engine's path-store slot that holds these cells too (ta_batch_setup.hpp PathSlots); -1: none
  int len() const { return static_cast<int>(g.size()); }
};
typedef std::shared_ptr<const Path> PathP;

struct Cons {
  std::vector<int32_t> vc;  // [n][3] time, x, y
  std::vector<int32_t> ec;  // [n][5] time, x1, y1, x2, y2
};
typedef std::shared_ptr<const Cons> ConsP;

struct Conflict {
  bool found = false;
  int32_t time = 0, agent1 = 0, agent2 = 0, type = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0;
};

inline void cellAt(const Path& p, int t, int32_t& x, int32_t& y) {  // getState, cbs_ta.cpp:472-481
  const int k = t < p.len() ? t : p.len() - 1;
  x = p.xy[2 * k];
  y = p.xy[2 * k + 1];
}
inline int longest(const std::vector<PathP>& sol) {
  int m = 0;
  for (const PathP& p : sol) m = p->len() > m ? p->len() : m;
  return m;
}
// the vertex pairs of ONE time step, in (i, j) order
inline bool vertexConflictAt(const std::vector<PathP>& sol, int t, Conflict& c) {
  for (size_t i = 0; i < sol.size(); ++i) {
    int32_t xi, yi;
    cellAt(*sol[i], t, xi, yi);
    for (size_t j = i + 1; j < sol.size(); ++j) {
      int32_t xj, yj;
      cellAt(*sol[j], t, xj, yj);
      if (xi == xj && yi == yj) {
        c = Conflict{true, t, static_cast<int32_t>(i), static_cast<int32_t>(j), 0, xi, yi, 0, 0};
        return true;
      }
    }
  }
  return false;
}
inline Conflict firstConflict(const std::vector<PathP>& sol, int fromT = 0) {  // cbs_ta.cpp:369-420
  Conflict c;
  const int maxT = longest(sol);
  for (int t = fromT; t < maxT; ++t) {
    if (vertexConflictAt(sol, t, c)) return c;
    for (size_t i = 0; i < sol.size(); ++i) {
      int32_t ax, ay, bx, by;
      cellAt(*sol[i], t, ax, ay);
      cellAt(*sol[i], t + 1, bx, by);
      for (size_t j = i + 1; j < sol.size(); ++j) {
        int32_t cx, cy, dx, dy;
        cellAt(*sol[j], t, cx, cy);
        cellAt(*sol[j], t + 1, dx, dy);
        if (ax == dx && ay == dy && bx == cx && by == cy) return Conflict{true, t, static_cast<int32_t>(i), static_cast<int32_t>(j), 1, ax, ay, bx, by};
      }
    }
  }
  return c;
}
// From the engine's scan of the same paths (mrp_ll_conflict: every step but the last): its first conflict if it has one, else
// what the last step adds — there nobody moves any more, so only vertex pairs are left to look at.
inline Conflict conflictFromScan(const mrp_ll_conflict& d, const std::vector<PathP>& sol) {
  if (d.found == 1) return Conflict{true, d.time, d.agent1, d.agent2, d.type, d.x1, d.y1, d.x2, d.y2};
  const int maxT = longest(sol);
  return firstConflict(sol, maxT > 0 ? maxT - 1 : 0);
}

struct Node {
  std::vector<PathP> sol;
  std::vector<ConsP> cons;
  std::vector<int32_t> taskOf;  // per agent: task index, -1 = none
  int64_t cost = 0;
  int32_t id = 0;
  bool isRoot = false;
  Conflict conflict;  // of `sol`, found when the node was made
};

struct Fnv {  // mrp_hl_solution.schedule_digest
  uint64_t h = 14695981039346656037ull;
  void byte(uint32_t b) { h = (h ^ (b & 0xFFu)) * 1099511628211ull; }
};

struct Tree {
  enum Status : int32_t { kRunning = -1 };
  // the instance
  int32_t nAgents = 0, mapId = -1;
  std::vector<int32_t> starts;           // [n][2]
  std::vector<int32_t> taskXY, taskHeur; // the distinct potential goals in order of first appearance; their tables
  int32_t maskWords = 1;                 // max(1, ceil(tasks / 64))
  std::vector<uint64_t> allowed;         // [nAgents][maskWords] the tasks an agent may take, as mrp_ll_assign_problem_w's masks
  // the search
  int32_t status = kRunning;
  std::vector<Node> nodes;
  struct Worse {
    const std::vector<Node>* nodes;
    bool operator()(int32_t a, int32_t b) const { return (*nodes)[a].cost > (*nodes)[b].cost; }  // cbs_ta.hpp:231-235
  };
  ExactHeap<Worse> open{Worse{&nodes}};
  int32_t nextId = 1;
  int64_t hlExpanded = 0, llExpanded = 0, numTaskAssignments = 0;
  int32_t nSearches = 0, nRootSearches = 0, nRoots = 0, rootConflicts = 0, solution = -1;
  bool firstRoot = true;
  // what the tree asks of this round
  bool wantAssignment = true, wantRoot = false, wantChildren = false;
  std::vector<int32_t> rootTasks;        // the assignment the pending root plans
  int32_t popped = -1;                   // the node whose children are pending
  int32_t childAgent[2] = {0, 0};
  ConsP childCons[2];

  Tree() = default;
  Tree(const Tree&) = delete;

  bool running() const { return status == kRunning; }
  void end(int32_t st) {
    status = st;
    wantAssignment = wantRoot = wantChildren = false;
  }
  // nextTaskAssignment (cbs_ta.cpp:442-456), first half: is the series asked at all?
  bool assignmentAllowed(int64_t maxTaskAssignments) const { return !(numTaskAssignments > maxTaskAssignments); }
  // ... second half: `taskOf` == nullptr or without any task: the empty assignment
  void gotAssignment(const int32_t* taskOf) {
    wantAssignment = false;
    bool any = false;
    for (int a = 0; taskOf && a < nAgents; ++a) any = any || taskOf[a] >= 0;
    if (!any) {
      if (firstRoot) end(MRP_HL_NO_SOLUTION);  // cbs_ta.hpp:105-113: no task, no search, `return false`
      return;                                  // a later root: `n.tasks.size() > 0` fails, no new root
    }
    numTaskAssignments += 1;
    rootTasks.assign(taskOf, taskOf + nAgents);
    wantRoot = true;
  }
  // The pending root's searches, agents 0 .. planned - 1 (paths[a] null: that search found no path); `conflict` of the node
  // when every agent has a path.
  void gotRoot(const std::vector<PathP>& paths, int planned, const Conflict& conflict) {
    wantRoot = false;
    bool all = planned == nAgents;
    for (int a = 0; a < planned; ++a) all = all && paths[a] != nullptr;
    const bool first = firstRoot;
    firstRoot = false;
    if (!all) {
      if (first) end(MRP_HL_NO_SOLUTION);  // cbs_ta.hpp:111-113
      return;                              // :159-170: not pushed, id stays
    }
    Node n;
    n.sol = paths;
    n.cons.assign(static_cast<size_t>(nAgents), std::make_shared<const Cons>());
    n.taskOf = rootTasks;
    for (const PathP& p : paths) n.cost += p->cost;
    n.isRoot = true;
    n.conflict = conflict;
    n.id = first ? 0 : nextId++;
    nodes.push_back(std::move(n));
    open.push(static_cast<int32_t>(nodes.size()) - 1);
    nRoots += 1;
  }
  // The two children of `popped`, in agent order; path null: no path (the child is not pushed, its id is used up).
  void gotChildren(const PathP path[2]) {
    wantChildren = false;
    for (int k = 0; k < 2; ++k) {
      const int32_t id = nextId++;
      if (!path[k]) continue;
      Node c = nodes[popped];
      c.id = id;
      c.isRoot = nodes[popped].isRoot;  // (`HighLevelNode newNode = P` copies the flag, cbs_ta.hpp:185)
      const int a = childAgent[k];
      c.cons[a] = childCons[k];
      c.cost += path[k]->cost - c.sol[a]->cost;
      c.sol[a] = path[k];
      c.conflict = firstConflict(c.sol);
      nodes.push_back(std::move(c));
      open.push(static_cast<int32_t>(nodes.size()) - 1);
    }
  }
  // cbs_ta.hpp:128-177 up to the next thing the engine has to do.
  void advance(int64_t maxHl) {
    if (!running() || wantAssignment || wantRoot || wantChildren) return;
    if (open.empty()) {
      end(MRP_HL_NO_SOLUTION);
      return;
    }
    if (maxHl >= 0 && hlExpanded + 1 > maxHl) {
      end(MRP_HL_CAP);
      return;
    }
    popped = open.top();
    hlExpanded += 1;
    open.pop();
    const Node& P = nodes[popped];
    if (!P.conflict.found) {
      solution = popped;
      end(MRP_HL_SOLVED);
      return;
    }
    if (P.isRoot) {
      rootConflicts += 1;
      wantAssignment = true;
    }
    const Conflict& c = P.conflict;
    childAgent[0] = c.agent1;
    childAgent[1] = c.agent2;
    for (int k = 0; k < 2; ++k) {
      auto nc = std::make_shared<Cons>(*P.cons[childAgent[k]]);
      if (c.type == 0) {
        nc->vc.insert(nc->vc.end(), {c.time, c.x1, c.y1});
      } else if (k == 0) {
        nc->ec.insert(nc->ec.end(), {c.time, c.x1, c.y1, c.x2, c.y2});
      } else {
        nc->ec.insert(nc->ec.end(), {c.time, c.x2, c.y2, c.x1, c.y1});
      }
      childCons[k] = nc;
    }
    wantChildren = true;
  }

  void write(mrp_hl_ta_solution& s) const {
    s.status = status;
    s.n_ll_searches = nSearches;
    s.cost = 0;
    s.makespan = 0;
    s.high_level_expanded = hlExpanded;
    s.low_level_expanded = llExpanded;
    s.num_task_assignments = numTaskAssignments;
    s.n_roots = nRoots;
    s.n_root_searches = nRootSearches;
    s.root_conflicts = rootConflicts;
    s.schedule_digest = 0;
    if (s.path_len)
      for (int a = 0; a < nAgents; ++a) s.path_len[a] = 0;
    if (s.task_xy)
      for (int a = 0; a < 2 * nAgents; ++a) s.task_xy[a] = -1;
    if (status != MRP_HL_SOLVED) return;
    const Node& n = nodes[solution];
    Fnv d;
    for (int a = 0; a < nAgents; ++a) {
      const Path& p = *n.sol[a];
      s.cost += p.cost;
      s.makespan = p.cost > s.makespan ? p.cost : s.makespan;
      for (int k = 0; k < p.len(); ++k) {
        d.byte(static_cast<uint32_t>(p.xy[2 * k]));
        d.byte(static_cast<uint32_t>(p.xy[2 * k + 1]));
        if (s.paths_xyt && k < s.path_cap) {
          int32_t* q = s.paths_xyt + (static_cast<size_t>(a) * s.path_cap + k) * 3;
          q[0] = p.xy[2 * k];
          q[1] = p.xy[2 * k + 1];
          q[2] = p.g[k];
        }
      }
      d.byte(0xFFu);
      if (s.path_len) s.path_len[a] = p.len();
      if (s.task_xy && n.taskOf[a] >= 0) {
        s.task_xy[2 * a] = taskXY[2 * n.taskOf[a]];
        s.task_xy[2 * a + 1] = taskXY[2 * n.taskOf[a] + 1];
      }
    }
    s.schedule_digest = d.h;
  }
};

}  // namespace ta
}  // namespace mrp_hl
