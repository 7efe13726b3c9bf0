// What the CBS-TA and the ECBS-TA conflict tree (hl/cbs_ta_tree.hpp, hl/ecbs_ta_tree.hpp) share: paths, constraints, conflicts
// and the conflict scan (example/ecbs_ta.cpp:440-511 equals example/cbs_ta.cpp there), the node, and the base of the two
// resumable state machines — the instance, the counters, what a tree asks of a round, the constraints of a popped node's
// children and the solution record.  Pure host logic: no engine call, no HIP.  The rules of each tree — what an empty
// assignment means, when the next assignment is asked for, which node is expanded — are the derived trees' alone.
//   getFirstConflict   example/cbs_ta.cpp:369-420: t = 0 .. (longest path's STATE COUNT) - 1 — one step more than example/cbs.cpp
//                      and mrp_ll_conflict_scan look at —, vertex pairs before edge pairs, pairs (i, j), i < j
//   constraints        createConstraintsFromConflict :422-440, children in agent order (std::map)
#pragma once
#include <stdint.h>

#include <memory>
#include <vector>

#include "../../../include/mrp_hl.h"

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
  Conflict conflict;  // getFirstConflict of `sol`, found when the node was made
};

struct Fnv {  // mrp_hl_solution.schedule_digest
  uint64_t h = 14695981039346656037ull;
  void byte(uint32_t b) { h = (h ^ (b & 0xFFu)) * 1099511628211ull; }
};

struct TreeBase {
  enum Status : int32_t { kRunning = -1 };
  // the instance
  int32_t nAgents = 0, mapId = -1;
  std::vector<int32_t> starts;           // [n][2]
  std::vector<int32_t> taskXY, taskHeur; // the distinct potential goals in order of first appearance; their tables
  int32_t maskWords = 1;                 // max(1, ceil(tasks / 64))
  std::vector<uint64_t> allowed;         // [nAgents][maskWords] the tasks an agent may take, as mrp_ll_assign_problem_w's masks
  // the search
  int32_t status = kRunning;
  int64_t hlExpanded = 0, llExpanded = 0, numTaskAssignments = 0;
  int32_t nSearches = 0, nRootSearches = 0, nRoots = 0, rootConflicts = 0;
  // what the tree asks of this round
  bool wantAssignment = true, wantRoot = false, wantChildren = false;
  std::vector<int32_t> rootTasks;        // the assignment the pending root plans
  int32_t popped = -1;                   // the node whose children are pending
  int32_t childAgent[2] = {0, 0};
  ConsP childCons[2];

  TreeBase() = default;
  TreeBase(const TreeBase&) = delete;

  bool running() const { return status == kRunning; }
  void end(int32_t st) {
    status = st;
    wantAssignment = wantRoot = wantChildren = false;
  }
  // nextTaskAssignment (cbs_ta.cpp:442-456, ecbs_ta.cpp:513-527), first half: is the series asked at all?
  bool assignmentAllowed(int64_t maxTaskAssignments) const { return !(numTaskAssignments > maxTaskAssignments); }
  // The popped node's conflict `c` as childAgent and childCons: each child's constraints are those of its agent in the popped
  // node (`cons`) and one more.
  void constrainChildren(const Conflict& c, const std::vector<ConsP>& cons) {
    childAgent[0] = c.agent1;
    childAgent[1] = c.agent2;
    for (int k = 0; k < 2; ++k) {
      auto nc = std::make_shared<Cons>(*cons[childAgent[k]]);
      if (c.type == 0) {
        nc->vc.insert(nc->vc.end(), {c.time, c.x1, c.y1});
      } else if (k == 0) {
        nc->ec.insert(nc->ec.end(), {c.time, c.x1, c.y1, c.x2, c.y2});
      } else {
        nc->ec.insert(nc->ec.end(), {c.time, c.x2, c.y2, c.x1, c.y1});
      }
      childCons[k] = nc;
    }
  }
  // The tree's record; `solved`: the node it ended MRP_HL_SOLVED with (its paths and tasks are written), else null.
  void write(mrp_hl_ta_solution& s, const Node* solved) const {
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
    if (!solved) return;
    Fnv d;
    for (int a = 0; a < nAgents; ++a) {
      const Path& p = *solved->sol[a];
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
      if (s.task_xy && solved->taskOf[a] >= 0) {
        s.task_xy[2 * a] = taskXY[2 * solved->taskOf[a]];
        s.task_xy[2 * a + 1] = taskXY[2 * solved->taskOf[a] + 1];
      }
    }
    s.schedule_digest = d.h;
  }
};

}  // namespace ta
}  // namespace mrp_hl
