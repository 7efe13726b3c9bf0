// One ECBS-TA conflict tree as a resumable state machine (ecbs_ta.hpp:94-352 as example/ecbs_ta.cpp compiles it —
// REBUILT_FOCAL_LIST, STYLE_MINROOT, Cost = int — over that file's Environment), cut at the three things a tree asks of the
// engine: the next task assignment, a new root (whole, or its next search), the two searches of an expanded node's children.  Pure host
// logic: no engine call, no HIP; csrc/hl/mrp_hl_ecbs_ta.cpp drives many of these in the rounds of hl/ta_rounds.hpp.  Paths,
// constraints, conflicts, the conflict scan and the tree's base are hl/ta_tree_base.hpp's.
//   open list          d_ary_heap ordered by cost alone (:387-391), replayed by hl/exact_heap.hpp
//   focal list         rebuilt before every expansion (:160-179): the open list in ordered_begin() order up to the first node with
//                      (float)cost > nextRootNodeCost; ordered by focalHeuristic, then cost (:420-428)
//   nextRootNodeCost   an int: LB * w in binary32, truncated (:142, :344-345)
//   focalHeuristic     the number of all conflicts over t < (longest state count) - 1 (ecbs_ta.cpp:347-382): mrp_ll_conflict's count
//   a root             agent after agent, each search against the paths of the agents before it (:117-137, :318-329)
// The phase order differs from CBS-TA's: children first, THEN the new-root test (:302), the assignment, the root's searches and
// the new nextRootNodeCost, then the next expansion — one expansion can take several dependent engine phases.
// What the reference leaves undefined is defined in include/mrp_hl.h: an empty open list at :302 asks for a new root, a still
// empty one at :344 ends the tree MRP_HL_NO_SOLUTION, an empty focal list at :238 ends it MRP_HL_LL_ERROR.
#pragma once
#include "exact_heap.hpp"
#include "ta_tree_base.hpp"

namespace mrp_hl {
namespace ecbs_ta {

using ta::Conflict;
using ta::Cons;
using ta::PathP;

// focalHeuristic, ecbs_ta.cpp:347-382: every vertex and every edge pair of every step t < (longest state count) - 1
inline int32_t countConflicts(const std::vector<PathP>& sol) {
  int32_t n = 0;
  const int maxT = ta::longest(sol) - 1;
  for (int t = 0; t < maxT; ++t)
    for (size_t i = 0; i < sol.size(); ++i) {
      int32_t ax, ay, bx, by;
      ta::cellAt(*sol[i], t, ax, ay);
      ta::cellAt(*sol[i], t + 1, bx, by);
      for (size_t j = i + 1; j < sol.size(); ++j) {
        int32_t cx, cy, dx, dy;
        ta::cellAt(*sol[j], t, cx, cy);
        ta::cellAt(*sol[j], t + 1, dx, dy);
        n += (ax == cx && ay == cy) ? 1 : 0;
        n += (ax == dx && ay == dy && bx == cx && by == cy) ? 1 : 0;
      }
    }
  return n;
}

inline int32_t rootCostBound(int64_t lb, float w) { return static_cast<int32_t>(static_cast<float>(lb) * w); }

struct Node : ta::Node {  // ecbs_ta.hpp:372-391
  std::vector<int32_t> fmin;  // per agent: PlanResult::fmin of its path
  int64_t lb = 0;
  int32_t focalH = 0;
};

struct Tree : ta::TreeBase {
  float w = 1.0f;
  std::vector<Node> nodes;
  struct Worse {
    const std::vector<Node>* nodes;
    bool operator()(int32_t a, int32_t b) const { return (*nodes)[a].cost > (*nodes)[b].cost; }  // :387-391
  };
  struct FocalWorse {  // :420-428
    const std::vector<Node>* nodes;
    bool operator()(int32_t a, int32_t b) const {
      const Node& x = (*nodes)[a];
      const Node& y = (*nodes)[b];
      if (x.focalH != y.focalH) return x.focalH > y.focalH;
      return x.cost > y.cost;
    }
  };
  ExactHeap<Worse> open{Worse{&nodes}};
  int32_t nextRootNodeCost = 0;
  int32_t nextId = 1, solution = -1;
  bool firstRoot = true;
  // the pending root (a tree asks at most one of the base's three things of a round)
  std::vector<PathP> rootPaths;          // its paths so far: agents 0 .. rootAgent - 1, the rest null
  std::vector<int32_t> rootFmin;
  int32_t rootAgent = 0;                 // the agent whose search is pending

  // nextTaskAssignment (ecbs_ta.cpp:513-527), second half: `taskOf` == nullptr or without any task: the empty assignment.
  // The FIRST root is planned even then, every agent without a task (ecbs_ta.hpp:104, :117-137 — unlike cbs_ta.hpp:105-113);
  // a later one is not (:309).
  void gotAssignment(const int32_t* taskOf) {
    wantAssignment = false;
    bool any = false;
    for (int a = 0; taskOf && a < nAgents; ++a) any = any || taskOf[a] >= 0;
    if (any) numTaskAssignments += 1;
    if (!any && !firstRoot) {
      rootAttemptOver();
      return;
    }
    if (any)
      rootTasks.assign(taskOf, taskOf + nAgents);
    else
      rootTasks.assign(static_cast<size_t>(nAgents), -1);
    rootPaths.assign(static_cast<size_t>(nAgents), nullptr);
    rootFmin.assign(static_cast<size_t>(nAgents), 0);
    rootAgent = 0;
    wantRoot = true;
  }
  // The search of the pending root's agent `rootAgent`; path null: no path.
  void gotRootSearch(const PathP& path, int32_t fmin) {
    if (!path) {
      wantRoot = false;
      if (firstRoot)
        end(MRP_HL_NO_SOLUTION);  // :129-131
      else
        rootAttemptOver();        // :323-326: not pushed, id stays
      return;
    }
    rootPaths[rootAgent] = path;
    rootFmin[rootAgent] = fmin;
    rootAgent += 1;
    if (rootAgent < nAgents) return;
    pushRoot(countConflicts(rootPaths), ta::firstConflict(rootPaths));
  }
  // The pending root as ONE answer (mrp_ll_ta_eps_root_batch): paths and fmin of the agents 0 .. planned - 1 (a null path: that
  // search found none, and it is the last), and the engine's scan of the n paths when every agent has one.
  void gotRoot(const std::vector<PathP>& paths, const std::vector<int32_t>& fmin, int planned, const mrp_ll_conflict& scan) {
    for (int a = 0; a < planned; ++a) {
      if (!paths[a]) {
        gotRootSearch(nullptr, 0);
        return;
      }
      rootPaths[a] = paths[a];
      rootFmin[a] = fmin[a];
    }
    rootAgent = planned;
    if (planned == nAgents) pushRoot(scan.count, ta::conflictFromScan(scan, rootPaths));
  }
  // every agent of the pending root has a path: the node (:135-138, :327-333)
  void pushRoot(int32_t focalH, const Conflict& conflict) {
    wantRoot = false;
    Node n;
    n.sol = rootPaths;
    n.fmin = rootFmin;
    n.cons.assign(static_cast<size_t>(nAgents), std::make_shared<const Cons>());
    n.taskOf = rootTasks;
    for (int a = 0; a < nAgents; ++a) {
      n.cost += n.sol[a]->cost;
      n.lb += n.fmin[a];
    }
    n.focalH = focalH;
    n.isRoot = true;
    n.conflict = conflict;
    n.id = firstRoot ? 0 : nextId++;  // :102, :314 and :339
    nodes.push_back(std::move(n));
    open.push(static_cast<int32_t>(nodes.size()) - 1);
    nRoots += 1;
    if (firstRoot) {
      firstRoot = false;
      nextRootNodeCost = rootCostBound(nodes.back().lb, w);  // :142
    } else {
      rootAttemptOver();
    }
  }
  // :344-345 (an open list that is still empty here: the loop ends)
  void rootAttemptOver() {
    if (open.empty()) {
      end(MRP_HL_NO_SOLUTION);
      return;
    }
    nextRootNodeCost = rootCostBound(nodes[open.top()].lb, w);
  }
  // The two children of `popped`, in agent order; path null: no path (the child is not pushed, its id is used up).  Then the
  // new-root test of :302 (an empty open list asks too).
  void gotChildren(const PathP path[2], const int32_t fmin[2]) {
    wantChildren = false;
    for (int k = 0; k < 2; ++k) {
      const int32_t id = nextId++;
      if (!path[k]) continue;
      Node c = nodes[popped];
      c.id = id;
      const int a = childAgent[k];
      c.cons[a] = childCons[k];
      c.cost += path[k]->cost - c.sol[a]->cost;
      c.lb += fmin[k] - c.fmin[a];
      c.sol[a] = path[k];
      c.fmin[a] = fmin[k];
      c.focalH = countConflicts(c.sol);
      c.conflict = ta::firstConflict(c.sol);
      nodes.push_back(std::move(c));
      open.push(static_cast<int32_t>(nodes.size()) - 1);
    }
    if (open.empty() || nodes[open.top()].cost > nextRootNodeCost) wantAssignment = true;
  }
  // ecbs_ta.hpp:157-258 up to the next thing the engine has to do.
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
    ExactHeap<FocalWorse> focal{FocalWorse{&nodes}};  // :160-179
    open.walkOrdered([&](int32_t id) {
      if (!(static_cast<float>(nodes[id].cost) <= static_cast<float>(nextRootNodeCost))) return false;
      focal.push(id);
      return true;
    });
    if (focal.empty()) {
      end(MRP_HL_LL_ERROR);
      return;
    }
    popped = focal.top();  // :238-244
    hlExpanded += 1;
    open.erase(popped);
    const Node& P = nodes[popped];
    if (!P.conflict.found) {
      solution = popped;
      end(MRP_HL_SOLVED);
      return;
    }
    if (P.isRoot) rootConflicts += 1;
    constrainChildren(P.conflict, P.cons);
    wantChildren = true;
  }

  void write(mrp_hl_ta_solution& s) const { TreeBase::write(s, status == MRP_HL_SOLVED ? &nodes[solution] : nullptr); }
};

}  // namespace ecbs_ta
}  // namespace mrp_hl
