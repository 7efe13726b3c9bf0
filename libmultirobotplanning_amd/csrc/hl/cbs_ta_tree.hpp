// One CBS-TA conflict tree as a resumable state machine (cbs_ta.hpp:87-214 over the Environment of example/cbs_ta.cpp), cut at
// the three things a tree asks of the engine: the next task assignment, the searches of a new root, the two searches of a
// popped node's children.  Pure host logic: no engine call, no HIP; csrc/hl/mrp_hl_ta.cpp drives many of these in the rounds
// of hl/ta_rounds.hpp.  Paths, constraints, the conflict scan, the node and the tree's base are hl/ta_tree_base.hpp's.
//   open list          boost d_ary_heap ordered by cost alone (cbs_ta.hpp:231-235), replayed by hl/exact_heap.hpp
//   ids                as cbs_ta.hpp:179-210
//   nextTaskAssignment :442-456, its `>` test and the count that rises only for a non-empty assignment
#pragma once
#include "exact_heap.hpp"
#include "ta_tree_base.hpp"

namespace mrp_hl {
namespace ta {

struct Tree : TreeBase {
  std::vector<Node> nodes;
  struct Worse {
    const std::vector<Node>* nodes;
    bool operator()(int32_t a, int32_t b) const { return (*nodes)[a].cost > (*nodes)[b].cost; }  // cbs_ta.hpp:231-235
  };
  ExactHeap<Worse> open{Worse{&nodes}};
  int32_t nextId = 1, solution = -1;
  bool firstRoot = true;

  // nextTaskAssignment, second half: `taskOf` == nullptr or without any task: the empty assignment
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
    constrainChildren(P.conflict, P.cons);
    wantChildren = true;
  }

  void write(mrp_hl_ta_solution& s) const { TreeBase::write(s, status == MRP_HL_SOLVED ? &nodes[solution] : nullptr); }
};

}  // namespace ta
}  // namespace mrp_hl
