// The next-best assignment series (mrp_ll_assign_series_*): the open list, the partition of a popped node's solution
// space and the "drop below K" rule of NextBestAssignment (next_best_assignment.hpp:49-122).  Pure host logic, NO HIP:
// the constrained problems themselves are solved by a callback — the engine passes its batched launch, the CPU tests
// pass the emulator of the wave program (the separation of hl/launch_plan.hpp).
//
// A node is a set of constraints in the form the solver takes: per agent a mask of forbidden tasks (the reference's O)
// and a mode — forced to a task (I), must stay without (Oagents), must get one (Iagents), free.  Popping a node hands
// its matching out and creates, for every agent i that the node does not fix, in index order, the child "the agents
// before i keep what the matching gave them, agent i must differ"; children that are infeasible or have fewer pairs
// than the optimum's K are dropped.  Every matching of cardinality K is therefore produced exactly once, in
// non-decreasing order of cost; among nodes of equal cost the one created first is popped first.
#pragma once
#include <stdint.h>

#include <functional>
#include <queue>
#include <vector>

#include "../../../include/mrp_ll.h"

namespace mrp {
namespace host {

// solves n problems into n results (task_of buffers set by the caller); returns an MRP_LL_* call status
using AssignSolveFn = std::function<int(int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results)>;

struct AssignNode {
  int64_t cost = 0;
  uint64_t seq = 0;  // creation order: the tie-break
  std::vector<int32_t> taskOf, mode;
  std::vector<uint64_t> forbidden;
};
struct AssignNodeLater {
  bool operator()(const AssignNode& a, const AssignNode& b) const { return a.cost != b.cost ? a.cost > b.cost : a.seq > b.seq; }
};

}  // namespace host
}  // namespace mrp

struct mrp_ll_assign_series {
  static constexpr int32_t kNoCost = 0;  // what `cost` points at when the matrix has no entry
  const void* owner = nullptr;  // the context that created it
  int32_t nA = 0, nT = 0;
  bool gather = false;
  std::vector<int32_t> cost, heurIds, startsXY;  // the caller's problem, copied
  std::vector<uint64_t> allowed;
  bool hasAllowed = false;
  int32_t K = 0;  // the optimum's cardinality
  uint64_t nextSeq = 0;
  std::priority_queue<mrp::host::AssignNode, std::vector<mrp::host::AssignNode>, mrp::host::AssignNodeLater> open;

  mrp_ll_assign_problem problem(const mrp::host::AssignNode* node) const {  // the base problem under a node's constraints
    mrp_ll_assign_problem p;
    p.n_agents = nA;
    p.n_tasks = nT;
    p.cost = gather ? nullptr : cost.empty() ? &kNoCost : cost.data();  // (NULL would mean the gather form)
    p.heuristic_ids = gather ? heurIds.data() : nullptr;
    p.starts_xy = gather ? startsXY.data() : nullptr;
    p.allowed = gather && hasAllowed ? allowed.data() : nullptr;
    p.forbidden = node ? node->forbidden.data() : nullptr;
    p.mode = node ? node->mode.data() : nullptr;
    p.min_matching = node ? K : 0;
    return p;
  }
};

namespace mrp {
namespace host {

// n series from n unconstrained problems; their optima are solved by ONE call of `solve`.  On failure nothing is created.
inline int assignSeriesCreate(const void* owner, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_series** out,
                              const AssignSolveFn& solve) {
  for (int32_t k = 0; k < n; ++k) out[k] = nullptr;
  for (int32_t k = 0; k < n; ++k) {
    if (problems[k].mode || problems[k].forbidden || problems[k].min_matching != 0) return MRP_LL_E_INVALID;
    if (problems[k].n_agents < 0 || problems[k].n_agents > 64 || problems[k].n_tasks < 0 || problems[k].n_tasks > 64) return MRP_LL_E_INVALID;
  }
  std::vector<mrp_ll_assign_series*> made(static_cast<size_t>(n), nullptr);
  std::vector<mrp_ll_assign_problem> base(static_cast<size_t>(n));
  std::vector<mrp_ll_assign_result> res(static_cast<size_t>(n));
  std::vector<std::vector<int32_t>> taskOf(static_cast<size_t>(n));
  auto fail = [&](int rc) {
    for (mrp_ll_assign_series* s : made) delete s;
    return rc;
  };
  for (int32_t k = 0; k < n; ++k) {
    const mrp_ll_assign_problem& p = problems[k];
    mrp_ll_assign_series* s = made[k] = new mrp_ll_assign_series();
    s->owner = owner;
    s->nA = p.n_agents;
    s->nT = p.n_tasks;
    s->gather = p.cost == nullptr;
    if (!s->gather) {
      s->cost.assign(p.cost, p.cost + static_cast<size_t>(p.n_agents) * p.n_tasks);
    } else {
      if ((p.n_tasks > 0 && !p.heuristic_ids) || (p.n_agents > 0 && !p.starts_xy)) return fail(MRP_LL_E_INVALID);
      s->heurIds.assign(p.heuristic_ids, p.heuristic_ids + p.n_tasks);
      s->startsXY.assign(p.starts_xy, p.starts_xy + 2 * static_cast<size_t>(p.n_agents));
      s->hasAllowed = p.allowed != nullptr;
      if (p.allowed) s->allowed.assign(p.allowed, p.allowed + p.n_agents);
    }
    base[k] = s->problem(nullptr);
    taskOf[k].assign(static_cast<size_t>(p.n_agents) + 1, -1);
    res[k].task_of = taskOf[k].data();
  }
  const int rc = solve(n, base.data(), res.data());
  if (rc != MRP_LL_SUCCESS) return fail(rc);
  for (int32_t k = 0; k < n; ++k)
    if (res[k].status == MRP_LL_BAD_JOB) return fail(MRP_LL_E_INVALID);
  for (int32_t k = 0; k < n; ++k) {
    mrp_ll_assign_series* s = made[k];
    if (res[k].status == MRP_LL_OK) {
      s->K = res[k].matched;
      AssignNode root;
      root.cost = res[k].cost;
      root.seq = s->nextSeq++;
      root.taskOf.assign(taskOf[k].begin(), taskOf[k].begin() + s->nA);
      root.mode.assign(static_cast<size_t>(s->nA), MRP_LL_ASSIGN_FREE);
      root.forbidden.assign(static_cast<size_t>(s->nA), 0);
      s->open.push(std::move(root));
    }
    out[k] = s;
  }
  return MRP_LL_SUCCESS;
}

// One step of n distinct series: pops, hands the matchings out, solves all children of all pops by ONE call of `solve`
// (none when no series has a child).
inline int assignSeriesNext(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results,
                            const AssignSolveFn& solve) {
  for (int32_t k = 0; k < n; ++k) {
    if (!series[k] || (series[k]->nA > 0 && !results[k].task_of)) return MRP_LL_E_INVALID;
    for (int32_t m = 0; m < k; ++m)
      if (series[m] == series[k]) return MRP_LL_E_INVALID;
  }
  std::vector<AssignNode> kids;
  std::vector<int32_t> kidOf;
  for (int32_t k = 0; k < n; ++k) {
    mrp_ll_assign_series* s = series[k];
    mrp_ll_assign_result& r = results[k];
    if (s->open.empty()) {
      r.status = MRP_LL_NO_SOLUTION;
      r.matched = 0;
      r.cost = 0;
      for (int32_t a = 0; a < s->nA; ++a) r.task_of[a] = -1;
      continue;
    }
    const AssignNode node = s->open.top();
    s->open.pop();
    r.status = MRP_LL_OK;
    r.matched = s->K;
    r.cost = node.cost;
    for (int32_t a = 0; a < s->nA; ++a) r.task_of[a] = node.taskOf[a];
    // the partition (next_best_assignment.hpp:79-119)
    AssignNode fixed;  // the node with the agents before i fixed to what they got
    fixed.mode = node.mode;
    fixed.forbidden = node.forbidden;
    for (int32_t i = 0; i < s->nA; ++i) {
      if (node.mode[i] >= 0 || node.mode[i] == MRP_LL_ASSIGN_NO_TASK) continue;  // fixed by the node already
      AssignNode kid;
      kid.mode = fixed.mode;
      kid.forbidden = fixed.forbidden;
      if (node.taskOf[i] >= 0)
        kid.forbidden[i] |= 1ull << node.taskOf[i];  // another task, or none
      else
        kid.mode[i] = MRP_LL_ASSIGN_SOME_TASK;  // it had none: it must get one
      kid.taskOf.assign(static_cast<size_t>(s->nA), -1);
      kids.push_back(std::move(kid));
      kidOf.push_back(k);
      fixed.mode[i] = node.taskOf[i] >= 0 ? node.taskOf[i] : MRP_LL_ASSIGN_NO_TASK;
    }
  }
  if (kids.empty()) return MRP_LL_SUCCESS;
  std::vector<mrp_ll_assign_problem> probs(kids.size());
  std::vector<mrp_ll_assign_result> res(kids.size());
  for (size_t c = 0; c < kids.size(); ++c) {
    probs[c] = series[kidOf[c]]->problem(&kids[c]);
    res[c].task_of = kids[c].taskOf.data();
  }
  const int rc = solve(static_cast<int32_t>(kids.size()), probs.data(), res.data());
  if (rc != MRP_LL_SUCCESS) return rc;
  for (size_t c = 0; c < kids.size(); ++c) {
    mrp_ll_assign_series* s = series[kidOf[c]];
    if (res[c].status != MRP_LL_OK || res[c].matched < s->K) continue;  // (min_matching = K makes the solver say so itself)
    kids[c].cost = res[c].cost;
    kids[c].seq = s->nextSeq++;
    s->open.push(std::move(kids[c]));
  }
  return MRP_LL_SUCCESS;
}

}  // namespace host
}  // namespace mrp
