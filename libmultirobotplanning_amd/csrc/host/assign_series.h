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
// A node's mask is `maskWords` 64-bit words per agent: one word is the narrow series (mrp_ll_assign_series_create), more
// are the wide one (mrp_ll_assign_series_create_w, up to 256 tasks).  A series remembers which it is; one step takes
// both kinds and hands the narrow children to the narrow solver and the wide children to the wide one.
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
using AssignSolveWideFn = std::function<int(int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_result* results)>;

struct AssignNode {
  int64_t cost = 0;
  uint64_t seq = 0;  // creation order: the tie-break
  std::vector<int32_t> taskOf, mode;
  std::vector<uint64_t> forbidden;  // [nA][maskWords]
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
  bool wide = false;       // made by assignSeriesCreateWide: its problems go to the wide solver
  int32_t maskWords = 1;   // words per agent of `allowed` and of a node's `forbidden`
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
  mrp_ll_assign_problem_w problemWide(const mrp::host::AssignNode* node) const {
    const mrp_ll_assign_problem n = problem(node);
    return mrp_ll_assign_problem_w{n.n_agents, n.n_tasks, n.cost, n.heuristic_ids, n.starts_xy, n.allowed, n.forbidden, n.mode,
                                   n.min_matching, maskWords};
  }
};

namespace mrp {
namespace host {

inline int32_t seriesMaskWords(const mrp_ll_assign_problem&) { return 1; }
inline int32_t seriesMaskWords(const mrp_ll_assign_problem_w& p) { return p.mask_words; }
inline mrp_ll_assign_problem seriesBase(const mrp_ll_assign_series& s, const mrp_ll_assign_problem*) { return s.problem(nullptr); }
inline mrp_ll_assign_problem_w seriesBase(const mrp_ll_assign_series& s, const mrp_ll_assign_problem_w*) { return s.problemWide(nullptr); }

// n series from n unconstrained problems; their optima are solved by ONE call of `solve`.  On failure nothing is created.
// Both kinds of series: Problem is mrp_ll_assign_problem (limit 64, one mask word) or mrp_ll_assign_problem_w (limit 256).
template <class Problem, class Solve>
inline int assignSeriesCreateAny(const void* owner, int32_t n, const Problem* problems, mrp_ll_assign_series** out, const Solve& solve,
                                 bool wide, int32_t limit) {
  for (int32_t k = 0; k < n; ++k) out[k] = nullptr;
  for (int32_t k = 0; k < n; ++k) {
    if (problems[k].mode || problems[k].forbidden || problems[k].min_matching != 0) return MRP_LL_E_INVALID;
    if (problems[k].n_agents < 0 || problems[k].n_agents > limit || problems[k].n_tasks < 0 || problems[k].n_tasks > limit) return MRP_LL_E_INVALID;
    const int32_t mw = seriesMaskWords(problems[k]);
    if (mw < 1 || mw > 4 || mw < (problems[k].n_tasks + 63) / 64) return MRP_LL_E_INVALID;  // (a node's masks need every word)
  }
  std::vector<mrp_ll_assign_series*> made(static_cast<size_t>(n), nullptr);
  std::vector<Problem> base(static_cast<size_t>(n));
  std::vector<mrp_ll_assign_result> res(static_cast<size_t>(n));
  std::vector<std::vector<int32_t>> taskOf(static_cast<size_t>(n));
  auto fail = [&](int rc) {
    for (mrp_ll_assign_series* s : made) delete s;
    return rc;
  };
  for (int32_t k = 0; k < n; ++k) {
    const Problem& p = problems[k];
    mrp_ll_assign_series* s = made[k] = new mrp_ll_assign_series();
    s->owner = owner;
    s->wide = wide;
    s->maskWords = seriesMaskWords(p);
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
      if (p.allowed) s->allowed.assign(p.allowed, p.allowed + static_cast<size_t>(p.n_agents) * s->maskWords);
    }
    base[k] = seriesBase(*s, &p);
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
      root.forbidden.assign(static_cast<size_t>(s->nA) * s->maskWords, 0);
      s->open.push(std::move(root));
    }
    out[k] = s;
  }
  return MRP_LL_SUCCESS;
}

inline int assignSeriesCreate(const void* owner, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_series** out,
                              const AssignSolveFn& solve) {
  return assignSeriesCreateAny(owner, n, problems, out, solve, false, 64);
}
inline int assignSeriesCreateWide(const void* owner, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_series** out,
                                  const AssignSolveWideFn& solve) {
  return assignSeriesCreateAny(owner, n, problems, out, solve, true, 256);
}

// One step of n distinct series: pops, hands the matchings out, solves all children of all pops by ONE call of `solve`
// (none when no series has a child).  With narrow and wide series mixed: the narrow children by one call of `solve`, the
// wide ones by one call of `solveWide` (a wide series without a wide solver is MRP_LL_E_INVALID).
inline int assignSeriesNext(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results,
                            const AssignSolveFn& solve, const AssignSolveWideFn& solveWide) {
  for (int32_t k = 0; k < n; ++k) {
    if (!series[k] || (series[k]->nA > 0 && !results[k].task_of)) return MRP_LL_E_INVALID;
    if (series[k]->wide && !solveWide) return MRP_LL_E_INVALID;
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
        kid.forbidden[static_cast<size_t>(i) * s->maskWords + (node.taskOf[i] >> 6)] |= 1ull << (node.taskOf[i] & 63);  // another task, or none
      else
        kid.mode[i] = MRP_LL_ASSIGN_SOME_TASK;  // it had none: it must get one
      kid.taskOf.assign(static_cast<size_t>(s->nA), -1);
      kids.push_back(std::move(kid));
      kidOf.push_back(k);
      fixed.mode[i] = node.taskOf[i] >= 0 ? node.taskOf[i] : MRP_LL_ASSIGN_NO_TASK;
    }
  }
  if (kids.empty()) return MRP_LL_SUCCESS;
  // the children in creation order, each kind in a batch of its own; `at[c]` is child c's place in its batch
  std::vector<mrp_ll_assign_problem> probs;
  std::vector<mrp_ll_assign_problem_w> probsWide;
  std::vector<mrp_ll_assign_result> res, resWide;
  std::vector<size_t> at(kids.size());
  for (size_t c = 0; c < kids.size(); ++c) {
    const mrp_ll_assign_series* s = series[kidOf[c]];
    const mrp_ll_assign_result r{0, 0, 0, kids[c].taskOf.data()};
    if (s->wide) {
      at[c] = probsWide.size();
      probsWide.push_back(s->problemWide(&kids[c]));
      resWide.push_back(r);
    } else {
      at[c] = probs.size();
      probs.push_back(s->problem(&kids[c]));
      res.push_back(r);
    }
  }
  if (!probs.empty()) {
    const int rc = solve(static_cast<int32_t>(probs.size()), probs.data(), res.data());
    if (rc != MRP_LL_SUCCESS) return rc;
  }
  if (!probsWide.empty()) {
    const int rc = solveWide(static_cast<int32_t>(probsWide.size()), probsWide.data(), resWide.data());
    if (rc != MRP_LL_SUCCESS) return rc;
  }
  for (size_t c = 0; c < kids.size(); ++c) {
    mrp_ll_assign_series* s = series[kidOf[c]];
    const mrp_ll_assign_result& r = s->wide ? resWide[at[c]] : res[at[c]];
    if (r.status != MRP_LL_OK || r.matched < s->K) continue;  // (min_matching = K makes the solver say so itself)
    kids[c].cost = r.cost;
    kids[c].seq = s->nextSeq++;
    s->open.push(std::move(kids[c]));
  }
  return MRP_LL_SUCCESS;
}
inline int assignSeriesNext(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results,
                            const AssignSolveFn& solve) {
  return assignSeriesNext(n, series, results, solve, AssignSolveWideFn());
}

}  // namespace host
}  // namespace mrp
