// The packer of the assignment calls: mrp_ll_assign_problem -> AssignJob + staged words (assign_layout.h), and the way
// back, result record -> mrp_ll_assign_result.  Pure host logic like ll_pack.h: no HIP, no mrp_ll_ctx; what it needs of
// the engine (maps, heuristic tables) it reads from the PackEnv.  tests/support/assign_host_check.cpp runs it under the
// host sanitizers, tests/support/emu_assign.cpp feeds the CPU emulation of the wave program with the words it writes.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../../include/mrp_ll.h"
#include "../assign_layout.h"
#include "ll_pack.h"

namespace mrp {
namespace host {

struct AssignStaging {
  std::vector<as::AssignJob> jobs;  // the problems that run
  std::vector<int32_t> problemOf;   // jobs[k] is problems[problemOf[k]]
  std::vector<uint32_t> data;       // what the jobs' offsets count in
  uint32_t outWords = 0;            // size of the result area
  uint32_t ldsBytes = 0;            // the launch's window: its largest problem's
  void clear() {
    jobs.clear();
    problemOf.clear();
    data.clear();
    outWords = 0;
    ldsBytes = 0;
  }
};

// Validates one problem and, when it is sound, appends it to the staging.  MRP_LL_OK or MRP_LL_BAD_JOB (nothing appended).
inline int packAssignProblem(const PackEnv& env, const mrp_ll_assign_problem& p, int32_t index, AssignStaging& st) {
  const int32_t nA = p.n_agents, nT = p.n_tasks;
  if (nA < 0 || nT < 0 || nA > static_cast<int32_t>(as::kMaxDim) || nT > static_cast<int32_t>(as::kMaxDim)) return MRP_LL_BAD_JOB;
  if (p.min_matching < 0 || p.min_matching > static_cast<int32_t>(as::kMaxDim)) return MRP_LL_BAD_JOB;
  const bool gather = p.cost == nullptr;
  const size_t cells = static_cast<size_t>(nA) * static_cast<size_t>(nT);
  int stride = 0;
  if (!gather) {
    for (size_t k = 0; k < cells; ++k)
      if (p.cost[k] != MRP_LL_ASSIGN_NO_EDGE && (p.cost[k] < 0 || p.cost[k] > static_cast<int32_t>(as::kMaxCost))) return MRP_LL_BAD_JOB;
  } else {
    if ((nT > 0 && !p.heuristic_ids) || (nA > 0 && !p.starts_xy)) return MRP_LL_BAD_JOB;
    int32_t mapId = -1;
    for (int32_t t = 0; t < nT; ++t) {
      const int32_t h = p.heuristic_ids[t];
      if (h < 0 || h >= static_cast<int32_t>(env.heurs.size())) return MRP_LL_BAD_JOB;
      if (t > 0 && env.heurs[h].mapId != mapId) return MRP_LL_BAD_JOB;
      mapId = env.heurs[h].mapId;
    }
    if (nT > 0) {
      const MapRec& mp = env.maps[mapId];
      stride = heurStride(mp);
      for (int32_t a = 0; a < nA; ++a) {
        const int32_t x = p.starts_xy[2 * a], y = p.starts_xy[2 * a + 1];
        if (x < 0 || x >= mp.dimx || y < 0 || y >= mp.dimy) return MRP_LL_BAD_JOB;
      }
    }
  }
  if (p.mode)
    for (int32_t a = 0; a < nA; ++a)
      if (p.mode[a] >= nT || p.mode[a] < MRP_LL_ASSIGN_SOME_TASK) return MRP_LL_BAD_JOB;

  as::AssignJob j;
  j.nA = static_cast<uint32_t>(nA);
  j.nT = static_cast<uint32_t>(nT);
  j.minMatching = static_cast<uint32_t>(p.min_matching);
  j.pad = 0;
  j.costOff = as::kNoCostOff;
  j.taskOff = 0;
  if (!gather) {
    j.costOff = static_cast<uint32_t>(st.data.size());
    for (size_t k = 0; k < cells; ++k)
      st.data.push_back(p.cost[k] == MRP_LL_ASSIGN_NO_EDGE ? as::kNoEdge : static_cast<uint32_t>(p.cost[k]));
  } else {
    j.taskOff = static_cast<uint32_t>(st.data.size());
    for (int32_t t = 0; t < nT; ++t) st.data.push_back(env.heurs[p.heuristic_ids[t]].wordOff);
  }
  j.agentOff = static_cast<uint32_t>(st.data.size());
  for (int32_t a = 0; a < nA; ++a) {
    uint64_t forb = p.forbidden ? p.forbidden[a] : 0;
    if (gather && p.allowed) forb |= ~p.allowed[a];  // a task the agent may not take is a forbidden one
    const int32_t m = p.mode ? p.mode[a] : MRP_LL_ASSIGN_FREE;
    st.data.push_back(static_cast<uint32_t>(forb));
    st.data.push_back(static_cast<uint32_t>(forb >> 32));
    st.data.push_back(m >= 0                         ? static_cast<uint32_t>(m)
                      : m == MRP_LL_ASSIGN_FREE      ? as::kModeFree
                      : m == MRP_LL_ASSIGN_NO_TASK   ? as::kModeNoTask
                                                     : as::kModeSomeTask);
    st.data.push_back(gather && nT > 0 ? static_cast<uint32_t>(p.starts_xy[2 * a + 1] * stride + p.starts_xy[2 * a]) : 0u);
  }
  j.outOff = st.outWords;
  st.outWords += as::outWords(j.nA);
  st.ldsBytes = std::max(st.ldsBytes, as::ldsBytes(j.nA));
  st.jobs.push_back(j);
  st.problemOf.push_back(index);
  return MRP_LL_OK;
}

// Packs a batch: results[k].status becomes MRP_LL_BAD_JOB for a rejected problem (matched 0, cost 0, task_of all -1),
// every other problem is staged.
inline void packAssignBatch(const PackEnv& env, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results,
                            AssignStaging& st) {
  st.clear();
  for (int32_t k = 0; k < n; ++k) {
    const int rc = problems[k].n_agents > 0 && !results[k].task_of ? MRP_LL_BAD_JOB : packAssignProblem(env, problems[k], k, st);
    results[k].status = rc;
    results[k].matched = 0;
    results[k].cost = 0;
    if (rc != MRP_LL_OK && results[k].task_of)
      for (int32_t a = 0; a < problems[k].n_agents && a < static_cast<int32_t>(as::kMaxDim); ++a) results[k].task_of[a] = -1;
  }
}

// The staged problems' result records -> the caller's results.
inline void unpackAssignBatch(const AssignStaging& st, const uint32_t* out, mrp_ll_assign_result* results) {
  for (size_t k = 0; k < st.jobs.size(); ++k) {
    const as::AssignJob& j = st.jobs[k];
    const uint32_t* r = out + j.outOff;
    mrp_ll_assign_result& res = results[st.problemOf[k]];
    res.status = r[0] == as::kStatusSolved ? MRP_LL_OK : MRP_LL_NO_SOLUTION;
    res.matched = static_cast<int32_t>(r[1]);
    res.cost = static_cast<int64_t>(static_cast<uint64_t>(r[3]) << 32 | r[2]);
    for (uint32_t a = 0; a < j.nA; ++a) res.task_of[a] = static_cast<int32_t>(r[as::kOutHeadWords + a]);
  }
}

// ---- the wide form (mrp_ll_assign_problem_w -> AssignJobWide): the narrow packer with 256 in the place of 64 ----

struct AssignStagingWide {
  std::vector<as::AssignJobWide> jobs;
  std::vector<int32_t> problemOf;
  std::vector<uint32_t> data;
  uint32_t outWords = 0;      // the result records
  uint64_t scratchWords = 0;  // behind them: the matrices of the gather problems with memory rows
  uint32_t ldsBytes = 0;
  void clear() {
    jobs.clear();
    problemOf.clear();
    data.clear();
    outWords = 0;
    scratchWords = 0;
    ldsBytes = 0;
  }
};

// As packAssignProblem; `budget` is the LDS budget that decides the row source (as::rowSourceWide).  A gather problem
// with memory rows gets its scratch offset relative to the scratch area: packAssignBatchWide makes it absolute.
inline int packAssignProblemWide(const PackEnv& env, const mrp_ll_assign_problem_w& p, int32_t index, uint32_t budget,
                                 AssignStagingWide& st) {
  const int32_t nA = p.n_agents, nT = p.n_tasks, kMax = static_cast<int32_t>(as::kMaxDimWide);
  if (nA < 0 || nT < 0 || nA > kMax || nT > kMax) return MRP_LL_BAD_JOB;
  if (p.min_matching < 0 || p.min_matching > kMax) return MRP_LL_BAD_JOB;
  const int32_t mw = p.mask_words;
  if (mw < 1 || mw > static_cast<int32_t>(as::kMaxWordsWide)) return MRP_LL_BAD_JOB;
  if ((p.allowed || p.forbidden) && mw < (nT + 63) / 64) return MRP_LL_BAD_JOB;
  const bool gather = p.cost == nullptr;
  const size_t cells = static_cast<size_t>(nA) * static_cast<size_t>(nT);
  int stride = 0;
  if (!gather) {
    for (size_t k = 0; k < cells; ++k)
      if (p.cost[k] != MRP_LL_ASSIGN_NO_EDGE && (p.cost[k] < 0 || p.cost[k] > static_cast<int32_t>(as::kMaxCost))) return MRP_LL_BAD_JOB;
  } else {
    if ((nT > 0 && !p.heuristic_ids) || (nA > 0 && !p.starts_xy)) return MRP_LL_BAD_JOB;
    int32_t mapId = -1;
    for (int32_t t = 0; t < nT; ++t) {
      const int32_t h = p.heuristic_ids[t];
      if (h < 0 || h >= static_cast<int32_t>(env.heurs.size())) return MRP_LL_BAD_JOB;
      if (t > 0 && env.heurs[h].mapId != mapId) return MRP_LL_BAD_JOB;
      mapId = env.heurs[h].mapId;
    }
    if (nT > 0) {
      const MapRec& mp = env.maps[mapId];
      stride = heurStride(mp);
      for (int32_t a = 0; a < nA; ++a) {
        const int32_t x = p.starts_xy[2 * a], y = p.starts_xy[2 * a + 1];
        if (x < 0 || x >= mp.dimx || y < 0 || y >= mp.dimy) return MRP_LL_BAD_JOB;
      }
    }
  }
  if (p.mode)
    for (int32_t a = 0; a < nA; ++a)
      if (p.mode[a] >= nT || p.mode[a] < MRP_LL_ASSIGN_SOME_TASK) return MRP_LL_BAD_JOB;

  as::AssignJobWide j;
  j.nA = static_cast<uint32_t>(nA);
  j.nT = static_cast<uint32_t>(nT);
  j.minMatching = static_cast<uint32_t>(p.min_matching);
  j.words = as::wordsWide(j.nA, j.nT);
  j.rowSource = as::rowSourceWide(j.nA, j.nT, budget);
  j.scratchOff = 0;
  j.pad[0] = j.pad[1] = 0;
  j.costOff = as::kNoCostOff;
  j.taskOff = 0;
  if (!gather) {
    j.costOff = static_cast<uint32_t>(st.data.size());
    for (size_t k = 0; k < cells; ++k)
      st.data.push_back(p.cost[k] == MRP_LL_ASSIGN_NO_EDGE ? as::kNoEdge : static_cast<uint32_t>(p.cost[k]));
  } else {
    j.taskOff = static_cast<uint32_t>(st.data.size());
    for (int32_t t = 0; t < nT; ++t) st.data.push_back(env.heurs[p.heuristic_ids[t]].wordOff);
  }
  j.agentOff = static_cast<uint32_t>(st.data.size());
  for (int32_t a = 0; a < nA; ++a) {
    const int32_t m = p.mode ? p.mode[a] : MRP_LL_ASSIGN_FREE;
    st.data.push_back(m >= 0                         ? static_cast<uint32_t>(m)
                      : m == MRP_LL_ASSIGN_FREE      ? as::kModeFree
                      : m == MRP_LL_ASSIGN_NO_TASK   ? as::kModeNoTask
                                                     : as::kModeSomeTask);
    st.data.push_back(gather && nT > 0 ? static_cast<uint32_t>(p.starts_xy[2 * a + 1] * stride + p.starts_xy[2 * a]) : 0u);
    for (uint32_t w = 0; w < j.words; ++w) {  // (a word the caller's masks do not have covers no task: mask_words >= ceil(nT / 64))
      const bool given = static_cast<int32_t>(w) < mw;
      uint64_t forb = p.forbidden && given ? p.forbidden[static_cast<size_t>(a) * mw + w] : 0;
      if (gather && p.allowed && given) forb |= ~p.allowed[static_cast<size_t>(a) * mw + w];
      st.data.push_back(static_cast<uint32_t>(forb));
      st.data.push_back(static_cast<uint32_t>(forb >> 32));
    }
  }
  j.outOff = st.outWords;
  st.outWords += as::outWords(j.nA);
  const uint32_t scratch = as::scratchWordsWide(j.nA, j.nT, gather, budget);
  if (scratch) {
    j.scratchOff = static_cast<uint32_t>(st.scratchWords);  // (a batch beyond 2^32 words is refused by the caller)
    st.scratchWords += scratch;
  }
  st.ldsBytes = std::max(st.ldsBytes, as::ldsBytesWide(j.nA, j.nT, budget));
  st.jobs.push_back(j);
  st.problemOf.push_back(index);
  return MRP_LL_OK;
}

inline void packAssignBatchWide(const PackEnv& env, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_result* results,
                                uint32_t budget, AssignStagingWide& st) {
  st.clear();
  for (int32_t k = 0; k < n; ++k) {
    const int rc = problems[k].n_agents > 0 && !results[k].task_of ? MRP_LL_BAD_JOB : packAssignProblemWide(env, problems[k], k, budget, st);
    results[k].status = rc;
    results[k].matched = 0;
    results[k].cost = 0;
    if (rc != MRP_LL_OK && results[k].task_of)
      for (int32_t a = 0; a < problems[k].n_agents && a < static_cast<int32_t>(as::kMaxDimWide); ++a) results[k].task_of[a] = -1;
  }
  for (as::AssignJobWide& j : st.jobs)  // the scratch area lies behind the result records
    if (j.costOff == as::kNoCostOff && j.rowSource == as::kRowsMem) j.scratchOff += st.outWords;
}

inline void unpackAssignBatchWide(const AssignStagingWide& st, const uint32_t* out, mrp_ll_assign_result* results) {
  for (size_t k = 0; k < st.jobs.size(); ++k) {
    const as::AssignJobWide& j = st.jobs[k];
    const uint32_t* r = out + j.outOff;
    mrp_ll_assign_result& res = results[st.problemOf[k]];
    res.status = r[0] == as::kStatusSolved ? MRP_LL_OK : MRP_LL_NO_SOLUTION;
    res.matched = static_cast<int32_t>(r[1]);
    res.cost = static_cast<int64_t>(static_cast<uint64_t>(r[3]) << 32 | r[2]);
    for (uint32_t a = 0; a < j.nA; ++a) res.task_of[a] = static_cast<int32_t>(r[as::kOutHeadWords + a]);
  }
}

}  // namespace host
}  // namespace mrp
