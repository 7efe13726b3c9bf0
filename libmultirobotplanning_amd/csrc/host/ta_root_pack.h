// The packer of mrp_ll_ta_root_batch: mrp_ll_ta_root -> the root's DevJob + three words per agent (ll_device.h
// kTaRootAgentWords), and the way back: the agents' DevResults, paths and the root's answer -> mrp_ll_result, planned,
// mrp_ll_conflict.  Pure host logic like ll_pack.h: no HIP, no mrp_ll_ctx; compiles with plain g++ -std=c++17
// (tests/support/ta_root_pack_check.cpp).
#pragma once
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../../include/mrp_ll.h"
#include "../ll_device.h"
#include "ll_pack.h"

namespace mrp {
namespace host {

struct TaRootStaging {
  std::vector<DevJob> recs;            // one per ACCEPTED root, in the caller's order
  std::vector<uint32_t> words;         // their agent words; DevJob::vc_off counts from wordBase
  std::vector<uint32_t> slotWords;     // mrp_ll_ta_eps_root_batch_stored: one path-store slot per agent of the roots that store,
                                       // behind `words` in the launch's buffer (DevJob::ec_off; ll_device.h)
  std::vector<int32_t> devRootOf;      // [n_roots] the root's record in recs, -1: refused
  std::vector<uint32_t> firstResult;   // [n_roots] its first result (refused: unused)
  uint32_t nResults = 0;               // results (DevResult + output area) of the launch
};

// What the call refuses (mrp_ll.h): a null array, n_agents outside 1 .. maxAgents (64; kTaRootWideMaxAgents for the _w calls), an unknown map, a start outside the grid, a task
// whose table is unknown or belongs to another map or whose goal lies outside the grid — every case in which packJob would
// refuse the ordinary job of one of the agents.  storeIds (mrp_ll_ta_eps_root_batch_stored; nullptr: none): the path-store
// slot of each agent's path, -1 = not stored; any other value outside the reserved store refuses the root.
static inline bool taRootValid(const PackEnv& env, const mrp_ll_ta_root& r, const int32_t* storeIds = nullptr,
                               uint32_t maxAgents = kTaRootMaxAgents) {
  if (r.n_agents < 1 || r.n_agents > static_cast<int32_t>(maxAgents)) return false;
  if (!r.starts_xy || !r.goals_xy || !r.heuristic_ids || !r.results) return false;
  if (storeIds)
    for (int a = 0; a < r.n_agents; ++a)
      if (storeIds[a] < -1 || (storeIds[a] >= 0 && static_cast<uint32_t>(storeIds[a]) >= env.pathStoreSlots)) return false;
  if (r.map_id < 0 || r.map_id >= static_cast<int32_t>(env.maps.size())) return false;
  const MapRec& mp = env.maps[r.map_id];
  auto inGrid = [&](int x, int y) { return x >= 0 && x < mp.dimx && y >= 0 && y < mp.dimy; };
  for (int a = 0; a < r.n_agents; ++a) {
    if (!inGrid(r.starts_xy[2 * a], r.starts_xy[2 * a + 1])) return false;
    const int32_t h = r.heuristic_ids[a];
    if (h < 0) continue;  // no task
    if (h >= static_cast<int32_t>(env.heurs.size()) || env.heurs[h].mapId != r.map_id) return false;
    if (!inGrid(r.goals_xy[2 * a], r.goals_xy[2 * a + 1])) return false;
  }
  return true;
}

// wordBase: where st.words will stand in the launch's constraint-word buffer.  algo / w: MRP_LL_ASTAR_TA (w unused) for
// mrp_ll_ta_root_batch, MRP_LL_ASTAR_EPS_TA and its weight for mrp_ll_ta_eps_root_batch (ll_device.h taEpsRootAgentJob).
// storeIds: nullptr, or per root nullptr or its agents' path-store slots (taRootValid): st.slotWords, which the caller
// copies behind st.words; a root without ids has no run there and keeps ec_off == vc_off.  maxAgents: taRootValid's.
static inline void packTaRootsAs(const PackEnv& env, uint32_t algo, float w, int32_t n, const mrp_ll_ta_root* roots, uint32_t wordBase,
                                 TaRootStaging& st, const int32_t* const* storeIds = nullptr, uint32_t maxAgents = kTaRootMaxAgents) {
  st.recs.clear();
  st.words.clear();
  st.slotWords.clear();
  std::vector<int64_t> slotRun;  // per record: where its run starts in slotWords, -1: none
  st.devRootOf.assign(n, -1);
  st.firstResult.assign(n, 0);
  st.nResults = 0;
  for (int32_t k = 0; k < n; ++k) {
    const mrp_ll_ta_root& r = roots[k];
    const int32_t* ids = storeIds ? storeIds[k] : nullptr;
    if (!taRootValid(env, r, ids, maxAgents)) continue;
    const MapRec& mp = env.maps[r.map_id];
    DevJob d;
    std::memset(&d, 0, sizeof(d));
    d.map_word_off = mp.wordOff;
    d.dimx = mp.dimx;
    d.dimy = mp.dimy;
    d.words_per_row = mp.wpr;
    d.algo = algo;
    d.w = w;
    d.max_expansions = r.max_expansions;
    d.last_goal_constraint = -1;  // no constraints
    d.vc_off = wordBase + static_cast<uint32_t>(st.words.size());
    d.ec_off = d.vc_off;
    d.store_out_id = kNoStoreSlot;
    d.n_ctx = static_cast<uint32_t>(r.n_agents);
    d.reserved = st.nResults;
    slotRun.push_back(ids ? static_cast<int64_t>(st.slotWords.size()) : -1);
    for (int a = 0; a < r.n_agents; ++a) {
      const bool noGoal = r.heuristic_ids[a] < 0;
      const uint32_t gx = noGoal ? 0u : static_cast<uint32_t>(r.goals_xy[2 * a]), gy = noGoal ? 0u : static_cast<uint32_t>(r.goals_xy[2 * a + 1]);
      st.words.push_back(static_cast<uint32_t>(r.starts_xy[2 * a]) | (static_cast<uint32_t>(r.starts_xy[2 * a + 1]) << 8) | (gx << 16) |
                         (gy << 24));
      st.words.push_back(noGoal ? 0u : env.heurs[r.heuristic_ids[a]].wordOff);
      st.words.push_back(noGoal ? kTaNoGoal : 0u);
      if (ids) st.slotWords.push_back(ids[a] >= 0 ? static_cast<uint32_t>(ids[a]) : kNoStoreSlot);
    }
    st.devRootOf[k] = static_cast<int32_t>(st.recs.size());
    st.firstResult[k] = st.nResults;
    st.nResults += static_cast<uint32_t>(r.n_agents);
    st.recs.push_back(d);
  }
  for (size_t q = 0; q < st.recs.size(); ++q)
    if (slotRun[q] >= 0) st.recs[q].ec_off = wordBase + static_cast<uint32_t>(st.words.size()) + static_cast<uint32_t>(slotRun[q]);
}

static inline void packTaRoots(const PackEnv& env, int32_t n, const mrp_ll_ta_root* roots, uint32_t wordBase, TaRootStaging& st,
                               uint32_t maxAgents = kTaRootMaxAgents) {
  packTaRootsAs(env, MRP_LL_ASTAR_TA, 0.0f, n, roots, wordBase, st, nullptr, maxAgents);
}

// The answer words of a root in its first result's output area.
static inline const uint32_t* taRootAnswer(const uint16_t* outPaths, uint32_t outStride, uint32_t firstResult) {
  return reinterpret_cast<const uint32_t*>(outPaths + static_cast<size_t>(firstResult) * outStride + (outStride - kScanOutHalfs));
}
// Before the launch: "nothing planned, no node" (what a root keeps whose workgroup never wrote).
static inline void blankTaRootAnswers(const TaRootStaging& st, uint16_t* outPaths, uint32_t outStride) {
  for (size_t k = 0; k < st.devRootOf.size(); ++k) {
    if (st.devRootOf[k] < 0) continue;
    uint32_t* w = const_cast<uint32_t*>(taRootAnswer(outPaths, outStride, st.firstResult[k]));
    std::memset(w, 0, (kTaRootPlannedWord + 1u) * 4u);
    w[0] = 0xFFFFFFFFu;
  }
}

static inline void notRunResult(mrp_ll_result& r, int32_t status) {
  r.status = status;
  r.cost = r.fmin = r.n_states = 0;
  r.expanded = 0;
  r.tier = 0;
}

// What the caller holds when nothing has run: planned = 0, found = -1 and the rest 0, every result of a refused root
// MRP_LL_BAD_JOB and of any other root MRP_LL_NOT_RUN, their other fields 0.  Written before the first step that can fail and
// again when one did, so that a non-zero return never leaves an output as the caller passed it in.
static inline void blankTaRootOutputs(const PackEnv& env, int32_t n, const mrp_ll_ta_root* roots, int32_t* planned,
                                      mrp_ll_conflict* conflicts, const int32_t* const* storeIds = nullptr,
                                      uint32_t maxAgents = kTaRootMaxAgents) {
  for (int32_t k = 0; k < n; ++k) {
    std::memset(&conflicts[k], 0, sizeof(mrp_ll_conflict));
    conflicts[k].found = -1;
    planned[k] = 0;
    const mrp_ll_ta_root& r = roots[k];
    if (!r.results || r.n_agents <= 0) continue;
    const int32_t status = taRootValid(env, r, storeIds ? storeIds[k] : nullptr, maxAgents) ? MRP_LL_NOT_RUN : MRP_LL_BAD_JOB;
    for (int a = 0; a < r.n_agents; ++a) notRunResult(r.results[a], status);
  }
}

// After the launch.  needScan receives the roots whose scan the device left to the host (every agent has a path, conflicts[k]
// is "none" until the caller has scanned).
static inline void unpackTaRoots(mrp_ll_stats& stats, const TaRootStaging& st, int32_t n, const mrp_ll_ta_root* roots,
                                 const DevResult* devResults, const uint16_t* outPaths, uint32_t outStride, int32_t* planned,
                                 mrp_ll_conflict* conflicts, std::vector<int32_t>& needScan) {
  static_assert(sizeof(mrp_ll_conflict) == 4 * kTaRootPlannedWord, "ten words");
  needScan.clear();
  for (int32_t k = 0; k < n; ++k) {
    const mrp_ll_ta_root& r = roots[k];
    std::memset(&conflicts[k], 0, sizeof(mrp_ll_conflict));
    conflicts[k].found = -1;
    planned[k] = 0;
    if (st.devRootOf[k] < 0) {  // refused: nothing was run
      if (r.results && r.n_agents > 0)
        for (int a = 0; a < r.n_agents; ++a) notRunResult(r.results[a], MRP_LL_BAD_JOB);
      continue;
    }
    const uint32_t first = st.firstResult[k];
    const uint32_t* ans = taRootAnswer(outPaths, outStride, first);
    const int32_t done = static_cast<int32_t>(std::min<uint32_t>(ans[kTaRootPlannedWord], static_cast<uint32_t>(r.n_agents)));
    planned[k] = done;
    bool allOk = done == r.n_agents;
    for (int a = 0; a < r.n_agents; ++a) {
      if (a >= done) {
        notRunResult(r.results[a], MRP_LL_NOT_RUN);
        continue;
      }
      const bool noGoal = r.heuristic_ids[a] < 0;
      const int32_t init = 0x40000000 | (noGoal ? 0x10000 : ((r.goals_xy[2 * a + 1] & 0xFF) << 8 | (r.goals_xy[2 * a] & 0xFF)));  // jobInitOf
      const DevResult& d = devResults[first + a];
      unpackResult(stats, d, outPaths + static_cast<size_t>(first + a) * outStride, false, r.results[a], false, 0, init);
      if (d.status != ST_OK) allOk = false;
    }
    if (!allOk) continue;
    if (ans[0] == kTaRootScanSkipped)
      needScan.push_back(k);
    else
      std::memcpy(&conflicts[k], ans, sizeof(mrp_ll_conflict));
  }
}

}  // namespace host
}  // namespace mrp
