// Device results -> the caller's records: mrp_ll_result of a search or of a root chain, mrp_ll_conflict of a flagged job.
// HIP-free; included by ll_pack.h.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../../include/mrp_ll.h"
#include "../ll_device.h"

namespace mrp {
namespace host {

static inline int actionFromDelta(int dx, int dy) {
  if (dx == 0 && dy == 0) return MRP_LL_ACT_WAIT;
  if (dx == -1 && dy == 0) return MRP_LL_ACT_LEFT;
  if (dx == 1 && dy == 0) return MRP_LL_ACT_RIGHT;
  if (dx == 0 && dy == 1) return MRP_LL_ACT_UP;
  if (dx == 0 && dy == -1) return MRP_LL_ACT_DOWN;
  return -1;
}

// What unpackResult needs to know about a job besides its device result: initial_cost (A*) / start_time (SIPP), or — for
// MRP_LL_ASTAR_TA, whose initial cost is always 0 — bit 30 + the goal cell and the no-task flag.
static inline int32_t jobInitOf(const mrp_ll_job& j, bool ok) {
  if (!ok) return 0;
  if (j.algo == MRP_LL_ASTAR_TA || j.algo == MRP_LL_ASTAR_EPS_TA)
    return 0x40000000 | ((j.flags & MRP_LL_JOB_NO_GOAL) ? 0x10000 : ((j.goal_y & 0xFF) << 8 | (j.goal_x & 0xFF)));
  return j.initial_cost;
}

// The conflicts of a flagged job (ll_device.h kCtxScan: ten words at the end of the job's output area) -> the caller's
// mrp_ll_conflict; a job that did not end with a path — or never ran — has none: found = -1, the rest 0.
static inline void unpackConflicts(const DevResult& d, const uint16_t* outArea, uint32_t outStride, bool rejected, mrp_ll_conflict& c) {
  static_assert(sizeof(mrp_ll_conflict) == 40 && sizeof(mrp_ll_conflict) <= 2 * kScanOutHalfs, "ten words");
  std::memset(&c, 0, sizeof(c));
  c.found = -1;
  if (rejected || d.status != ST_OK) return;
  std::memcpy(&c, outArea + (outStride - kScanOutHalfs), sizeof(c));
}

// Device result -> caller's mrp_ll_result (+ statistics).
static inline void unpackResult(mrp_ll_stats& stats, const DevResult& d, const uint16_t* p, bool rejected, mrp_ll_result& r, bool sipp,
                                int dimx, int32_t init) {
  if (rejected) {
    r.status = MRP_LL_BAD_JOB;
    r.cost = r.fmin = r.n_states = 0;
    r.expanded = 0;
    r.tier = 0;
    return;
  }
  r.status = d.status;
  r.cost = d.cost;
  r.fmin = d.fmin;
  if (init & 0x40000000) {
    // not an initial cost: the goal of an MRP_LL_ASTAR_TA job (used for the action costs below)
  } else if (d.status == ST_OK && init != 0) {
    if (sipp) {
      r.cost = d.cost - init;  // sipp.hpp:103; fmin stays the A* f value (absolute)
    } else {                   // a_star.hpp:64,78: every node but the start carries initialCost in g and f
      r.cost = d.cost + init;
      if (d.n_states > 1) r.fmin = d.fmin + init;
    }
  }
  r.n_states = d.status == ST_OK ? d.n_states : 0;
  r.expanded = d.expanded;
  r.tier = static_cast<int32_t>(d.tier & 0xFFu);
  stats.jobs += 1;
  stats.expansions += d.expanded;
  stats.nodes_created += d.nodes_created;
  stats.migrated += (d.tier & 0xFFu) ? 1 : 0;
  for (int q = 0; q < 8; ++q) stats.prof[q] += d.prof[q];
  if (d.status == ST_OK && sipp) {
    // raw A* states (cell | g << 16) -> PlanResult with explicit Wait actions (sipp.hpp:105-128)
    const uint32_t* raw = reinterpret_cast<const uint32_t*>(p);
    const int nRaw = d.n_states;
    int out = 0;
    bool trunc = false;
    auto emit = [&](int cell, int t, int action, int cost, bool hasAction) {
      if (out < r.states_cap) {
        if (r.states_txy) {
          r.states_txy[3 * out] = t;
          r.states_txy[3 * out + 1] = cell % dimx;
          r.states_txy[3 * out + 2] = cell / dimx;
        }
        if (hasAction) {
          if (r.actions) r.actions[out] = action;
          if (r.action_costs) r.action_costs[out] = cost;
        }
      } else {
        trunc = true;
      }
      out += 1;
    };
    for (int k = 0; k + 1 < nRaw; ++k) {
      const int c0 = raw[k] & 0xFFFF, g0 = raw[k] >> 16, c1 = raw[k + 1] & 0xFFFF, g1 = raw[k + 1] >> 16;
      const int motion = actionFromDelta(c1 % dimx - c0 % dimx, c1 / dimx - c0 / dimx);
      const int waitTime = (g1 - g0) - 1;
      if (waitTime == 0) {
        emit(c0, g0, motion, g1 - g0, true);
      } else {
        emit(c0, g0, MRP_LL_ACT_WAIT, waitTime, true);
        emit(c0, g0 + waitTime, motion, 1, true);
      }
    }
    if (nRaw > 0) emit(raw[nRaw - 1] & 0xFFFF, raw[nRaw - 1] >> 16, 0, 0, false);
    r.n_states = out;
    if (trunc && (r.states_txy || r.actions)) r.status = MRP_LL_PATH_TRUNCATED;
    return;
  }
  if (d.status == ST_OK) {
    int n = d.n_states;
    int lim = std::min(n, r.states_cap);
    if (r.states_txy)
      for (int k = 0; k < lim; ++k) {
        r.states_txy[3 * k] = k;
        r.states_txy[3 * k + 1] = p[k] & 0xFF;
        r.states_txy[3 * k + 2] = p[k] >> 8;
      }
    if (r.actions)
      for (int k = 0; k + 1 < n && k < r.states_cap; ++k)
        r.actions[k] = actionFromDelta((p[k + 1] & 0xFF) - (p[k] & 0xFF), (p[k + 1] >> 8) - (p[k] >> 8));
    if (r.action_costs) {
      // MRP_LL_ASTAR_TA (init carries goal and flags, see jobInitOf): a Wait at the goal is free (cbs_ta.cpp:333-338)
      const bool ta = (init & 0x40000000) != 0, noGoal = (init & 0x10000) != 0;
      const int tgx = init & 0xFF, tgy = (init >> 8) & 0xFF;
      for (int k = 0; k + 1 < n && k < r.states_cap; ++k) {
        const bool wait = p[k] == p[k + 1];
        const bool atGoal = noGoal || ((p[k] & 0xFF) == tgx && (p[k] >> 8) == tgy);
        r.action_costs[k] = (ta && wait && atGoal) ? 0 : 1;
      }
    }
    if ((r.states_txy || r.actions) && r.states_cap < n) r.status = MRP_LL_PATH_TRUNCATED;
  }
}

// Entries of mrp_ll_result::chain_results that a job's collection fills in (JobNote::chain): n_agents - agent_idx for a
// root chain — accepted or rejected, in a session or in a batch —, 0 for every other job.
static inline int32_t chainResultsOf(const mrp_ll_job& j) {
  return (j.flags & MRP_LL_JOB_ROOT_CHAIN) ? std::max(1, j.n_agents - j.agent_idx) : 0;
}

// The output of a root chain (ll_device.h kCtxChain) -> the caller's per-agent results; `count` = results the job may fill,
// `outWords` = words of the job's host area.
static inline void unpackChain(mrp_ll_stats& stats, const DevResult& d, const uint16_t* out, bool rejected, mrp_ll_result& r,
                               int32_t count, uint32_t outWords) {
  r.status = rejected ? MRP_LL_BAD_JOB : d.status;
  // the root node's conflicts, when the chain planned every agent of the instance (mrp_ll.h): count and first one, else -1
  r.cost = (rejected || d.status != ST_OK) ? -1 : d.cost;
  r.fmin = (rejected || d.status != ST_OK) ? -1 : d.fmin;
  r.tier = 0;
  const int32_t done = (rejected || d.status != ST_OK) ? 0 : std::min<int32_t>(d.n_states, count);
  r.n_states = done;
  r.expanded = rejected ? 0 : d.expanded;
  if (!rejected)
    for (int q = 0; q < 8; ++q) stats.prof[q] += d.prof[q];
  if (!r.chain_results) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(out);
  for (int32_t i = 0; i < count; ++i) {
    mrp_ll_result& ri = r.chain_results[i];
    if (i < done) {
      const uint32_t* e = w + static_cast<size_t>(i) * kChainEntryWords;
      DevResult f;
      std::memset(&f, 0, sizeof(f));
      f.status = static_cast<int32_t>(e[0]);
      f.cost = static_cast<int32_t>(e[1]);
      f.fmin = static_cast<int32_t>(e[2]);
      f.n_states = static_cast<int32_t>(e[3]);
      f.expanded = e[4];
      // (the path offset is a word the device wrote: never read past the job's host area)
      const uint32_t pathWords = (static_cast<uint32_t>(std::max(f.n_states, 0)) + 1u) / 2u;
      if (e[5] > outWords || pathWords > outWords - e[5]) {
        f.status = ST_BAD;
        f.n_states = 0;
      }
      unpackResult(stats, f, reinterpret_cast<const uint16_t*>(w + (f.status == ST_BAD ? 0u : e[5])), false, ri, false, 0, 0);
    } else {
      ri.status = MRP_LL_NOT_RUN;
      ri.cost = ri.fmin = ri.n_states = 0;
      ri.expanded = 0;
      ri.tier = 0;
    }
  }
}

}  // namespace host
}  // namespace mrp
