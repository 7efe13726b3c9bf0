// The roots of CBS-TA and ECBS-TA conflict trees, one workgroup each, in ONE launch of one of ll_ta_root.h's four kernels:
// mrp_ll_ta_root_batch, mrp_ll_ta_eps_root_batch, mrp_ll_ta_eps_root_batch_stored and the _w calls for roots of up to 256
// agents.  ONE launcher for all five (taRootsLaunch): the packers of ta_root_pack.h / ta_eps_root_pack.h, the first ticket's
// staging buffers and stream (the engine is idle), the launch parameters of an ordinary MRP_LL_ASTAR_TA / MRP_LL_ASTAR_EPS_TA
// batch, unpackResult on the way back.  What the device left open is finished here before the call returns: a root whose
// table did not fit its arena slot's path area is scanned with mrp_ll_conflict_scan, and the agents an ECBS-TA kernel did
// not reach for that reason are run first, as ordinary MRP_LL_ASTAR_EPS_TA jobs with shipped contexts, one after the other
// (contexts of any width, ll_pack.h: the same path for the narrow and the wide call).
// mrp_ll_ta_eps_root_batch_stored: the agents' paths also go to the path-store slots the caller names, from the kernel
// (a run of slot words behind the agent words) and from the jobs run here (MRP_LL_JOB_STORE_RESULT) alike.
#pragma once
#include "ll_batch.h"
#include "ll_ctx.h"
#include "ll_heur_host.h"
#include "ll_maps.h"
#include "ta_eps_root_pack.h"

namespace {

// What the five calls differ in.
struct TaRootsCall {
  const char* name;                 // the prefix of its error messages
  bool eps;                         // false: CBS-TA, MRP_LL_ASTAR_TA; true: ECBS-TA, MRP_LL_ASTAR_EPS_TA under weight w
  float w;
  const int32_t* const* storeIds;   // mrp_ll_ta_eps_root_batch_stored: the paths' slots; nullptr: nothing stored
  bool wide;                        // roots of up to kTaRootWideMaxAgents agents
  uint32_t maxAgents() const { return wide ? mrp::kTaRootWideMaxAgents : mrp::kTaRootMaxAgents; }
};

// The agents planned[k] .. n - 1 of root R as ordinary jobs; paths: the planned agents' ([x, y] per state), extended here.
// storeIds: nullptr, or the agents' path-store slots (-1: not stored): their jobs carry MRP_LL_JOB_STORE_RESULT.
// Returns an engine error, or MRP_LL_SUCCESS with `all` = every agent has a path.
int taEpsRootRest(mrp_ll_ctx* ctx, float w, const mrp_ll_ta_root& R, const int32_t* storeIds, int32_t& planned,
                  std::vector<std::vector<int32_t>>& paths, bool& all) {
  const int32_t cap = ctx->env.maxHorizon;
  std::vector<int32_t> st(static_cast<size_t>(cap) * 3), ac(cap), co(cap), len(R.n_agents, 0);
  std::vector<const int32_t*> xy(R.n_agents, nullptr);
  int64_t budget = R.max_expansions;
  for (int a = 0; a < planned && budget >= 0; ++a) budget = budget > R.results[a].expanded ? budget - R.results[a].expanded : 0;
  all = true;
  while (planned < R.n_agents) {
    const int a = planned;
    for (int q = 0; q < R.n_agents; ++q) {
      len[q] = q < a ? static_cast<int32_t>(paths[q].size() / 2) : 0;
      xy[q] = q < a ? paths[q].data() : st.data();
    }
    mrp_ll_job j;
    std::memset(&j, 0, sizeof(j));
    j.map_id = R.map_id;
    j.algo = MRP_LL_ASTAR_EPS_TA;
    j.w = w;
    j.agent_idx = a;
    j.start_x = R.starts_xy[2 * a];
    j.start_y = R.starts_xy[2 * a + 1];
    j.n_agents = R.n_agents;
    j.path_len = len.data();
    j.path_xy = xy.data();
    j.max_expansions = budget;
    j.result_path_id = -1;
    if (storeIds && storeIds[a] >= 0) {
      j.result_path_id = storeIds[a];
      j.flags |= MRP_LL_JOB_STORE_RESULT;
    }
    j.heuristic_id = R.heuristic_ids[a];
    if (R.heuristic_ids[a] >= 0) {
      j.goal_x = R.goals_xy[2 * a];
      j.goal_y = R.goals_xy[2 * a + 1];
    } else {
      j.flags |= MRP_LL_JOB_NO_GOAL;
    }
    mrp_ll_result full;
    std::memset(&full, 0, sizeof(full));
    full.states_txy = st.data();
    full.actions = ac.data();
    full.action_costs = co.data();
    full.states_cap = cap;
    const int rc = mrp_ll_search_batch(ctx, 1, &j, &full);
    if (rc != MRP_LL_SUCCESS) return rc;
    mrp_ll_result& out = R.results[a];  // what the caller's buffers hold of it, as unpackResult fills them
    out.status = full.status; out.cost = full.cost; out.fmin = full.fmin; out.n_states = full.n_states;
    out.expanded = full.expanded; out.tier = full.tier;
    planned += 1;
    if (full.status != MRP_LL_OK) {
      all = false;
      break;
    }
    const int lim = std::min(full.n_states, out.states_cap);
    if (out.states_txy) std::memcpy(out.states_txy, st.data(), static_cast<size_t>(lim) * 12);
    for (int k = 0; k + 1 < full.n_states && k < out.states_cap; ++k) {
      if (out.actions) out.actions[k] = ac[k];
      if (out.action_costs) out.action_costs[k] = co[k];
    }
    if ((out.states_txy || out.actions) && out.states_cap < full.n_states) out.status = MRP_LL_PATH_TRUNCATED;
    paths.emplace_back();
    for (int k = 0; k < full.n_states; ++k) paths.back().insert(paths.back().end(), {st[3 * k + 1], st[3 * k + 2]});
    if (budget >= 0) budget = budget > full.expanded ? budget - full.expanded : 0;
  }
  for (int a = planned; a < R.n_agents; ++a) mrp::host::notRunResult(R.results[a], MRP_LL_NOT_RUN);
  return MRP_LL_SUCCESS;
}

int taRootsLaunch(mrp_ll_ctx* ctx, const TaRootsCall& c, int32_t n, const mrp_ll_ta_root* roots, int32_t* planned,
                  mrp_ll_conflict* conflicts) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = syncMaps(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = reserveMapsDev(ctx, 1);
  if (rc != MRP_LL_SUCCESS) return rc;
  Ticket& t = ctx->tickets[0];  // idle: no session, no batch in flight
  auto packT0 = std::chrono::steady_clock::now();
  mrp::host::TaRootStaging st;
  if (c.eps)
    mrp::host::packTaEpsRoots(ctx->env, c.w, n, roots, 0, st, c.storeIds, c.maxAgents());
  else
    mrp::host::packTaRoots(ctx->env, n, roots, 0, st, c.maxAgents());
  const uint32_t outStride = static_cast<uint32_t>(ctx->env.maxHorizon) + mrp::kScanOutHalfs;
  const uint32_t nDev = static_cast<uint32_t>(st.recs.size());
  // needScan: every agent has a path, the scan is left to the host; needRest (ECBS-TA alone): so are the agents behind planned[k]
  std::vector<int32_t> needScan, needRest;
  auto unpack = [&](const DevResult* devResults, const uint16_t* outPaths) {
    if (c.eps)
      mrp::host::unpackTaEpsRoots(ctx->stats, st, n, roots, devResults, outPaths, outStride, planned, conflicts, needScan, needRest);
    else
      mrp::host::unpackTaRoots(ctx->stats, st, n, roots, devResults, outPaths, outStride, planned, conflicts, needScan);
  };
  if (nDev == 0) {
    unpack(nullptr, nullptr);
    return MRP_LL_SUCCESS;
  }
  t.jobs.clear();
  t.cons.clear();
  t.paths.clear();
  HIPCHK(ctx, t.jobs.resize(nDev));
  HIPCHK(ctx, t.cons.resize(std::max<size_t>(st.words.size() + st.slotWords.size(), 16)));
  HIPCHK(ctx, t.paths.reserve(16));
  HIPCHK(ctx, t.results.resize(st.nResults));
  HIPCHK(ctx, t.outPaths.resize(static_cast<size_t>(st.nResults) * outStride));
  std::memcpy(t.jobs.host, st.recs.data(), nDev * sizeof(DevJob));
  std::memcpy(t.cons.host, st.words.data(), st.words.size() * 4);
  if (!st.slotWords.empty()) std::memcpy(t.cons.host + st.words.size(), st.slotWords.data(), st.slotWords.size() * 4);
  mrp::host::blankTaRootAnswers(st, t.outPaths.host, outStride);
  ctx->stats.pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - packT0).count();
  ctx->stats.staged_bytes += static_cast<int64_t>(nDev * sizeof(DevJob) + (st.words.size() + st.slotWords.size()) * 4);

  mrp::LaunchParams P;
  std::memset(&P, 0, sizeof(P));
  P.jobs = t.jobs.dev;
  P.results = t.results.dev;
  P.out_paths = t.outPaths.dev;
  P.cons = t.cons.dev;
  P.paths = t.paths.dev;
  P.queue_base = t.queueBase;  // (the kernel takes no tickets)
  P.n_jobs = nDev;
  uint32_t ldsBytes = 0;
  // the window an ordinary batch of the algorithm is launched with: the mixed kernel's for MRP_LL_ASTAR_EPS_TA, the A* kernels'
  rc = fillCommonParams(ctx, t, P, ldsBytes, c.eps ? 0 : 2);
  if (rc != MRP_LL_SUCCESS) return rc;
  const uint32_t grid = std::min<uint32_t>(nDev, static_cast<uint32_t>(ctx->opt.slots));
  HIPCHK(ctx, hipEventRecord(t.evK0, t.stream));
  HIPCHK(ctx, mrp_ll_launch_ta_root(&P, grid, ldsBytes, c.eps ? 1 : 0, c.wide ? 1 : 0, t.stream));
  HIPCHK(ctx, hipEventRecord(t.evK1, t.stream));
  HIPCHK(ctx, hipEventSynchronize(t.evK1));
  ctx->stats.launches += 1;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, t.evK0, t.evK1) == hipSuccess) ctx->stats.kernel_ms += ms;

  auto unpackT0 = std::chrono::steady_clock::now();
  unpack(t.results.host, t.outPaths.host);
  ctx->stats.unpack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - unpackT0).count();
  if (needScan.empty() && needRest.empty()) return MRP_LL_SUCCESS;
  // The paths of those roots as the device returned them, taken out of the ticket's buffers before the next batch uses them
  // (a needScan root has planned[k] == n_agents: all of its paths).
  std::vector<int32_t> todo = needScan;
  todo.insert(todo.end(), needRest.begin(), needRest.end());
  std::vector<std::vector<std::vector<int32_t>>> paths(todo.size());
  for (size_t q = 0; q < todo.size(); ++q) {
    const int32_t k = todo[q];
    for (int a = 0; a < planned[k]; ++a) {
      const uint32_t ri = st.firstResult[k] + static_cast<uint32_t>(a);
      const uint16_t* p = t.outPaths.host + static_cast<size_t>(ri) * outStride;
      const int32_t len = std::min<int32_t>(t.results.host[ri].n_states, ctx->env.maxHorizon);
      paths[q].emplace_back();
      for (int32_t s = 0; s < len; ++s) paths[q].back().insert(paths[q].back().end(), {p[s] & 0xFF, p[s] >> 8});
    }
  }
  std::vector<int32_t> setFirst(1, 0), pathFirst(1, 0), states, scanned;
  for (size_t q = 0; q < todo.size(); ++q) {
    const int32_t k = todo[q];
    bool all = true;
    if (q >= needScan.size()) {
      rc = taEpsRootRest(ctx, c.w, roots[k], c.storeIds ? c.storeIds[k] : nullptr, planned[k], paths[q], all);
      if (rc != MRP_LL_SUCCESS) return rc;
    }
    if (!all) continue;  // no node: found stays -1
    for (const std::vector<int32_t>& p : paths[q]) {
      states.insert(states.end(), p.begin(), p.end());
      pathFirst.push_back(static_cast<int32_t>(states.size() / 2));
    }
    setFirst.push_back(static_cast<int32_t>(pathFirst.size()) - 1);
    scanned.push_back(k);
  }
  if (scanned.empty()) return MRP_LL_SUCCESS;
  std::vector<mrp_ll_conflict> found(scanned.size());
  rc = mrp_ll_conflict_scan(ctx, static_cast<int32_t>(scanned.size()), setFirst.data(), pathFirst.data(), states.data(), found.data());
  if (rc != MRP_LL_SUCCESS) return rc;
  for (size_t q = 0; q < scanned.size(); ++q) conflicts[scanned[q]] = found[q];
  return MRP_LL_SUCCESS;
}

int taRootsBatch(mrp_ll_ctx* ctx, const TaRootsCall& c, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned,
                 mrp_ll_conflict* conflicts) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (nRoots < 0 || (c.eps && !(c.w >= 1.0f)) || (nRoots > 0 && (!roots || !planned || !conflicts))) {
    ctx->err = std::string(c.name) + ": invalid argument";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = std::string(c.name) + ": a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (nRoots == 0) return MRP_LL_SUCCESS;
  mrp::host::blankTaRootOutputs(ctx->env, nRoots, roots, planned, conflicts, c.storeIds, c.maxAgents());
  const int rc = taRootsLaunch(ctx, c, nRoots, roots, planned, conflicts);
  if (rc != MRP_LL_SUCCESS)
    mrp::host::blankTaRootOutputs(ctx->env, nRoots, roots, planned, conflicts, c.storeIds, c.maxAgents());  // nothing half-told
  return rc;
}

}  // namespace

extern "C" {

int mrp_ll_ta_root_batch(mrp_ll_ctx* ctx, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts) {
  return taRootsBatch(ctx, {"mrp_ll_ta_root_batch", false, 0.0f, nullptr, false}, nRoots, roots, planned, conflicts);
}

int mrp_ll_ta_root_batch_w(mrp_ll_ctx* ctx, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts) {
  return taRootsBatch(ctx, {"mrp_ll_ta_root_batch", false, 0.0f, nullptr, true}, nRoots, roots, planned, conflicts);
}

int mrp_ll_ta_eps_root_batch_stored(mrp_ll_ctx* ctx, float w, int32_t nRoots, const mrp_ll_ta_root* roots, mrp_ll_conflict* conflicts,
                                    int32_t* planned, const int32_t* const* resultPathIds) {
  return taRootsBatch(ctx, {"mrp_ll_ta_eps_root_batch", true, w, resultPathIds, false}, nRoots, roots, planned, conflicts);
}

int mrp_ll_ta_eps_root_batch(mrp_ll_ctx* ctx, float w, int32_t nRoots, const mrp_ll_ta_root* roots, mrp_ll_conflict* conflicts,
                             int32_t* planned) {
  return taRootsBatch(ctx, {"mrp_ll_ta_eps_root_batch", true, w, nullptr, false}, nRoots, roots, planned, conflicts);
}

int mrp_ll_ta_eps_root_batch_w(mrp_ll_ctx* ctx, float w, int32_t nRoots, const mrp_ll_ta_root* roots, mrp_ll_conflict* conflicts,
                               int32_t* planned) {
  return taRootsBatch(ctx, {"mrp_ll_ta_eps_root_batch", true, w, nullptr, true}, nRoots, roots, planned, conflicts);
}

}  // extern "C"
