// The root node of an ECBS-TA conflict tree as ONE workgroup's work (ecbs_ta.hpp:117-138, :306-343;
// mrp_ll_ta_eps_root_batch): the agents are planned in index order, each with no constraints, each by the search an ordinary
// MRP_LL_ASTAR_EPS_TA job runs (runJobTaEps, arena tier) with the paths of the agents BEFORE it as its focal context, and
// when every agent has a path the workgroup scans the node with ns::nodeScan — whose count is the node's focalHeuristic.
// A batch launch that ends, like ll_ta_root.h: workgroup b takes roots b, b + grid, ...
// Needs ll_jobs.h, ll_ta.h (runJobTaEps<true>) and ll_ta_root.h (the scan's blocks in the window, the answer's layout).
//
// The root's record is ll_ta_root.h's with algo MRP_LL_ASTAR_EPS_TA and w; the per-agent descriptor is made from it by
// ll_device.h taEpsRootAgentJob — word for word what host/ll_pack.h packJob makes for the ordinary job, except path_off: the
// table is not shipped.
//
// ONE time-major table [rows][npad] (x | y << 8, npad = agents rounded up to 16) in the slot's path area is both the focal
// context of the next search and the scan's input.  runJobTaEps<true> takes it where it lies (the ordinary job copies its
// shipped table into this very area).  The search loads a whole row for every lane < npad and repeats row t_pad - 1 beyond
// the table, so BEFORE EVERY SEARCH: every column not yet planned — the searching agent's own and the pad columns
// included — holds kEmptyCell in every row, every planned column is held at its last cell up to the longest path so far,
// and t_pad is that length.  A path longer than all before it therefore extends the rows first (planned columns at their
// last cell, the others empty), then its own column is written.  Agent 0 searches with no table at all (n_agents_pad = 0),
// as its ordinary job does.
// The table is written and read by this one wave with plain stores and loads, under the rule ll_ta_root.h's header cites;
// __syncthreads() stands between a column's stores and the next search's loads.
// A table that would outgrow the path area (only under MRP_LL_ARENA_PATHS_BYTES) ends the kernel's part behind the agent
// whose path did not fit: the answer says kTaRootScanSkipped and how many agents are planned, the host runs the rest.
// mrp_ll_ta_eps_root_batch_stored: cons[ec_off + a] names the path-store slot that also receives agent a's path
// (publishPath, as an ordinary job with MRP_LL_JOB_STORE_RESULT); the slot of an agent the root did not plan is not touched.
#ifndef MRP_LL_TA_EPS_ROOT_H
#define MRP_LL_TA_EPS_ROOT_H

#include "ll_ta_root.h"

namespace mrp {

DEVI void runTaEpsRoot(const LaunchParams& P, const DevJob* rootSrc, uint8_t* smem, uint8_t* arenaSlot, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  DevResult res;
  beginJob<true>(rootSrc, jobS, res, 0);
  const uint32_t n = rfl(jobS.n_ctx), base = rfl(jobS.reserved);
  if (n < 1u || n > kTaRootMaxAgents) return;  // (the host refuses such a root: nothing is run, nothing written)
  const uint32_t* who = P.cons + rfl(jobS.vc_off);
  const uint32_t* storeIds = rfl(jobS.ec_off) != rfl(jobS.vc_off) ? P.cons + rfl(jobS.ec_off) : nullptr;  // (ll_device.h)
  int64_t budget = (int64_t)rfl64((uint64_t)jobS.max_expansions);  // < 0: unlimited
  const uint32_t npad = (n + 15u) & ~15u;  // <= 64: one lane per column
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint16_t* table = (uint16_t*)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint32_t* ansDst = (uint32_t*)(P.out_paths + (size_t)base * P.out_host_stride + (P.out_host_stride - kScanOutHalfs));
  uint32_t planned = 0, maxLen = 0, lastLen = 0;
  uint32_t endL = kEmptyCell;  // lane a: the last cell of agent a's path (kEmptyCell: not planned)
  bool allOk = true, tableOk = true;
  for (uint32_t a = 0; allOk && tableOk && a < n; ++a) {
    const uint32_t sg = rfl(hostLoad32(who + a * kTaRootAgentWords)), heurOff = rfl(hostLoad32(who + a * kTaRootAgentWords + 1u)),
                   flags = rfl(hostLoad32(who + a * kTaRootAgentWords + 2u));
    const uint32_t storeId = storeIds ? rfl(hostLoad32(storeIds + a)) : kNoStoreSlot;  // kNoStoreSlot: the path goes to the host only
    __syncthreads();
    taEpsRootAgentJob(jobS, sg, heurOff, flags, budget, a ? npad : 0u, a ? maxLen : 0u);  // (every lane stores the same words)
    __syncthreads();
    runJobTaEps<true>(&jobS, &resS, arenaSlot, P.maps, P.cons, P.paths, P.arena_scratch_off, P.out_stride, P.arena_nodes,
                      P.arena_rows, P.arena_row_words, P.arena_paths_bytes, P.path_store, P.path_store_stride, P.path_store_slots);
    __syncthreads();
    res.status = rfli(resS.status); res.cost = rfli(resS.cost); res.fmin = rfli(resS.fmin);
    res.n_states = rfli(resS.n_states);
    res.expanded = (int64_t)rfl64((uint64_t)resS.expanded);
    res.nodes_created = rfl(resS.nodes_created);
    res.tier = rfl(resS.tier);
    for (int q = 0; q < 8; ++q) res.prof[q] = 0;
    endJob(res, resS, P.results + base + a);
    planned += 1;
    if (rfl((uint32_t)res.status) != (uint32_t)ST_OK) {  // no path / budget / capacity: the root ends behind this agent
      allOk = false;
      break;
    }
    const uint32_t len = rfl((uint32_t)res.n_states);
    publishPath(P, outPath, len, (uint32_t*)(P.out_paths + (size_t)(base + a) * P.out_host_stride), [&] { return storeId; });
    const uint32_t newMax = len > maxLen ? len : maxLen;
    if (len >= 1u && (uint64_t)newMax * npad * 2u <= (uint64_t)P.arena_paths_bytes) {
      // the rows this path adds: the planned columns at their last cell, every other column empty (its own comes below)
      if (lane < npad && lane != a)
        for (uint32_t t = maxLen; t < newMax; ++t) table[t * npad + lane] = (uint16_t)endL;
      const uint32_t last = outPath[len - 1u];  // (all lanes, same address)
      for (uint32_t t = lane; t < newMax; t += 64) table[t * npad + a] = t < len ? outPath[t] : (uint16_t)last;
      endL = lane == a ? last : endL;
      maxLen = newMax;
    } else {
      tableOk = false;
    }
    lastLen = len;
    if (budget >= 0) {
      const int64_t expanded = (int64_t)rfl64((uint64_t)res.expanded);
      budget = budget > expanded ? budget - expanded : 0;
    }
  }
  __syncthreads();
  if (!allOk) {  // no node: found = -1, the rest 0
    if (lane <= kTaRootPlannedWord) hostStore32(ansDst + lane, lane == 0 ? 0xFFFFFFFFu : lane == kTaRootPlannedWord ? planned : 0u);
    return;
  }
  if (!tableOk) {  // the table outgrew the slot's path area: the host plans the agents behind `planned` and scans
    if (lane <= kTaRootPlannedWord) hostStore32(ansDst + lane, lane == 0 ? kTaRootScanSkipped : lane == kTaRootPlannedWord ? planned : 0u);
    return;
  }
  // nodeScan's node: the table's columns (every one complete), and for the last agent the path its search left in outPath
  ns::NsJob nj;
  nj.nAgents = n; nj.nPad = npad; nj.tPad = maxLen;
  nj.agentIdx = n - 1u;
  nj.nStates = lastLen;
  nj.tabLds = ns::kTableInGlobal;
  nj.tabG = (uint64_t)table;
  nj.newPath = (uint64_t)outPath;
  __syncthreads();
  {
    auto w32 = (__attribute__((address_space(3))) uint32_t*)((wv::Lds)smem + kRootScanJobOff);
    const uint32_t* src = (const uint32_t*)&nj;
#pragma unroll
    for (uint32_t q = 0; q < sizeof(ns::NsJob) / 4; ++q) w32[q] = src[q];
  }
  __syncthreads();
  ns::nodeScan<kRootScanJobOff, kRootScanOutOff>((wv::Lds)smem);
  __syncthreads();
  auto r32 = (__attribute__((address_space(3))) const uint32_t*)((wv::Lds)smem + kRootScanOutOff);
  if (lane < ns::kOutWords) hostStore32(ansDst + lane, r32[lane]);
  if (lane == kTaRootPlannedWord) hostStore32(ansDst + lane, planned);
}

// Workgroup b takes roots b, b + grid, ... of the launch's n_jobs roots.
DEVI void taEpsRootLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  for (uint32_t r = blockIdx.x; r < P.n_jobs; r += gridDim.x) runTaEpsRoot(P, P.jobs + r, smem, arenaSlot, jobS, resS);
}

}  // namespace mrp

#endif  // MRP_LL_TA_EPS_ROOT_H
