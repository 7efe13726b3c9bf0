// The root node of a CBS-TA or an ECBS-TA conflict tree as ONE workgroup's work (cbs_ta.hpp:142-172, mrp_ll_ta_root_batch;
// ecbs_ta.hpp:117-138, :306-343, mrp_ll_ta_eps_root_batch): the agents of the root are planned in index order, each with no
// constraints, and when every agent has a path the workgroup scans the node for conflicts with ns::nodeScan (for ECBS-TA
// its count is the node's focalHeuristic).  A batch launch that ends: workgroup b takes roots b, b + grid, ...; no queue, no
// polling, nothing shared between workgroups.
// ONE runner, runTaRoot<EPS, GROUPS>, is the source of four kernels (ll_kernel.hip):
//   EPS     false: CBS-TA, each agent by the search an ordinary MRP_LL_ASTAR_TA job runs (runJobTA: the compact tier where
//           the job fits it, the arena tier otherwise); true: ECBS-TA, each by the search an ordinary MRP_LL_ASTAR_EPS_TA job
//           runs (runJobTaEps, arena tier) with the paths of the agents BEFORE it as its focal context.
//   GROUPS  roots of 1 .. 64 * GROUPS agents: 1 for mrp_ll_ta_root_batch / _eps_root_batch, kTaRootWideGroups for the _w
//           calls.  Still one wave per root: lane l keeps agents l + 64 k, k < GROUPS, in one register per group — arrays
//           indexed by unrolled loops only, never by a run-time value (that would put them in scratch) — and every loop over
//           "lane = column" runs once per group.  A root of at most 64 agents gets the same answer from either width.
// What the two algorithms share is written once; what differs — the descriptor, the search, the loop's guard and the
// table's policy — stands under `if constexpr (EPS)`.
// Needs ll_jobs.h (beginJob / endJob, publishPath, hostLoad32 / hostStore32) and ll_ta.h (runJobTA, runJobTaEps<true>).
//
// The root's record is a DevJob (ll_device.h kTaRootAgentWords): map, budget, n_ctx = agents, reserved = the root's first
// result, vc_off = its agent words; for ECBS-TA with algo MRP_LL_ASTAR_EPS_TA and w.  The per-agent descriptor is made from
// it in the window's job block: start, goal, table offset and the no-task flag come from the agent's three words,
// max_expansions is what the searches before left, and n_ctx / reserved are cleared (ll_device.h taRootAgentJob and
// taEpsRootAgentJob, one function each for this kernel and for the check) — word for word the descriptor host/ll_pack.h
// packJob makes for the ordinary job, except ECBS-TA's path_off: the table is not shipped.
//
// The node's solution is kept as a time-major table [rows][npad] (x | y << 8, npad = agents rounded up to 16) in the slot's
// path area, which no task-assignment search touches: a column per path, appended behind its search, every column held at
// its last cell up to the longest path once all are there.  The table is written and read by this one wave with plain
// stores and loads — lanes read what other lanes of the wave stored.  The statement the project holds for that is ll_jobs.h
// runChain's ordering rule (a wave's vector-memory operations reach its CU's L1 in program order and that cache writes
// through), and the precedent is ll_kernel.hip scanNode: stageFocalTable builds a table in this same path area with plain
// stores, lane = agent, and ns::nodeScan reads it back with the plain loads of nsRow, lane = another agent.  (wave_dev.h's
// note at gLoad32Coherent is about the path STORE, whose slots other workgroups wrote: that is the case an agent-scope load
// is for.)  A path whose rows x npad x 2 bytes exceed the area ends the table: the searches go on, the scan is left to the
// host (found = kTaRootScanSkipped).
//
// ECBS-TA: that ONE table is both the focal context of the next search and the scan's input.  runJobTaEps<true> takes it
// where it lies (the ordinary job copies its shipped table into this very area).  The search loads a whole row for every
// lane < npad (GROUPS > 1: whole rows of npad entries) and repeats row t_pad - 1 beyond the table, so
// BEFORE EVERY SEARCH: every column not yet planned — the searching agent's own and the pad columns
// included — holds kEmptyCell in every row, every planned column is held at its last cell up to the longest path so far,
// and t_pad is that length.  A path longer than all before it therefore extends the rows first (planned columns at their
// last cell, the others empty), then its own column is written.  Agent 0 searches with no table at all (n_agents_pad = 0),
// as its ordinary job does.
// CBS-TA's searches do not read the table, so it only writes each column, and fills every column up to the longest path
// once, in front of the scan.  (It is not moved onto ECBS-TA's policy: that would add stores to its kernels.)
// Ordering: every store loop to the table stands in front of the __syncthreads() that precedes the next search's loads.
// An ECBS-TA table that would outgrow the path area (only under MRP_LL_ARENA_PATHS_BYTES) ends the kernel's part behind the
// agent whose path did not fit: the answer says kTaRootScanSkipped and how many agents are planned, the host runs the rest.
// mrp_ll_ta_eps_root_batch_stored: cons[ec_off + a] names the path-store slot that also receives agent a's path
// (publishPath, as an ordinary job with MRP_LL_JOB_STORE_RESULT); the slot of an agent the root did not plan is not touched.
// Every other record has ec_off == vc_off (ll_device.h): the host supplies slots for the narrow ECBS-TA call alone, and
// only runTaRoot<true, 1> reads them.
#ifndef MRP_LL_TA_ROOT_H
#define MRP_LL_TA_ROOT_H

#include "ll_node_scan.h"

namespace mrp {

// the scan's job and answer in the window's control block, behind the job descriptor and the result record (the blocks
// scanNode uses, ll_kernel.hip)
constexpr uint32_t kRootScanJobOff = ct::oCtl + sizeof(DevJob) + sizeof(DevResult), kRootScanOutOff = kRootScanJobOff + sizeof(ns::NsJob);
static_assert(kRootScanJobOff % 8 == 0 && kRootScanOutOff + ns::kOutWords * 4u <= ct::oJob, "the scan's blocks fit the control block");
static_assert(ns::kOutWords == kTaRootPlannedWord && (kTaRootPlannedWord + 1u) * 2u <= kScanOutHalfs, "the root's answer fits its area");

constexpr uint32_t kTaRootWideGroups = kTaRootWideMaxAgents / 64u;
static_assert(kTaRootMaxAgents == 64u && kTaRootWideGroups * 64u == kTaRootWideMaxAgents, "whole groups of 64 columns");

// x[a >> 6] of lane a & 63 for a wave-uniform agent a
template <uint32_t GROUPS>
DEVI uint32_t taRootLaneRead(const uint32_t (&x)[GROUPS], uint32_t a) {
  if constexpr (GROUPS == 1) {
    return __builtin_amdgcn_readlane(x[0], a);
  } else {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < GROUPS; ++k) {
      const uint32_t r = __builtin_amdgcn_readlane(x[k], a & 63u);
      v = (a >> 6) == k ? r : v;
    }
    return v;
  }
}
// x[a >> 6] of lane a & 63 = val
template <uint32_t GROUPS>
DEVI void taRootLaneWrite(uint32_t (&x)[GROUPS], uint32_t a, uint32_t val) {
  const uint32_t lane = threadIdx.x;
  if constexpr (GROUPS == 1) {
    x[0] = lane == a ? val : x[0];
  } else {
#pragma unroll
    for (uint32_t k = 0; k < GROUPS; ++k) x[k] = ((a >> 6) == k && lane == (a & 63u)) ? val : x[k];
  }
}

// The root's answer when the device does not scan: `found` (0xFFFFFFFF: no node; kTaRootScanSkipped: the host scans), nine
// zero words, and the number of results filled in.
DEVI void taRootAnswer(uint32_t* ansDst, uint32_t found, uint32_t planned) {
  const uint32_t lane = threadIdx.x;
  if (lane <= kTaRootPlannedWord) hostStore32(ansDst + lane, lane == 0 ? found : lane == kTaRootPlannedWord ? planned : 0u);
}
// The scan of a complete table and the answer it gives: ten words of an mrp_ll_conflict, then the number of results filled
// in.  nodeScan's node: the table's columns, and in place of the last agent's the path its search left in outPath.
DEVI void taRootScan(uint8_t* smem, uint32_t* ansDst, const uint16_t* table, const uint16_t* outPath, uint32_t n, uint32_t npad,
                     uint32_t maxLen, uint32_t lastLen, uint32_t planned) {
  const uint32_t lane = threadIdx.x;
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

template <bool EPS, uint32_t GROUPS>
DEVI void runTaRoot(const LaunchParams& P, const DevJob* rootSrc, uint8_t* smem, uint8_t* arenaSlot, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  DevResult res;
  beginJob<true>(rootSrc, jobS, res, 0);
  const uint32_t n = rfl(jobS.n_ctx), base = rfl(jobS.reserved);
  if (n < 1u || n > 64u * GROUPS) return;  // (the host refuses such a root: nothing is run, nothing written)
  const uint32_t* who = P.cons + rfl(jobS.vc_off);
  // (ll_device.h; the narrow ECBS-TA call alone has a stored variant: without `GROUPS == 1` the wide kernel would carry
  // publishPath's store branch — 81 instructions, ten SGPR spills — for words the host never gives it)
  const uint32_t* storeIds = EPS && GROUPS == 1 && rfl(jobS.ec_off) != rfl(jobS.vc_off) ? P.cons + rfl(jobS.ec_off) : nullptr;
  int64_t budget = (int64_t)rfl64((uint64_t)jobS.max_expansions);  // < 0: unlimited
  const uint32_t npad = (n + 15u) & ~15u;  // <= 64 * GROUPS: GROUPS columns per lane
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint16_t* table = (uint16_t*)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint32_t* ansDst = (uint32_t*)(P.out_paths + (size_t)base * P.out_host_stride + (P.out_host_stride - kScanOutHalfs));
  uint32_t planned = 0, maxLen = 0, lastLen = 0;
  // lane l, group k: the length of agent l + 64 k's path (CBS-TA alone) and its last cell (ECBS-TA: kEmptyCell: not planned).
  // (Both start from = {}: an init loop in its place reorders the CBS-TA kernels' code.)
  uint32_t lenL[GROUPS] = {}, endL[GROUPS] = {};
  if constexpr (EPS) {
#pragma unroll
    for (uint32_t k = 0; k < GROUPS; ++k) endL[k] = kEmptyCell;
  }
  bool allOk = true, tableOk = true;
  // CBS-TA goes on searching after the table stopped fitting; ECBS-TA, whose searches read it, stops there
  for (uint32_t a = 0; allOk && (!EPS || tableOk) && a < n; ++a) {
    const uint32_t sg = rfl(hostLoad32(who + a * kTaRootAgentWords)), heurOff = rfl(hostLoad32(who + a * kTaRootAgentWords + 1u)),
                   flags = rfl(hostLoad32(who + a * kTaRootAgentWords + 2u));
    const uint32_t storeId = storeIds ? rfl(hostLoad32(storeIds + a)) : kNoStoreSlot;  // kNoStoreSlot: the path goes to the host only
    __syncthreads();
    // (every lane stores the same words)
    if constexpr (EPS) taEpsRootAgentJob(jobS, sg, heurOff, flags, budget, a ? npad : 0u, a ? maxLen : 0u);
    else taRootAgentJob(jobS, sg, heurOff, flags, budget);
    __syncthreads();
    if constexpr (EPS) {
      runJobTaEps<true>(&jobS, &resS, arenaSlot, P.maps, P.cons, P.paths, P.arena_scratch_off, P.out_stride, P.arena_nodes,
                        P.arena_rows, P.arena_row_words, P.arena_paths_bytes, P.path_store, P.path_store_stride, P.path_store_slots);
      __syncthreads();
      res.status = rfli(resS.status); res.cost = rfli(resS.cost); res.fmin = rfli(resS.fmin);
      res.n_states = rfli(resS.n_states);
      res.expanded = (int64_t)rfl64((uint64_t)resS.expanded);
      res.nodes_created = rfl(resS.nodes_created);
      res.tier = rfl(resS.tier);
      for (int q = 0; q < 8; ++q) res.prof[q] = 0;
    } else {
      res.status = ST_BAD; res.cost = 0; res.fmin = 0; res.n_states = 0; res.expanded = 0; res.nodes_created = 0; res.tier = 0;
      for (int q = 0; q < 8; ++q) res.prof[q] = 0;
      runJobTA(P, jobS, smem, arenaSlot, res, outPath);
    }
    endJob(res, resS, P.results + base + a);
    planned += 1;
    if (rfl((uint32_t)res.status) != (uint32_t)ST_OK) {  // no path / budget / capacity: the root ends behind this agent
      allOk = false;
      break;
    }
    const uint32_t len = rfl((uint32_t)res.n_states);
    publishPath(P, outPath, len, (uint32_t*)(P.out_paths + (size_t)(base + a) * P.out_host_stride), [&] { return storeId; });
    if constexpr (EPS) {
      const uint32_t newMax = len > maxLen ? len : maxLen;
      if (len >= 1u && (uint64_t)newMax * npad * 2u <= (uint64_t)P.arena_paths_bytes) {
        // the rows this path adds, in every group: the planned columns at their last cell, every other column empty (its own
        // comes below)
#pragma unroll
        for (uint32_t k = 0; k < GROUPS; ++k) {
          const uint32_t col = lane + 64u * k;
          if (col < npad && col != a)
            for (uint32_t t = maxLen; t < newMax; ++t) table[t * npad + col] = (uint16_t)endL[k];
        }
        const uint32_t last = outPath[len - 1u];  // (all lanes, same address)
        for (uint32_t t = lane; t < newMax; t += 64) table[t * npad + a] = t < len ? outPath[t] : (uint16_t)last;
        taRootLaneWrite(endL, a, last);
        maxLen = newMax;
      } else {
        tableOk = false;
      }
    } else {
      if (tableOk && len >= 1u && (uint64_t)len * npad * 2u <= (uint64_t)P.arena_paths_bytes) {
        for (uint32_t t = lane; t < len; t += 64) table[t * npad + a] = outPath[t];
        const uint32_t last = outPath[len - 1u];  // (all lanes, same address)
        taRootLaneWrite(lenL, a, len);
        taRootLaneWrite(endL, a, last);
      } else {
        tableOk = false;
      }
      maxLen = len > maxLen ? len : maxLen;
    }
    lastLen = len;
    if (budget >= 0) {
      const int64_t expanded = (int64_t)rfl64((uint64_t)res.expanded);
      budget = budget > expanded ? budget - expanded : 0;
    }
  }
  __syncthreads();
  // no node: found = -1, the rest 0.  (CBS-TA leaves its loop with allOk only behind the last agent; the compare is the
  // narrow runner's of old and keeps its kernels' code)
  if (!(allOk && (EPS || planned == n))) {
    taRootAnswer(ansDst, 0xFFFFFFFFu, planned);
    return;
  }
  // the table does not fit the slot's path area.  CBS-TA: every agent is planned, the host scans the paths it holds;
  // ECBS-TA: the host plans the agents behind `planned` and scans
  if (!tableOk) {
    taRootAnswer(ansDst, kTaRootScanSkipped, planned);
    return;
  }
  if constexpr (!EPS) {
    // every column up to the longest path (rows maxLen x npad fit: the longest path's own test above said so)
    for (uint32_t a = 0; a < n; ++a) {
      const uint32_t la = taRootLaneRead(lenL, a), cell = taRootLaneRead(endL, a);
      for (uint32_t t = la + lane; t < maxLen; t += 64) table[t * npad + a] = (uint16_t)cell;
    }
  }
  taRootScan(smem, ansDst, table, outPath, n, npad, maxLen, lastLen, planned);
}

// Workgroup b takes roots b, b + grid, ... of the launch's n_jobs roots.
template <bool EPS, uint32_t GROUPS>
DEVI void taRootLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  for (uint32_t r = blockIdx.x; r < P.n_jobs; r += gridDim.x) runTaRoot<EPS, GROUPS>(P, P.jobs + r, smem, arenaSlot, jobS, resS);
}

}  // namespace mrp

#endif  // MRP_LL_TA_ROOT_H
