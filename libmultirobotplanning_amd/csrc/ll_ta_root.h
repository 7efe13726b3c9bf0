// The root node of a CBS-TA conflict tree as ONE workgroup's work (cbs_ta.hpp:142-172; mrp_ll_ta_root_batch): the agents of
// the root are planned in index order, each with no constraints, each by the search an ordinary MRP_LL_ASTAR_TA job runs
// (runJobTA: the compact tier where the job fits it, the arena tier otherwise), and when every agent has a path the
// workgroup scans the node for conflicts with ns::nodeScan.  A batch launch that ends: workgroup b takes roots b, b + grid,
// ...; no queue, no polling, nothing shared between workgroups.
// Needs ll_jobs.h (beginJob / endJob, publishPath, hostLoad32 / hostStore32) and ll_ta.h (runJobTA).
//
// The root's record is a DevJob (ll_device.h kTaRootAgentWords): map, budget, n_ctx = agents, reserved = the root's first
// result, vc_off = its agent words.  The per-agent descriptor is made from it in the window's job block: start, goal, table
// offset and the no-task flag come from the agent's three words, max_expansions is what the searches before left, and
// n_ctx / reserved are cleared (ll_device.h taRootAgentJob, one function for this kernel and for the check) — word for word
// the descriptor host/ll_pack.h packJob makes for the ordinary job.
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
#ifndef MRP_LL_TA_ROOT_H
#define MRP_LL_TA_ROOT_H

#include "ll_node_scan.h"

namespace mrp {

// the scan's job and answer in the window's control block, behind the job descriptor and the result record (the blocks
// scanNode uses, ll_kernel.hip)
constexpr uint32_t kRootScanJobOff = ct::oCtl + sizeof(DevJob) + sizeof(DevResult), kRootScanOutOff = kRootScanJobOff + sizeof(ns::NsJob);
static_assert(kRootScanJobOff % 8 == 0 && kRootScanOutOff + ns::kOutWords * 4u <= ct::oJob, "the scan's blocks fit the control block");
static_assert(ns::kOutWords == kTaRootPlannedWord && (kTaRootPlannedWord + 1u) * 2u <= kScanOutHalfs, "the root's answer fits its area");

DEVI void runTaRoot(const LaunchParams& P, const DevJob* rootSrc, uint8_t* smem, uint8_t* arenaSlot, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  DevResult res;
  beginJob<true>(rootSrc, jobS, res, 0);
  const uint32_t n = rfl(jobS.n_ctx), base = rfl(jobS.reserved);
  if (n < 1u || n > kTaRootMaxAgents) return;  // (the host refuses such a root: nothing is run, nothing written)
  const uint32_t* who = P.cons + rfl(jobS.vc_off);
  int64_t budget = (int64_t)rfl64((uint64_t)jobS.max_expansions);  // < 0: unlimited
  const uint32_t npad = (n + 15u) & ~15u;
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint16_t* table = (uint16_t*)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  // the root's answer: ten words of an mrp_ll_conflict, then the number of results filled in
  uint32_t* ansDst = (uint32_t*)(P.out_paths + (size_t)base * P.out_host_stride + (P.out_host_stride - kScanOutHalfs));
  uint32_t planned = 0, maxLen = 0, lastLen = 0;
  uint32_t lenL = 0, endL = 0;  // lane a: the length of agent a's path and its last cell
  bool allOk = true, tableOk = true;
  for (uint32_t a = 0; allOk && a < n; ++a) {
    const uint32_t sg = rfl(hostLoad32(who + a * kTaRootAgentWords)), heurOff = rfl(hostLoad32(who + a * kTaRootAgentWords + 1u)),
                   flags = rfl(hostLoad32(who + a * kTaRootAgentWords + 2u));
    __syncthreads();
    taRootAgentJob(jobS, sg, heurOff, flags, budget);  // (every lane stores the same words)
    __syncthreads();
    res.status = ST_BAD; res.cost = 0; res.fmin = 0; res.n_states = 0; res.expanded = 0; res.nodes_created = 0; res.tier = 0;
    for (int q = 0; q < 8; ++q) res.prof[q] = 0;
    runJobTA(P, jobS, smem, arenaSlot, res, outPath);
    endJob(res, resS, P.results + base + a);
    planned += 1;
    if (rfl((uint32_t)res.status) != (uint32_t)ST_OK) {  // no path / budget / capacity: the root ends behind this agent
      allOk = false;
      break;
    }
    const uint32_t len = rfl((uint32_t)res.n_states);
    publishPath(P, outPath, len, (uint32_t*)(P.out_paths + (size_t)(base + a) * P.out_host_stride), [] { return kNoStoreSlot; });
    if (tableOk && len >= 1u && (uint64_t)len * npad * 2u <= (uint64_t)P.arena_paths_bytes) {
      for (uint32_t t = lane; t < len; t += 64) table[t * npad + a] = outPath[t];
      const uint32_t last = outPath[len - 1u];  // (all lanes, same address)
      lenL = lane == a ? len : lenL;
      endL = lane == a ? last : endL;
    } else {
      tableOk = false;
    }
    maxLen = len > maxLen ? len : maxLen;
    lastLen = len;
    if (budget >= 0) {
      const int64_t expanded = (int64_t)rfl64((uint64_t)res.expanded);
      budget = budget > expanded ? budget - expanded : 0;
    }
  }
  __syncthreads();
  if (!(allOk && planned == n)) {  // no node: found = -1, the rest 0
    if (lane <= kTaRootPlannedWord) hostStore32(ansDst + lane, lane == 0 ? 0xFFFFFFFFu : lane == kTaRootPlannedWord ? planned : 0u);
    return;
  }
  if (!tableOk) {  // the table does not fit the slot's path area: the host scans the paths it holds
    if (lane <= kTaRootPlannedWord) hostStore32(ansDst + lane, lane == 0 ? kTaRootScanSkipped : lane == kTaRootPlannedWord ? planned : 0u);
    return;
  }
  for (uint32_t a = 0; a < n; ++a) {  // every column up to the longest path
    const uint32_t la = __builtin_amdgcn_readlane(lenL, a), cell = __builtin_amdgcn_readlane(endL, a);
    for (uint32_t t = la + lane; t < maxLen; t += 64) table[t * npad + a] = (uint16_t)cell;
  }
  // nodeScan's node: the table's columns, and in place of the last agent's the path its search left in outPath
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
DEVI void taRootLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  for (uint32_t r = blockIdx.x; r < P.n_jobs; r += gridDim.x) runTaRoot(P, P.jobs + r, smem, arenaSlot, jobS, resS);
}

}  // namespace mrp

#endif  // MRP_LL_TA_ROOT_H
