// The wide siblings of ll_ta_root.h runTaRoot and ll_ta_eps_root.h runTaEpsRoot (mrp_ll_ta_root_batch_w,
// mrp_ll_ta_eps_root_batch_w): roots of 1 .. kTaRootWideMaxAgents agents, still ONE workgroup (one wave) per root.  Records,
// descriptors, the table's layout, the answer and every fall-back are the narrow runners'; read their headers first.
// What differs is what was one lane per agent there: lane l now keeps agents l + 64 k, k < kTaRootWideGroups, in one
// register per group — arrays indexed by unrolled loops only, never by a run-time value (that would put them in scratch) —
// and every loop over "lane = column" runs once per group.  The narrow runners are left as they are, so the narrow kernels
// keep their code; a root of at most 64 agents gets the same answer from either.
// Ordering as in the narrow runners: every store loop stands in front of the __syncthreads() before the next search's loads.
// Needs ll_ta_root.h and ll_ta_eps_root.h.
#ifndef MRP_LL_TA_ROOT_WIDE_H
#define MRP_LL_TA_ROOT_WIDE_H

#include "ll_ta_eps_root.h"

namespace mrp {

constexpr uint32_t kTaRootWideGroups = kTaRootWideMaxAgents / 64u;
static_assert(kTaRootWideGroups * 64u == kTaRootWideMaxAgents, "whole groups of 64 columns");

// x[a >> 6] of lane a & 63 for a wave-uniform agent a
DEVI uint32_t taRootWideRead(const uint32_t (&x)[kTaRootWideGroups], uint32_t a) {
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTaRootWideGroups; ++k) {
    const uint32_t r = __builtin_amdgcn_readlane(x[k], a & 63u);
    v = (a >> 6) == k ? r : v;
  }
  return v;
}
// x[a >> 6] of lane a & 63 = val
DEVI void taRootWideWrite(uint32_t (&x)[kTaRootWideGroups], uint32_t a, uint32_t val) {
  const uint32_t lane = threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < kTaRootWideGroups; ++k) x[k] = ((a >> 6) == k && lane == (a & 63u)) ? val : x[k];
}

// The root's answer when the device does not scan: `found` (0xFFFFFFFF: no node; kTaRootScanSkipped: the host scans), nine
// zero words, and the number of results filled in.
DEVI void taRootWideAnswer(uint32_t* ansDst, uint32_t found, uint32_t planned) {
  const uint32_t lane = threadIdx.x;
  if (lane <= kTaRootPlannedWord) hostStore32(ansDst + lane, lane == 0 ? found : lane == kTaRootPlannedWord ? planned : 0u);
}
// The scan of a complete table and the answer it gives.  nodeScan's node: the table's columns, and in place of the last
// agent's the path its search left in outPath.
DEVI void taRootWideScan(uint8_t* smem, uint32_t* ansDst, const uint16_t* table, const uint16_t* outPath, uint32_t n, uint32_t npad,
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

DEVI void runTaRootWide(const LaunchParams& P, const DevJob* rootSrc, uint8_t* smem, uint8_t* arenaSlot, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  DevResult res;
  beginJob<true>(rootSrc, jobS, res, 0);
  const uint32_t n = rfl(jobS.n_ctx), base = rfl(jobS.reserved);
  if (n < 1u || n > kTaRootWideMaxAgents) return;  // (the host refuses such a root: nothing is run, nothing written)
  const uint32_t* who = P.cons + rfl(jobS.vc_off);
  int64_t budget = (int64_t)rfl64((uint64_t)jobS.max_expansions);  // < 0: unlimited
  const uint32_t npad = (n + 15u) & ~15u;
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint16_t* table = (uint16_t*)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint32_t* ansDst = (uint32_t*)(P.out_paths + (size_t)base * P.out_host_stride + (P.out_host_stride - kScanOutHalfs));
  uint32_t planned = 0, maxLen = 0, lastLen = 0;
  uint32_t lenL[kTaRootWideGroups] = {}, endL[kTaRootWideGroups] = {};  // lane l, group k: agent l + 64 k's length and last cell
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
      taRootWideWrite(lenL, a, len);
      taRootWideWrite(endL, a, last);
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
    taRootWideAnswer(ansDst, 0xFFFFFFFFu, planned);
    return;
  }
  if (!tableOk) {  // the table does not fit the slot's path area: the host scans the paths it holds
    taRootWideAnswer(ansDst, kTaRootScanSkipped, planned);
    return;
  }
  // every column up to the longest path (rows maxLen x npad fit: the longest path's own test above said so)
  for (uint32_t a = 0; a < n; ++a) {
    const uint32_t la = taRootWideRead(lenL, a), cell = taRootWideRead(endL, a);
    for (uint32_t t = la + lane; t < maxLen; t += 64) table[t * npad + a] = (uint16_t)cell;
  }
  taRootWideScan(smem, ansDst, table, outPath, n, npad, maxLen, lastLen, planned);
}

// ll_ta_eps_root.h's invariant for npad up to 256 — BEFORE EVERY SEARCH every column not yet planned (the searching agent's
// own and the pad columns included) holds kEmptyCell in every row, every planned column is held at its last cell up to the
// longest path so far, and t_pad is that length: runJobTaEps<true> reads whole rows of npad entries.  No path-store variant.
DEVI void runTaEpsRootWide(const LaunchParams& P, const DevJob* rootSrc, uint8_t* smem, uint8_t* arenaSlot, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  DevResult res;
  beginJob<true>(rootSrc, jobS, res, 0);
  const uint32_t n = rfl(jobS.n_ctx), base = rfl(jobS.reserved);
  if (n < 1u || n > kTaRootWideMaxAgents) return;  // (the host refuses such a root: nothing is run, nothing written)
  const uint32_t* who = P.cons + rfl(jobS.vc_off);
  int64_t budget = (int64_t)rfl64((uint64_t)jobS.max_expansions);  // < 0: unlimited
  const uint32_t npad = (n + 15u) & ~15u;  // <= 256: kTaRootWideGroups columns per lane
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint16_t* table = (uint16_t*)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  uint32_t* ansDst = (uint32_t*)(P.out_paths + (size_t)base * P.out_host_stride + (P.out_host_stride - kScanOutHalfs));
  uint32_t planned = 0, maxLen = 0, lastLen = 0;
  uint32_t endL[kTaRootWideGroups];  // lane l, group k: the last cell of agent l + 64 k's path (kEmptyCell: not planned)
#pragma unroll
  for (uint32_t k = 0; k < kTaRootWideGroups; ++k) endL[k] = kEmptyCell;
  bool allOk = true, tableOk = true;
  for (uint32_t a = 0; allOk && tableOk && a < n; ++a) {
    const uint32_t sg = rfl(hostLoad32(who + a * kTaRootAgentWords)), heurOff = rfl(hostLoad32(who + a * kTaRootAgentWords + 1u)),
                   flags = rfl(hostLoad32(who + a * kTaRootAgentWords + 2u));
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
    publishPath(P, outPath, len, (uint32_t*)(P.out_paths + (size_t)(base + a) * P.out_host_stride), [] { return kNoStoreSlot; });
    const uint32_t newMax = len > maxLen ? len : maxLen;
    if (len >= 1u && (uint64_t)newMax * npad * 2u <= (uint64_t)P.arena_paths_bytes) {
      // the rows this path adds, in every group: the planned columns at their last cell, every other column empty (its own
      // comes below)
#pragma unroll
      for (uint32_t k = 0; k < kTaRootWideGroups; ++k) {
        const uint32_t col = lane + 64u * k;
        if (col < npad && col != a)
          for (uint32_t t = maxLen; t < newMax; ++t) table[t * npad + col] = (uint16_t)endL[k];
      }
      const uint32_t last = outPath[len - 1u];  // (all lanes, same address)
      for (uint32_t t = lane; t < newMax; t += 64) table[t * npad + a] = t < len ? outPath[t] : (uint16_t)last;
      taRootWideWrite(endL, a, last);
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
    taRootWideAnswer(ansDst, 0xFFFFFFFFu, planned);
    return;
  }
  if (!tableOk) {  // the table outgrew the slot's path area: the host plans the agents behind `planned` and scans
    taRootWideAnswer(ansDst, kTaRootScanSkipped, planned);
    return;
  }
  taRootWideScan(smem, ansDst, table, outPath, n, npad, maxLen, lastLen, planned);
}

// Workgroup b takes roots b, b + grid, ... of the launch's n_jobs roots.
DEVI void taRootWideLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  for (uint32_t r = blockIdx.x; r < P.n_jobs; r += gridDim.x) runTaRootWide(P, P.jobs + r, smem, arenaSlot, jobS, resS);
}
DEVI void taEpsRootWideLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  for (uint32_t r = blockIdx.x; r < P.n_jobs; r += gridDim.x) runTaEpsRootWide(P, P.jobs + r, smem, arenaSlot, jobS, resS);
}

}  // namespace mrp

#endif  // MRP_LL_TA_ROOT_WIDE_H
