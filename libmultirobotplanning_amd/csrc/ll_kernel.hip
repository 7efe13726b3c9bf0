// Low-level space-time searches of CBS / ECBS, their task-assignment variants and SIPP as hand-written HIP for gfx950
// (MI355X, CDNA4): the kernels, their job loops and the host-callable launchers.
//
// One 64-lane wavefront (== one workgroup) runs ONE low-level search at a time: a batch kernel pulls jobs from the batch's
// queue until it is empty, a resident kernel is fed through a host job ring for a whole session.  Inside a search the
// reference's sequential semantics are replayed verbatim — the results of A*-epsilon depend on the tie order of
// boost::heap::d_ary_heap — so the open list, the focal list and the ordered walk are exact array-heap
// emulations executed wave-uniformly (scalar control flow), while the 64 lanes do everything whose order cannot be
// observed: the successor probes, the O(N) focal heuristics, lazy bitmap rows, and the data-independent part of every
// heap operation.
// A CBS / ECBS search starts in the compact tier (ll_compact.h: the whole search in LDS, a state is its 32-bit heap
// entry); one that outgrows it is run again from the start in the arena tier, with its state in this workgroup's slot of a
// global-memory arena and the heaps' top levels in LDS.  This translation unit is split by subject; the headers are
// included once, here, in dependency order:
//   ll_slot.h          the arena slot's layout: sizes and scratch areas (also the host's, mrp_ll_create)
//   ll_compact.h       the compact tier (also compiled for the CPU emulator of the tests)
//   ll_compact_ta_eps.h  the LDS tier of MRP_LL_ASTAR_EPS_TA, in the same vocabulary and window (likewise)
//   ll_arena_heap.h    tiers, Mem views, the exact heap emulations, PushChains, the ordered walk
//   ll_arena_search.h  ensureRows, initSearch, runSearch: the CBS / ECBS search of the arena tier
//   ll_jobs.h          job staging and bracket, the arena slot's cut, baseCJob, runJob (stageFocalTable, compactAttempt,
//                      arenaAttempt), publishPath and runChain (ECBS root chains)
//   ll_ta.h            TaEnv, runTaArena / runJobTA, runJobTaEps, runTaEpsLds: the task-assignment low levels
//   ll_ta_root.h       runTaRoot<EPS, GROUPS>, taRootLoop: the root node of a CBS-TA or an ECBS-TA conflict tree, searches
//                      and scan, by one workgroup; roots of up to 64 agents, or up to 256 with four agents per lane
//   ll_sipp.h          SIPP: its tiers, sippLoop, runSipp, processSippJob
//   ll_node_scan.h     nodeScan, nodeScanFromParent: the conflicts of the conflict-tree node a search has completed (also
//                      compiled for the CPU)
//   here               scanNode, processJob, batchLoop, publishDone, residentLoop, the twelve kernels, the launchers
//
// Reference semantics implemented (file:line in the reference project, libMultiRobotPlanning):
//   AStarEpsilon::search   include/libMultiRobotPlanning/a_star_epsilon.hpp:86-285
//   AStar::search          include/libMultiRobotPlanning/a_star.hpp:63-161
//   Environment (grid)     example/ecbs.cpp:264-312,352-399,497-510  (example/cbs.cpp identical minus focal parts)
//   heap rules             boost::heap::d_ary_heap<arity<2>, mutable_<true>> as restated in oracle/heap_restated.hpp
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "ll_device.h"
#include "ll_slot.h"
#include "ll_launch.h"
#include "wave_dev.h"
#include "ll_compact.h"
#include "ll_compact_ta_eps.h"

#include "ll_arena_heap.h"
#include "ll_arena_search.h"
#include "ll_jobs.h"
#include "ll_ta.h"
#include "ll_ta_root.h"
#include "ll_sipp.h"
#include "ll_node_scan.h"

namespace mrp {

// The conflicts of the conflict-tree node this workgroup has just completed (ll_device.h kCtxScan): the focal table runJob
// built from the path store is still where it was — the searches only read it, the compact tier works in the window in
// front of it and the arena tier keeps its heap tops inside that window — and outPath holds the new path.  The scan
// (ll_node_scan.h: a function of its own, so that it does not take part in this kernel's register allocation) finds its
// job in the window's control block, behind the job descriptor and the result record, and leaves its answer behind that:
// the one part of the window every launch has, also one without the compact tier.
constexpr uint32_t kScanJobOff = ct::oCtl + sizeof(DevJob) + sizeof(DevResult), kScanOutOff = kScanJobOff + sizeof(ns::NsJob);
// A kCtxScanParent job (mrp_ll_submit_node) scans from what the caller knows of the parent node: that block lies ON the
// result record's staging block, which only endJob uses, behind the scan (MRP_LL_ASTAR_EPS_TA reads it back in front of it).
constexpr uint32_t kScanBaseOff = ct::oCtl + sizeof(DevJob);
static_assert(kScanJobOff % 8 == 0 && kScanOutOff + ns::kOutWords * 4u <= ct::oJob && kScanBaseOff % 8 == 0 &&
                  sizeof(ns::NsBase) <= sizeof(DevResult),
              "the scan's blocks fit the control block");
// The scan of a kCtxScanParent job, behind scanNode's staging of the NsJob.  `words`: the three staged words behind the
// context's ids (ll_device.h) — the replaced path's slot, the parent's conflict count, the time before which it has none.
// A slot the store does not have gets the full scan.  A function of its own, with plain values for arguments, so that the
// kernels' code in front of the call is what it is without it.
__device__ __attribute__((noinline)) void scanNodeFromParent(uint8_t* smem, const uint32_t* words, const uint16_t* store,
                                                              uint32_t storeStride, uint32_t storeSlots) {
  const uint32_t sid = rfl(hostLoad32(words));
  const uint64_t oldSlot = (uint64_t)(store + (size_t)(sid < storeSlots ? sid : 0u) * storeStride);
  const uint32_t parentCount = rfl(hostLoad32(words + 1)), cleanBefore = rfl(hostLoad32(words + 2));
  auto nb = (__attribute__((address_space(3))) uint32_t*)((wv::Lds)smem + kScanBaseOff);  // the NsBase, word by word
  static_assert(offsetof(ns::NsBase, oldSlot) == 0 && offsetof(ns::NsBase, oldCap) == 8 && offsetof(ns::NsBase, parentCount) == 12 &&
                    offsetof(ns::NsBase, cleanBefore) == 16 && sizeof(ns::NsBase) == 24, "NsBase as written here");
  nb[0] = (uint32_t)oldSlot;
  nb[1] = (uint32_t)(oldSlot >> 32);
  nb[2] = storeStride - 1u;
  nb[3] = parentCount;
  nb[4] = cleanBefore;
  nb[5] = 0u;
  __syncthreads();
  if (sid < storeSlots && storeStride != 0u)
    ns::nodeScanFromParent<kScanJobOff, kScanOutOff, kScanBaseOff>((wv::Lds)smem);
  else
    ns::nodeScan<kScanJobOff, kScanOutOff>((wv::Lds)smem);
}
template <bool BG, int TIERS>
DEVI void scanNode(const LaunchParams& P, const DevJob& J, uint8_t* smem, uint8_t* arenaSlot, int32_t status, uint32_t nStates,
                   const uint16_t* outPath, uint16_t* pathDst) {
  typedef typename std::conditional<TIERS == kTiersHeavy, ct::Wide, ct::Narrow>::type Geo;
  const uint32_t lane = threadIdx.x;
  uint32_t* dst = (uint32_t*)(pathDst + (P.out_host_stride - kScanOutHalfs));
  if (status != ST_OK || nStates == 0u) {
    if (lane < ns::kOutWords) hostStore32(dst + lane, lane == 0 ? 0xFFFFFFFFu : 0u);
    return;
  }
  const bool byId = (J.ctx_flags & kCtxById) != 0;
  const uint32_t pathBytes = J.t_pad * J.n_agents_pad * 2;
  const bool inLds = idTableInLds<TIERS>(P, pathBytes);
  ns::NsJob nj;
  nj.nAgents = byId ? J.n_ctx : 1u;
  nj.nPad = J.n_agents_pad; nj.tPad = J.t_pad;
  nj.agentIdx = J.reserved;
  nj.nStates = nStates;
  nj.tabLds = inLds ? Geo::windowBytes(BG) : ns::kTableInGlobal;
  nj.tabG = (uint64_t)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  nj.newPath = (uint64_t)outPath;
  __syncthreads();
  {
    auto w32 = (__attribute__((address_space(3))) uint32_t*)((wv::Lds)smem + kScanJobOff);
    const uint32_t* src = (const uint32_t*)&nj;
#pragma unroll
    for (uint32_t q = 0; q < sizeof(ns::NsJob) / 4; ++q) w32[q] = src[q];
  }
  __syncthreads();
  if (byId && (J.ctx_flags & kCtxScanParent))
    scanNodeFromParent(smem, P.cons + J.path_off + J.n_ctx, P.path_store, P.path_store_stride, P.path_store_slots);
  else
    ns::nodeScan<kScanJobOff, kScanOutOff>((wv::Lds)smem);
  __syncthreads();
  auto r32 = (__attribute__((address_space(3))) const uint32_t*)((wv::Lds)smem + kScanOutOff);
  if (lane < ns::kOutWords) hostStore32(dst + lane, r32[lane]);
}

// Runs the job whose descriptor is at `jobSrc` (host memory) and writes result + path to host memory.
// KIND: 0 = the job's own algo field decides (mixed batches / sessions), 1 = A*-epsilon jobs only (ECBS), 2 = A* jobs
// only (CBS).  The specialised kernels carry one search loop per memory tier instead of two, which halves their code
// (instruction-cache footprint) and takes the other algorithm's live ranges out of the register allocation; a job of
// the other kind comes back as ST_BAD.
// Returns true when the job was NOT run here and has to be handed to the heavy workgroups (TIERS == kTiersFront only):
// nothing has been written to the job's result area then.
template <int KIND, int TIERS = kTiersAll>
DEVI bool processJob(const LaunchParams& P, const DevJob* jobSrc, DevResult* resDst, uint16_t* pathDst, uint8_t* smem,
                     uint8_t* arenaSlot, DevJob& jobS, DevResult& resS) {
  static_assert(TIERS == kTiersAll || KIND == 1, "front / heavy workgroups exist for the A*-epsilon sessions");
  const DevJob& J = jobS;
  DevResult res;
  beginJob<true>(jobSrc, jobS, res, 0);
  PROF_T0();
#ifndef MRP_LL_TRACE
  const uint64_t tj0 = __builtin_amdgcn_s_memrealtime();
#endif
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);  // device scratch; copied out below
  uint32_t algo = rfl(J.algo);
  bool handOver = false;
  // A job that names its constraint set in the device store (ll_device.h DevJob::pad_): the union goes into the arena slot's
  // copy area — and into the result slot — here, in front of runJob; a descriptor that does not fit stays ST_BAD.  (Not in a
  // front workgroup that hands the search over unseen: the heavy workgroup that runs it stages, and writes the result slot.)
  if ((rfl(J.pad_[0]) | rfl(J.pad_[2])) != 0u && !(TIERS == kTiersFront && frontHandsOver(P, J))) {
    if (algo > 1u || (rfl(J.ctx_flags) & kCtxChain) ||
        !stageConstraintSet(&jobS, P.cons, P.cons_store, P.cons_store_stride, P.cons_store_slots,
                            slot::consCopy(arenaSlot, P.arena_scratch_off, P.out_stride)))
      algo = 0xFFFFFFFFu;  // no search below takes it
  }
  if constexpr (KIND == 0) {
    // MRP_LL_JOB_TABLE_H: the arena tier with h from the goal's table.  (Its algo word is kAlgoTableH | algo: the
    // one-algorithm kernels below take no such job and leave it ST_BAD without a test of their own.)
    if ((algo & ~1u) == kAlgoTableH && (rfl(J.ctx_flags) & kCtxTableH)) {
      if (algo & 1u)
        runJobTableH<true>(&jobS, &resS, smem, arenaSlot, P.maps, P.cons, P.paths, P.arena_scratch_off, P.out_stride, P.arena_nodes,
                           P.arena_rows, P.arena_row_words, P.arena_paths_bytes, P.lds_nodes, P.lds_paths_bytes);
      else
        runJobTableH<false>(&jobS, &resS, smem, arenaSlot, P.maps, P.cons, P.paths, P.arena_scratch_off, P.out_stride, P.arena_nodes,
                            P.arena_rows, P.arena_row_words, P.arena_paths_bytes, P.lds_nodes, P.lds_paths_bytes);
      __syncthreads();
      res.status = rfli(resS.status); res.cost = rfli(resS.cost); res.fmin = rfli(resS.fmin);
      res.n_states = rfli(resS.n_states);
      res.expanded = (int64_t)rfl64((uint64_t)resS.expanded);
      res.nodes_created = rfl(resS.nodes_created);
      res.tier = rfl(resS.tier);
      for (int q = 0; q < 8; ++q) res.prof[q] = rfl(resS.prof[q]);  // the tiers' ticks and expansions (compactAttempt, arenaAttempt)
    } else if (algo == 1)
      runJob<true, false, kTiersAll>(P, J, smem, arenaSlot, res, outPath);
    else if (algo == 3)
      runJobTA(P, J, smem, arenaSlot, res, outPath);
    else if (algo == 4 && (rfl(J.ctx_flags) & kCtxTryLds) && runTaEpsLds(P, J, smem, arenaSlot, res, outPath)) {
      // MRP_LL_ASTAR_EPS_TA with MRP_LL_JOB_TRY_LDS: answered in the LDS tier
    } else if (algo == 4) {  // MRP_LL_ASTAR_EPS_TA: the arena tier; the result comes back through the staging record
      const uint64_t th0 = __builtin_amdgcn_s_memrealtime();
      runJobTaEps<false>(&jobS, &resS, arenaSlot, P.maps, P.cons, P.paths, P.arena_scratch_off, P.out_stride, P.arena_nodes,
                  P.arena_rows, P.arena_row_words, P.arena_paths_bytes, P.path_store, P.path_store_stride, P.path_store_slots);
      __syncthreads();
      res.status = rfli(resS.status); res.cost = rfli(resS.cost); res.fmin = rfli(resS.fmin);
      res.n_states = rfli(resS.n_states);
      res.expanded = (int64_t)rfl64((uint64_t)resS.expanded);
      res.nodes_created = rfl(resS.nodes_created);
      res.tier = rfl(resS.tier);
      res.prof[2] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - th0);
      res.prof[3] = (uint32_t)res.expanded;
    } else if (algo == 0)
      runJob<false, false, kTiersAll>(P, J, smem, arenaSlot, res, outPath);
  } else if constexpr (KIND == 1) {  // the A*-epsilon-only kernels: the small window (mrp_ll_lds_bytes(kind = 1))
    if (algo == 1) {
      if (rfl(J.ctx_flags) & kCtxChain) {
        if constexpr (TIERS != kTiersHeavy) runChain(P, J, smem, arenaSlot, res, outPath, pathDst);  // (heavy: stays ST_BAD)
      } else {
        handOver = runJob<true, true, TIERS>(P, J, smem, arenaSlot, res, outPath);
      }
    }
  } else {
    if (algo == 0) runJob<false, false, kTiersAll>(P, J, smem, arenaSlot, res, outPath);
    if (algo == 3) runJobTA(P, J, smem, arenaSlot, res, outPath);
  }
  if (TIERS == kTiersFront && handOver) return true;
  if constexpr (KIND != 2) {
    if (rfl(J.ctx_flags) & kCtxScan)
      scanNode<KIND == 1, TIERS>(P, J, smem, arenaSlot, (int32_t)rfl((uint32_t)res.status), rfl((uint32_t)res.n_states), outPath, pathDst);
  }
  PROF_ADD(res, 5);
#if !defined(MRP_LL_TRACE) && !defined(MRP_CT_PROF)
  res.prof[4] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tj0);  // the whole job on the device (tables, search)
  res.prof[5] = 1;
#endif
  DBG(P, 2, res.status + 100);
  endJob(res, resS, resDst);
  if (res.status == ST_OK && !(KIND == 1 && (rfl(J.ctx_flags) & kCtxChain)))  // (a root chain wrote its own output)
    publishPath(P, outPath, (uint32_t)res.n_states, (uint32_t*)pathDst, [&] { return rfl(J.store_out_id); });
  return false;
}

// Batch mode.  One workgroup == one wavefront; pulls jobs from the batch's queue (exit: queue exhausted).
// The CBS / ECBS kernels declare NO static LDS: their dynamic window then starts at LDS address 0, which is what makes
// every address inside ll_compact.h's window a constant of the ds_ instructions (wave_dev.h windowBase).  The job
// descriptor and the result record they stage through LDS live in the window's control block instead.
static_assert(sizeof(DevJob) + sizeof(DevResult) <= ct::oJob, "control block of the window");
#define MRP_LL_WINDOW_BLOCKS(smem, jobS, resS)                                                        \
  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem != 0u) __builtin_trap(); \
  DevJob& jobS = *(DevJob*)(smem + ct::oCtl);                                                         \
  DevResult& resS = *(DevResult*)(smem + ct::oCtl + sizeof(DevJob))
// A kernel whose whole body is one job loop on the window's blocks
#define MRP_LL_WINDOW_KERNEL_PRE(NAME, PRE, ...)                                         \
  extern "C" __global__ void __launch_bounds__(64) NAME(LaunchParams Parg) {             \
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];                       \
    PRE;                                                                                 \
    MRP_LL_WINDOW_BLOCKS(smem, jobS, resS);                                              \
    const LaunchParams& P = Parg;                                                        \
    __VA_ARGS__(P, smem, jobS, resS);                                                    \
  }
#define MRP_LL_WINDOW_KERNEL(NAME, ...) MRP_LL_WINDOW_KERNEL_PRE(NAME, (void)0, __VA_ARGS__)
// The two mixed kernels are held to three waves per SIMD (168 registers): their own need is 167 vector registers, and the
// scalar registers saved around the calls of the searches that are real functions (runJobTaEps, runTaEpsLds, runJobTableH) took
// one accumulation register beyond that — a fourth of the kernel's residency for a register that holds spilled scalars.
#define MRP_LL_MIXED_KERNEL(NAME, ...)                                                                          \
  extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) NAME(LaunchParams Parg) { \
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];                                              \
    MRP_LL_WINDOW_BLOCKS(smem, jobS, resS);                                                                     \
    const LaunchParams& P = Parg;                                                                               \
    __VA_ARGS__(P, smem, jobS, resS);                                                                           \
  }
// The A*-epsilon-only kernels stay at two waves per SIMD, eight windows per CU: they name vector register 175 once, at
// their entry, where nothing is live, so their allocation is 176 registers — in the compiler's report, in the code object
// and in what the runtime grants alike.  (Their own need is 155 since the goal branch of compactSearch, with its 32 staging
// registers, stands behind the search loop: a third wave, ten windows per CU.  More searches per CU make each one slower,
// DESIGN.md section 7, so that residency is a change of its own to measure.)
#define MRP_LL_TWO_WAVES asm volatile("; two waves per SIMD" ::: "v175")
template <int KIND>
DEVI void batchLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  DBG(P, 0, 1);
  for (;;) {
    // every lane takes part (lane 0 adds 1, the others 0): the kernel deliberately contains no `if (lane == 0)`
    // blocks — hipcc once merged two of them into a wave-divergent wrapper loop that only lane 0 could leave.
    uint32_t j = atomicAdd(P.queue_head, lane == 0 ? 1u : 0u);
    j = rfl(j) - P.queue_base;
    DBG(P, 1, j + 1);
    if (j >= P.n_jobs) break;
    processJob<KIND>(P, P.jobs + j, P.results + j, P.out_paths + (size_t)j * P.out_host_stride, smem, arenaSlot, jobS, resS);
    DBG(P, 3, j + 1);
  }
  DBG(P, 4, 1);
}

MRP_LL_MIXED_KERNEL(mrp_ll_search_kernel, batchLoop<0>)  // mixed batches
MRP_LL_WINDOW_KERNEL_PRE(mrp_ll_ecbs_search_kernel, MRP_LL_TWO_WAVES, batchLoop<1>)  // A*-epsilon jobs only
MRP_LL_WINDOW_KERNEL(mrp_ll_cbs_search_kernel, batchLoop<2>)  // A* jobs only
// ll_ta_root.h's one runner, four times (the macro is variadic: a template-id with a comma passes as it stands)
MRP_LL_WINDOW_KERNEL(mrp_ll_ta_root_kernel, taRootLoop<false, 1>)  // roots of CBS-TA conflict trees, the A* kernels' window
MRP_LL_WINDOW_KERNEL(mrp_ll_ta_eps_root_kernel, taRootLoop<true, 1>)  // roots of ECBS-TA conflict trees, the mixed kernel's window
MRP_LL_WINDOW_KERNEL(mrp_ll_ta_root_wide_kernel, taRootLoop<false, kTaRootWideGroups>)  // the same for roots of up to 256 agents
MRP_LL_WINDOW_KERNEL(mrp_ll_ta_eps_root_wide_kernel, taRootLoop<true, kTaRootWideGroups>)

// SIPP batches (MRP_LL_SIPP jobs only) run in their own kernels so that the CBS/ECBS kernels' register allocation is
// not widened by a path they never take.  Same queue discipline as mrp_ll_search_kernel.
extern "C" __global__ void __launch_bounds__(64) mrp_ll_sipp_kernel(LaunchParams Parg) {
  __shared__ DevJob jobS;
  __shared__ DevResult resS;
  const LaunchParams& P = Parg;
  const uint32_t lane = threadIdx.x;
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  for (;;) {
    uint32_t j = atomicAdd(P.queue_head, lane == 0 ? 1u : 0u);
    j = rfl(j) - P.queue_base;
    if (j >= P.n_jobs) break;
    processSippJob(P, P.jobs + j, P.results + j, P.out_paths + (size_t)j * P.out_host_stride, arenaSlot, nullptr, jobS, resS);
  }
}

// Session mode.  The same workgroups stay resident for a whole solve and are fed through a ticket ring in coherent
// pinned host memory.  An entry is (generation << 11) | job slot; job slots (descriptor, constraint words, path table,
// result) come from a host-side free list, so a slow search holds one slot, not the ring.  A workgroup takes ticket t
// with a device fetch-add and waits until the host has published it.  There is ONE queue and it is first in, first out:
// which search runs next is decided by the HOST, which keeps the queue shallow and publishes in priority order (the
// conflict-tree drivers, csrc/hl/mrp_hl.cpp) — a second, device-side priority ring that every polling wavefront had to
// look at (round 1) cost more in claim traffic than it saved.
// The finished job's slot gets ring_done[slot] = (ticket + 1) & 0x3FFFFFFF | 1 << 30 (never 0) and an entry in the
// completion queue.
// Exit conditions every wave reaches: *ring_stop != 0, or the host's heartbeat word has not moved for
// ring_idle_limit_s seconds (the host is gone).
// A finished job becomes visible to the host: its done word, then its entry in the completion queue.
template <bool SIPP>
DEVI void publishDone(const LaunchParams& P, uint32_t slot, uint32_t doneVal) {
  const uint32_t lane = threadIdx.x;
  const uint32_t compSize = P.n_slots;
#ifdef MRP_LL_SESSION_FENCES
  __threadfence_system();
  __hip_atomic_store(P.ring_done + slot, doneVal, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  // completion queue: the host consumes finished jobs in O(1) each instead of scanning the ring
  uint32_t cidx = atomicAdd(P.comp_count, lane == 0 ? 1u : 0u);
  cidx = rfl(cidx);
  __hip_atomic_store(P.comp_ring + (cidx % compSize), ((cidx / compSize + 1) << kRingSlotBits) | slot, __ATOMIC_RELEASE,
                     __HIP_MEMORY_SCOPE_SYSTEM);
#else
  // Publication without a cache write-back.  What the host reads (result record, path, done word, completion entry)
  // was written with system-scope stores (processJob: hostStore32) that go through the L2 to host memory, and they
  // are complete — in order for the host — once vmcnt says so.  What other workgroups read (the path-store slot) was
  // written with agent-scope stores that go through to memory (processJob).  A system-scope release would add a
  // buffer_wbl2 sc0 sc1: a write-back of EVERY dirty line of this XCD's L2 (the bitmaps, cameFrom bytes, arena nodes and
  // heaps of every search on the XCD), per job.
  // The rule this relies on (LLVM AMDGPU memory model, gfx942 / gfx950): a system-scope (sc0 sc1) store is a write-through
  // store — it is performed at the system coherence point, not held in this XCD's L2 — and `s_waitcnt vmcnt(0)` returns only
  // when every earlier vector-memory operation of the wave, stores included (gfx9 counts them in vmcnt), has been
  // acknowledged there.  Stores of ONE wave that have all been acknowledged before a later store is issued cannot be
  // observed out of order by any agent.  That is the release half of the model's store-release code sequence
  // (`buffer_wbl2 sc0 sc1; s_waitcnt vmcnt(0); store sc0 sc1`) minus the write-back, which exists for data written with
  // weaker scopes — of which the host reads none.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(P.ring_done + slot, doneVal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // completion queue: the host consumes finished jobs in O(1) each instead of scanning the ring; it looks at the done
  // word of the slot an entry names, so the done word goes first
  uint32_t cidx = atomicAdd(P.comp_count, lane == 0 ? 1u : 0u);
  cidx = rfl(cidx);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(P.comp_ring + (cidx % compSize), ((cidx / compSize + 1) << kRingSlotBits) | slot, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
#endif
}

// Safety net for a host that died: the host bumps a heartbeat word on every submit / poll.  True when that word has not
// moved for ring_idle_limit_s (tBeat: the last look, lastBeat: what it saw) — the waiting workgroup leaves; a live host that is
// merely slow to publish (a long tail search elsewhere, a caller pausing between submits while it keeps polling) never loses
// the workgroup that holds the ticket it will publish next.
DEVI bool hostGone(const LaunchParams& P, uint64_t& tBeat, uint32_t& lastBeat) {
  const uint64_t idleLimit = (uint64_t)P.ring_idle_limit_s * 100000000ull;  // s_memrealtime ticks at 100 MHz
  if (__builtin_amdgcn_s_memrealtime() - tBeat <= idleLimit) return false;
  const uint32_t hb = rfl(__hip_atomic_load(P.ring_head + kHeartbeatWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
  if (hb == lastBeat) return true;
  lastBeat = hb;
  tBeat = __builtin_amdgcn_s_memrealtime();
  return false;
}
// A leaving workgroup's share of sess_ticks[first .. first + 2]: busy ticks, idle ticks, "ran at least one job"
DEVI void reportTicks(const LaunchParams& P, uint32_t first, uint64_t busyTicks, uint64_t idleTicks) {
  const uint32_t lane = threadIdx.x;
  atomicAdd(P.sess_ticks + first, lane == 0 ? (unsigned long long)busyTicks : 0ull);
  atomicAdd(P.sess_ticks + first + 1, lane == 0 ? (unsigned long long)idleTicks : 0ull);
  atomicAdd(P.sess_ticks + first + 2, (lane == 0 && busyTicks != 0) ? 1ull : 0ull);
}

template <bool SIPP, int KIND, int TIERS = kTiersAll>
DEVI void residentLoop(const LaunchParams& P, uint8_t* smem, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  uint64_t busyTicks = 0, idleTicks = 0;
  const uint32_t q0 = P.ring_size;
  uint32_t* const ring0 = P.ring_state;
  uint32_t* const tickets0 = P.queue_head;        // device counters, 64 bytes apart
  uint32_t* const head0 = P.ring_head;            // host words, 64 bytes apart
  uint32_t* const mirror = P.queue_head + 32;     // device: [0] copy of *head0, [16] copy of *ring_stop (zeroed with the tickets)
  bool haveBulk = false;                          // a bulk ticket is held and not yet served
  uint32_t bulkT = 0;
  uint32_t lastBeat = 0;                          // host heartbeat value seen at the last idle-limit check
  for (;;) {
    uint32_t slot = 0, doneVal = 0;
    bool stop = false;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t tBeat = t0;
    for (;;) {
      if (!haveBulk) {
        bulkT = rfl(atomicAdd(tickets0, lane == 0 ? 1u : 0u));
        haveBulk = true;
      }
      // Waiting workgroups do NOT poll the host.  The published-ticket count lives in pinned host memory (head0); its
      // device-side MIRROR (tickets0[32], in HBM) is what every waiting workgroup looks at, with agent-scope loads that
      // cost an L2 access.  Exactly one waiting workgroup — the one whose ticket equals the mirror, i.e. the next in line;
      // tickets are consecutive, so while anybody waits there is one — reads the host's word (every ~2 us), copies it
      // into the mirror when it has moved, and copies the host's stop flag likewise.  PCIe reads per engine: one poller
      // instead of one per idle workgroup.  (Round 2 let every idle workgroup poll the host with a back-off; with two
      // engines of 896 workgroups and a host that cannot keep them busy that is ~4e7 uncached reads/s through a handful
      // of L2 channels: measured, the HBM tier ran 14x slower and a 65536-instance step took 6.8 s instead of 1 s.)
      // The others back off in proportion to how far ahead of the mirror their ticket is (next every ~2 us, the k-th
      // every ~2k us, <= ~100 us).
      // The host loads are RELAXED system-scope loads (they go to the host word, not to a cached copy); the ONE acquire
      // sits behind the generation match.  An acquire load per poll is a buffer_inv on this CU's L1 — the cache the
      // ten other searches of the CU are working in — for every look of every idle wavefront (MI355X_MICROARCH.md:
      // "polling with ACQUIRE loads -> correct, 2-3x slower per hop").  -DMRP_LL_RING_POLL_ACQUIRE: the old form (A/B).
#ifdef MRP_LL_RING_POLL_ACQUIRE
      constexpr int kPollOrder = __ATOMIC_ACQUIRE;
#else
      constexpr int kPollOrder = __ATOMIC_RELAXED;
#endif
      uint32_t hd = rfl(__hip_atomic_load(mirror, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      uint32_t sp = 0;
#ifndef MRP_LL_RING_POLL_ALL
      if (hd == bulkT) {  // next in line: look at the host for everybody
#else
      {                   // A/B: every waiting workgroup polls the host (round 2)
#endif
        const uint32_t hh = rfl(__hip_atomic_load(head0, kPollOrder, __HIP_MEMORY_SCOPE_SYSTEM));
        if ((int32_t)(hh - hd) > 0) {
          hd = hh;
#ifndef MRP_LL_RING_POLL_ALL
          __hip_atomic_store(mirror, hh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // single writer: only T == mirror gets here
#endif
        }
        sp = rfl(__hip_atomic_load(P.ring_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
        if (sp != 0) __hip_atomic_store(mirror + 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if ((int32_t)(hd - bulkT) > 0) {
        const uint32_t gen = (bulkT / q0 + 1) & 0x1FFFFFu;
        const uint32_t e = rfl(__hip_atomic_load(ring0 + bulkT % q0, kPollOrder, __HIP_MEMORY_SCOPE_SYSTEM));
        if ((e >> kRingSlotBits) == gen) {
          // NO acquire fence here.  What the host wrote before publishing (descriptor, constraint words, ids, tables) is
          // read with system-scope loads that go past the caches (hostLoad32: processJob, runJob).  A system-scope
          // acquire FENCE is a buffer_inv sc0 sc1 — it throws away every clean line of this XCD's L2, i.e. the bitmaps,
          // nodes and heaps of the 380 other searches that share it — and round 3 measured what 4e6 of them per second
          // (with the write-backs below) cost: 2.9 instead of 2.5 us per expansion in the compact tier and 11.7
          // instead of 5.1 us in the arena tier on a full chip.  -DMRP_LL_SESSION_FENCES restores them (A/B).
#if defined(MRP_LL_SESSION_FENCES) && !defined(MRP_LL_RING_POLL_ACQUIRE)
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: the job data the host wrote before publishing
#elif !defined(MRP_LL_RING_POLL_ACQUIRE)
          if (SIPP) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // (the SIPP kernels read their tables with plain loads)
#endif
          slot = e & kRingSlotMask;
          doneVal = ((bulkT + 1u) & 0x3FFFFFFFu) | 0x40000000u;
          haveBulk = false;
          break;
        }
      }
      if (sp == 0) sp = rfl(__hip_atomic_load(mirror + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (sp != 0 || hostGone(P, tBeat, lastBeat)) {  // (a workgroup always holds a bulk ticket while it waits)
        stop = true;
        break;
      }
      uint32_t naps = (int32_t)(bulkT - hd) > 0 ? 1 + (bulkT - hd) : 1;
      if (naps > 48) naps = 48;
      for (uint32_t q = 0; q < naps; ++q) __builtin_amdgcn_s_sleep(64);
    }
    const uint64_t t1c = __builtin_amdgcn_s_memrealtime();
    idleTicks += t1c - t0;
    if (stop) break;
    bool handOver = false;
    if constexpr (SIPP)
      processSippJob(P, P.jobs + slot, P.results + slot, P.out_paths + (size_t)slot * P.out_host_stride, arenaSlot, smem, jobS,
                     resS);
    else
      handOver = processJob<KIND, TIERS>(P, P.jobs + slot, P.results + slot, P.out_paths + (size_t)slot * P.out_host_stride, smem,
                                         arenaSlot, jobS, resS);
    if (TIERS == kTiersFront && handOver) {
      // The search does not fit the narrow tier: the heavy workgroups take it over (ll_device.h heavy_q).  One 8-byte store
      // carries everything they need — the job slot (whose descriptor still sits in host memory) and the done value.
      const uint32_t ht = rfl(atomicAdd(P.heavy_ctr, lane == 0 ? 1u : 0u));
      const unsigned long long he = ((unsigned long long)doneVal << 32) | (unsigned long long)(((ht / kRingSlots + 1u) << kRingSlotBits) | slot);
      __hip_atomic_store(P.heavy_q + (ht % kRingSlots), he, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      publishDone<SIPP>(P, slot, doneVal);
    }
    busyTicks += __builtin_amdgcn_s_memrealtime() - t1c;
  }
  reportTicks(P, 0, busyTicks, idleTicks);
}

MRP_LL_MIXED_KERNEL(mrp_ll_persistent_kernel, residentLoop<false, 0>)  // mixed sessions
MRP_LL_WINDOW_KERNEL_PRE(mrp_ll_ecbs_persistent_kernel, MRP_LL_TWO_WAVES, residentLoop<false, 1>)  // A*-epsilon only
// The front / heavy pair of an A*-epsilon session (ll_device.h heavy_q).  Front workgroups are the resident loop above
// with the narrow compact tier alone — no arena-tier code, hence a smaller register allocation; heavy workgroups wait on
// the device-side queue the front ones fill, run each search in the WIDE compact geometry (31.4 KB of LDS: open and focal
// lists of 3071 entries, walk queue) and, beyond even that, in the arena tier.
// Two builds of the front kernel.  mrp_ll_ecbs_front_kernel is the compiler's own allocation (153 VGPRs, three waves per
// SIMD = twelve per CU): the launch whose window holds a path table, which LDS caps at twelve per CU or fewer anyway.
// mrp_ll_ecbs_front4_kernel is held to 128 VGPRs = four waves per SIMD, sixteen per CU, so that registers do not cap the
// fourteen 10 880-byte windows of a launch WITHOUT a table (mrp_ll_session_front_tables); the searches' own function needs
// 118 and is a call, what is spilled is state of the job set-up and of the chain's conflict scan.  Measured with the table in
// the window, the four-wave build runs an expansion 1.5-2 % slower than the other: each mode keeps
// the build that suits it.
#define MRP_LL_FRONT_KERNEL(NAME, ATTR)                                                                                  \
  extern "C" __global__ void __launch_bounds__(64) ATTR NAME(LaunchParams Parg) {                                        \
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];                                                       \
    MRP_LL_WINDOW_BLOCKS(smem, jobS, resS);                                                                              \
    const LaunchParams& P = Parg;                                                                                        \
    /* "the front launch runs" (the host turns a launch that never starts - streams sharing a hardware queue with a  */ \
    /* resident kernel - into an error instead of a hang): the last alive word                                        */ \
    if (blockIdx.x == 0) hostStore32(P.heavy_alive + (kRingSlots - 1u), 1u);                                             \
    residentLoop<false, 1, kTiersFront>(P, smem, jobS, resS);                                                            \
  }
MRP_LL_FRONT_KERNEL(mrp_ll_ecbs_front_kernel, )
MRP_LL_FRONT_KERNEL(mrp_ll_ecbs_front4_kernel, __attribute__((amdgpu_waves_per_eu(4, 4))))

// Exit conditions every wave reaches: the stop flag (its device mirror, written by the front workgroup that polls the
// host, or the host word itself, looked at every ~0.5 ms), or a host heartbeat that stood still for ring_idle_limit_s.
extern "C" __global__ void __launch_bounds__(64) mrp_ll_ecbs_heavy_kernel(LaunchParams Parg) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  MRP_LL_WINDOW_BLOCKS(smem, jobS, resS);
  const LaunchParams& P = Parg;
  const uint32_t lane = threadIdx.x;
  uint8_t* arenaSlot = P.arena + (size_t)blockIdx.x * P.arena_stride;
  uint32_t* const mirror = P.queue_head + 32;
  uint64_t busyTicks = 0, idleTicks = 0;
  hostStore32(P.heavy_alive + blockIdx.x, 1u);  // "this workgroup is resident" (the host checks before it relies on us)
  uint32_t lastBeat = 0;
  for (;;) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t tBeat = t0;
    const uint32_t ht = rfl(atomicAdd(P.heavy_ctr + 16, lane == 0 ? 1u : 0u));
    const uint32_t gen = ht / kRingSlots + 1u;
    unsigned long long e = 0;
    bool stop = false;
    uint32_t naps = 1, looks = 0;
    for (;;) {
      e = rfl64(__hip_atomic_load(P.heavy_q + (ht % kRingSlots), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if ((((uint32_t)e) >> kRingSlotBits) == gen) break;
      uint32_t sp = rfl(__hip_atomic_load(mirror + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (sp == 0 && (++looks & 31u) == 0u) sp = rfl(__hip_atomic_load(P.ring_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
      if (sp != 0 || hostGone(P, tBeat, lastBeat)) {
        stop = true;
        break;
      }
      for (uint32_t q = 0; q < naps; ++q) __builtin_amdgcn_s_sleep(64);  // ~2 us, doubling to ~16 us
      if (naps < 8) naps *= 2;
    }
    const uint64_t t1c = __builtin_amdgcn_s_memrealtime();
    idleTicks += t1c - t0;
    if (stop) break;
    const uint32_t slot = (uint32_t)e & kRingSlotMask, doneVal = (uint32_t)(e >> 32);
    (void)processJob<1, kTiersHeavy>(P, P.jobs + slot, P.results + slot, P.out_paths + (size_t)slot * P.out_host_stride, smem,
                                     arenaSlot, jobS, resS);
    publishDone<false>(P, slot, doneVal);
    busyTicks += __builtin_amdgcn_s_memrealtime() - t1c;
  }
  reportTicks(P, 4, busyTicks, idleTicks);
}

MRP_LL_WINDOW_KERNEL(mrp_ll_cbs_persistent_kernel, residentLoop<false, 2>)  // A* only

// The same resident loop for SIPP sessions (jobs of algo MRP_LL_SIPP only).  9.2 KB of LDS per workgroup hold up to 768
// nodes and the open list of a search on a device-resident table (16 workgroups per CU; ll_sipp.h kSippLdsCap).
extern "C" __global__ void __launch_bounds__(64) mrp_ll_sipp_persistent_kernel(LaunchParams Parg) {
  __shared__ __attribute__((aligned(16))) uint8_t sippTier[kSippLdsBytes];
  __shared__ DevJob jobS;
  __shared__ DevResult resS;
  const LaunchParams& P = Parg;
  residentLoop<true, 0>(P, sippTier, jobS, resS);
}

// The CBS / ECBS kernels by role and kind (0 = mixed, 1 = A*-epsilon jobs only, 2 = A* jobs only, see processJob; the front /
// heavy pair exists for kind 1 alone).  `slot` numbers the kernel for allowFullLds.
typedef void (*Kern)(LaunchParams);
enum Role : int { kBatch = 0, kResident = 1, kFront = 2, kHeavy = 3, kFront4 = 4, kTaRoot = 5, kTaEpsRoot = 6, kTaRootWide = 7, kTaEpsRootWide = 8 };
struct KernelRef {
  Kern fn;
  int slot;
};
static KernelRef kernelFor(Role role, int kind) {
  static const Kern table[13] = {mrp_ll_search_kernel,     mrp_ll_ecbs_search_kernel,     mrp_ll_cbs_search_kernel,
                                 mrp_ll_persistent_kernel, mrp_ll_ecbs_persistent_kernel, mrp_ll_cbs_persistent_kernel,
                                 mrp_ll_ecbs_front_kernel, mrp_ll_ecbs_heavy_kernel,      mrp_ll_ecbs_front4_kernel,
                                 mrp_ll_ta_root_kernel,    mrp_ll_ta_eps_root_kernel,     mrp_ll_ta_root_wide_kernel,
                                 mrp_ll_ta_eps_root_wide_kernel};
  const int slot = role == kFront ? 6 : role == kHeavy ? 7 : role == kFront4 ? 8 : role == kTaRoot ? 9 : role == kTaEpsRoot ? 10
                   : role == kTaRootWide ? 11 : role == kTaEpsRootWide ? 12 : 3 * role + (kind == 1 || kind == 2 ? kind : 0);
  return KernelRef{table[slot], slot};
}

// hipFuncAttributeMaxDynamicSharedMemorySize (a workgroup may take up to the CU's 160 KiB minus the static jobS/resS) for
// kernel `k` on the calling thread's current device; thread-safe, done once per (kernel, device): every worker thread
// launches through here, and the attribute is per device.
static hipError_t allowFullLds(const KernelRef& k) {
  static std::mutex mu;
  static bool done[13][64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  if (dev >= 0 && dev < 64 && done[k.slot][dev]) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[k.slot][dev] = true;
  return e;
}
static hipError_t launchWithLds(const KernelRef& k, const LaunchParams* P, uint32_t grid, uint32_t ldsBytes, hipStream_t stream) {
  const hipError_t e = allowFullLds(k);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k.fn, dim3(grid), dim3(64), ldsBytes, stream, *P);
  return hipGetLastError();
}
// Resident workgroups per CU the runtime reports for kernel `k` with `ldsBytes` of dynamic LDS (0 on error)
static int occupancyOf(const KernelRef& k, uint32_t ldsBytes) {
  int n = 0;
  if (allowFullLds(k) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(k.fn), 64, ldsBytes) != hipSuccess) return 0;
  return n;
}

}  // namespace mrp

// ---- host-callable launchers (declared in ll_launch.h) -----------------------------------------------------------
extern "C" uint32_t mrp_ll_lds_bytes(int kind, uint32_t capNodes, uint32_t rows, uint32_t rowWords, uint32_t pathBytes) {
  (void)rows; (void)rowWords;
  // without the compact tier a workgroup still stages its job descriptor and result through the window's control block
  return capNodes ? mrp::ldsBytes(pathBytes, kind == 1) : mrp::ct::oJob;
}

// kind: 0 = mixed, 1 = A*-epsilon jobs only, 2 = A* jobs only (see processJob)
extern "C" hipError_t mrp_ll_launch(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int kind,
                                    hipStream_t stream) {
  return mrp::launchWithLds(mrp::kernelFor(mrp::kBatch, kind), P, grid, ldsBytes, stream);
}
extern "C" hipError_t mrp_ll_launch_persistent(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int kind,
                                               hipStream_t stream) {
  return mrp::launchWithLds(mrp::kernelFor(mrp::kResident, kind), P, grid, ldsBytes, stream);
}
// Resident workgroups per CU of the persistent kernel of `kind`: what mrp_ll_configure_tiers tells its caller, who sizes a
// session with it.
extern "C" int mrp_ll_persistent_occupancy(int kind, uint32_t ldsBytes) {
  return mrp::occupancyOf(mrp::kernelFor(mrp::kResident, kind), ldsBytes);
}

// The front / heavy pair (kind 1 sessions with heavy workgroups).  `heavy`: 0 = the front workgroups with the narrow window
// and the table behind it (`ldsBytes`), 1 = the heavy ones with the wide window, 2 = the front workgroups of a launch whose
// window holds no table (the four-wave build of the kernel).
extern "C" uint32_t mrp_ll_heavy_lds_bytes(void) { return mrp::ct::Wide::windowBytes(true); }
static mrp::KernelRef frontHeavyKernel(int heavy) {
  return mrp::kernelFor(heavy == 1 ? mrp::kHeavy : heavy == 2 ? mrp::kFront4 : mrp::kFront, 1);
}
extern "C" hipError_t mrp_ll_launch_front_heavy(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int heavy,
                                                hipStream_t stream) {
  return mrp::launchWithLds(frontHeavyKernel(heavy), P, grid, heavy == 1 ? mrp_ll_heavy_lds_bytes() : ldsBytes, stream);
}
// Resident workgroups per CU of that kernel alone (0 on error).
extern "C" int mrp_ll_front_heavy_occupancy(int heavy, uint32_t ldsBytes) {
  return mrp::occupancyOf(frontHeavyKernel(heavy), heavy == 1 ? mrp_ll_heavy_lds_bytes() : ldsBytes);
}

// The roots of CBS-TA (eps = 0) or ECBS-TA (eps = 1) conflict trees (ll_ta_root.h): `grid` workgroups share P->n_jobs roots.
// ldsBytes: the window of the A* kernels (mrp_ll_lds_bytes(kind = 2)) for CBS-TA and of the mixed kernel (kind = 0) for
// ECBS-TA, so that every search meets the tiers an ordinary MRP_LL_ASTAR_TA / MRP_LL_ASTAR_EPS_TA batch gives it.
// wide: the kernel for roots of up to 256 agents, same window.
extern "C" hipError_t mrp_ll_launch_ta_root(const mrp::LaunchParams* P, uint32_t grid, uint32_t ldsBytes, int eps, int wide,
                                            hipStream_t stream) {
  const mrp::Role role = eps ? (wide ? mrp::kTaEpsRootWide : mrp::kTaEpsRoot) : (wide ? mrp::kTaRootWide : mrp::kTaRoot);
  return mrp::launchWithLds(mrp::kernelFor(role, 0), P, grid, ldsBytes, stream);
}

// The SIPP kernels' LDS is static: no attribute to set.
extern "C" hipError_t mrp_ll_launch_sipp(const mrp::LaunchParams* P, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(mrp::mrp_ll_sipp_kernel, dim3(grid), dim3(64), 0, stream, *P);
  return hipGetLastError();
}
extern "C" hipError_t mrp_ll_launch_sipp_persistent(const mrp::LaunchParams* P, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(mrp::mrp_ll_sipp_persistent_kernel, dim3(grid), dim3(64), 0, stream, *P);
  return hipGetLastError();
}
extern "C" int mrp_ll_sipp_persistent_occupancy(void) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(mrp::mrp_ll_sipp_persistent_kernel), 64, 0) !=
      hipSuccess)
    return 0;
  return n;
}
