// C-ABI of the host-side conflict-tree drivers (include/mrp_hl.h).  Worker threads each own one low-level engine
// context (mrp_ll_ctx is not thread-safe).  Default schedule (session mode): every worker keeps a resident kernel fed
// through the engine's job ring, draws instances from one shared pool and publishes an instance's next searches the
// moment its previous ones are back (SessionWorker in ct_session.hpp, runSippGroupSession).  Round-based schedule (mode 1 /
// MRP_HL_SIPP_BATCH): every round a thread gathers the ready searches of its instances into one batch (runGroup,
// runSippGroup).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "../../../include/mrp_hl.h"
#include "ct_session.hpp"
#include "ct_solver.hpp"
#include "grid2d_astar.hpp"
#include "instance_io.hpp"

using namespace mrp_hl;

struct mrp_hl_preloaded {
  mrp_hl_solver* owner = nullptr;
  int32_t nInst = 0;
  const mrp_hl_instance* instances = nullptr;
  std::vector<std::vector<int32_t>> idx;  // per worker: the instances of the interleaved static split
  std::vector<int32_t> mapBase;           // per engine: map id of instance 0 (every engine holds every map, so any
                                          // worker can take any instance; instance k has map id mapBase + k)
};

struct mrp_hl_solver {
  int32_t device = 0;
  std::vector<mrp_ll_ctx*> engines;
  mrp_ll_options llOpt;
  std::string err;
  int32_t nWorkers = 0;    // host worker threads the caller asked for (>= engines.size(): two may share an engine)
  int32_t nPreloaded = 0;  // live mrp_hl_preloaded objects (their maps are released with the last one)
  int32_t pathSlots = 0;   // slots of the engines' device path stores (0: not allocated)
  int32_t consSlots = 0, consWords = 0;  // the engines' device constraint stores (MRP_HL_DEVICE_CONSTRAINTS; 0: not allocated)
};

namespace {

// Drives instances idx[...] (map ids mapBase + idx[...]) to completion on one engine, one mrp_ll_search_batch per round
// of ready searches.
void runGroup(mrp_ll_ctx* ctx, const mrp_hl_options& opt, const mrp_hl_instance* instIn, mrp_hl_solution* sols,
              const std::vector<int32_t>& idx, int32_t mapBase, int32_t horizon, GroupResult& out) {
  const size_t n = idx.size();
  std::vector<std::unique_ptr<Instance>> inst(n);
  for (size_t k = 0; k < n; ++k) inst[k].reset(new Instance(instIn[idx[k]], mapBase + idx[k], opt));
  std::vector<std::vector<LLRequest>> req(n), nextReq(n);
  for (size_t k = 0; k < n; ++k) inst[k]->start(req[k]);

  JobBatch batch;
  std::vector<mrp_ll_job>& jobs = batch.jobs;
  std::vector<mrp_ll_result> results;
  std::vector<int32_t> statesPool;
  std::vector<LLAnswer> ans;
  int64_t ranExpansions = 0;

  for (;;) {
    auto tA = clockNow();
    batch.clear();
    for (size_t k = 0; k < n; ++k)
      for (const LLRequest& r : req[k]) batch.add(*inst[k], r);
    if (jobs.empty()) break;
    batch.patch();
    results.assign(jobs.size(), mrp_ll_result());
    bindResults(results.data(), jobs.size(), statesPool, horizon);
    auto tB = clockNow();
    int rc = mrp_ll_search_batch(ctx, static_cast<int32_t>(jobs.size()), jobs.data(), results.data());
    auto tC = clockNow();
    if (rc != MRP_LL_SUCCESS) {
      out.err = std::string("mrp_ll_search_batch: ") + mrp_ll_last_error(ctx);
      return;
    }
    out.rounds += 1;
    out.searches += static_cast<int64_t>(jobs.size());
    // answers go back group by group (the requests of one group are consecutive), in request order
    size_t q = 0;
    for (size_t k = 0; k < n; ++k) {
      nextReq[k].clear();
      const std::vector<LLRequest>& rq = req[k];
      for (size_t a = 0; a < rq.size();) {
        size_t b = a;
        ans.clear();
        while (b < rq.size() && rq[b].group == rq[a].group) {
          ranExpansions += results[q].expanded;
          ans.push_back(answerOf(results[q]));
          ++q;
          ++b;
        }
        inst[k]->deliver(rq[a].group, ans, nextReq[k]);
        a = b;
      }
      if (inst[k]->done()) nextReq[k].clear();  // requests of a finished instance point into freed CT nodes
      req[k].swap(nextReq[k]);
    }
    auto tD = clockNow();
    out.buildS += secondsBetween(tA, tB);
    out.llS += secondsBetween(tB, tC);
    out.consumeS += secondsBetween(tC, tD);
  }
  for (size_t k = 0; k < n; ++k) {
    writeSolution(*inst[k], sols[idx[k]]);
    out.expansions += inst[k]->llExpanded();
    out.specSearches += inst[k]->specSearches();
  }
  out.specWasted += ranExpansions - out.expansions;
}

// MRP_HL_PIN="base[,stride]": worker t of a batch call runs on CPU base + t * stride (default: wherever the scheduler
// puts it).  Tuning knob for hosts whose CPUs are spread over sockets / SMT siblings.
void pinWorker(int32_t t) {
  const char* e = std::getenv("MRP_HL_PIN");
  if (!e) return;
  int base = 0, stride = 1;
  if (std::sscanf(e, "%d,%d", &base, &stride) < 1) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  CPU_SET(base + t * stride, &set);
  (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
}

}  // namespace

extern "C" {

int mrp_hl_solver_create(int32_t device, int32_t nThreads, const mrp_ll_options* llOpt, mrp_hl_solver** out) {
  if (!out) return MRP_LL_E_INVALID;
  *out = nullptr;
  if (nThreads <= 0) {
    unsigned hc = std::thread::hardware_concurrency();
    nThreads = static_cast<int32_t>(hc ? std::min<unsigned>(hc, 16) : 8);
  }
  // Engines: at most eight.  An engine of an ECBS batch keeps two resident kernels (front + heavy workgroups), and the
  // device time-slices a process's hardware queues — idle ones included — beyond about twenty (measured: the LDS tier's
  // 2.0 us per expansion becomes 2.5 with 24 streams in the process, 3.1 with 32).  Worker threads beyond the engines
  // share them two by two (co-workers, mrp_ll.h mrp_ll_submit_tagged): host cores feed conflict trees, engines feed the
  // device.
  int32_t maxEngines = 8;
  if (const char* e = std::getenv("MRP_HL_MAX_ENGINES")) maxEngines = std::max(1, std::atoi(e));
  const int32_t nWorkers = nThreads;
  nThreads = std::min(nThreads, maxEngines);
  // One HIP stream (= one resident kernel) per worker: each needs its own hardware queue, the ROCm default is 4.  Only
  // effective if the HIP runtime has not been initialised yet in this process; never overrides the caller.
  (void)setenv("GPU_MAX_HW_QUEUES", "32", 0);
  auto* s = new mrp_hl_solver();
  s->device = device;
  s->nWorkers = nWorkers;
  std::memset(&s->llOpt, 0, sizeof(s->llOpt));
  if (llOpt) s->llOpt = *llOpt;
  s->llOpt.device = device;
  // One batch in flight per engine.  A second ticket (MRP_HL_TICKETS=2: the round-based prioritized-SIPP schedule then
  // pipelines two half-batches) means a second arena per engine, and with it allocated the resident A*-epsilon searches
  // ran 7 % slower (busy workgroup time 731 s -> 788 s per 65 536 instances, same kernel) — so it is opt-in.
  if (s->llOpt.n_tickets <= 0) s->llOpt.n_tickets = 1;
  if (const char* e = std::getenv("MRP_HL_TICKETS")) s->llOpt.n_tickets = std::max(1, std::atoi(e));
  if (s->llOpt.slots <= 0) s->llOpt.slots = 512;
  if (s->llOpt.arena_nodes <= 0) s->llOpt.arena_nodes = 65536;
  for (int32_t t = 0; t < nThreads; ++t) {
    mrp_ll_ctx* ctx = nullptr;
    int rc = mrp_ll_create(&s->llOpt, &ctx);
    if (rc != MRP_LL_SUCCESS) {  // no GPU, no solver: there is no CPU path
      for (auto* e : s->engines) mrp_ll_destroy(e);
      delete s;
      return rc;
    }
    s->engines.push_back(ctx);
  }
  *out = s;
  return MRP_LL_SUCCESS;
}

void mrp_hl_solver_destroy(mrp_hl_solver* s) {
  if (!s) return;
  for (auto* e : s->engines) mrp_ll_destroy(e);
  delete s;
}

const char* mrp_hl_solver_last_error(const mrp_hl_solver* s) { return s ? s->err.c_str() : "null solver"; }

int mrp_hl_solver_ll_stats(mrp_hl_solver* s, mrp_ll_stats* out, int32_t reset) {
  if (!s || !out) return MRP_LL_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  for (auto* e : s->engines) {
    mrp_ll_stats st;
    mrp_ll_get_stats(e, &st);
    out->launches += st.launches;
    out->jobs += st.jobs;
    out->expansions += st.expansions;
    out->nodes_created += st.nodes_created;
    out->migrated += st.migrated;
    out->kernel_ms += st.kernel_ms;
    out->h2d_ms += st.h2d_ms;
    out->d2h_ms += st.d2h_ms;
    out->pack_ms += st.pack_ms;
    out->staged_bytes += st.staged_bytes;
    out->session_busy_ms += st.session_busy_ms;
    out->session_idle_ms += st.session_idle_ms;
    out->session_active_wgs += st.session_active_wgs;
    out->unpack_ms += st.unpack_ms;
    out->heavy_busy_ms += st.heavy_busy_ms;
    out->heavy_idle_ms += st.heavy_idle_ms;
    out->heavy_active_wgs += st.heavy_active_wgs;
    out->heavy_fallbacks += st.heavy_fallbacks;
    for (int q = 0; q < 8; ++q) out->prof[q] += st.prof[q];
    if (reset) mrp_ll_reset_stats(e);
  }
  return MRP_LL_SUCCESS;
}

int mrp_hl_solver_preload(mrp_hl_solver* s, int32_t nThreadsWanted, int32_t nInst, const mrp_hl_instance* instances,
                          mrp_hl_preloaded** out) {
  if (!s || !out || nInst < 0 || (nInst > 0 && !instances)) return MRP_LL_E_INVALID;
  *out = nullptr;
  int32_t nThreads = static_cast<int32_t>(s->engines.size());
  if (nThreadsWanted > 0) nThreads = std::min(nThreads, nThreadsWanted);
  const int32_t nEng = std::max(1, nThreads);  // engines that receive the maps: all the caller allows, however small the batch
  nThreads = std::max(1, std::min(nThreads, std::max(nInst, 1)));
  auto* p = new mrp_hl_preloaded();
  p->owner = s;
  p->nInst = nInst;
  p->instances = instances;
  p->idx.resize(nThreads);
  // Every engine receives every map (a 32x32 bitmap is 128 bytes), so any worker can run any instance: the session
  // driver lets the workers draw instances from one pool.  idx keeps the interleaved static split (instance k ->
  // thread k % nThreads) for the round-based schedule.
  for (int32_t k = 0; k < nInst; ++k) p->idx[k % nThreads].push_back(k);
  p->mapBase.assign(nEng, 0);
  std::vector<int> rcs(nEng, MRP_LL_SUCCESS);
  {
    std::vector<std::thread> th;
    for (int32_t t = 0; t < nEng; ++t)
      th.emplace_back([&, t]() {
        for (int32_t k = 0; k < nInst; ++k) {
          const mrp_hl_instance& in = instances[k];
          int32_t mid = -1;
          int rc = mrp_ll_upload_map(s->engines[t], in.dimx, in.dimy, in.n_obstacles, in.obstacles_xy, &mid);
          if (rc != MRP_LL_SUCCESS) {
            rcs[t] = rc;
            return;
          }
          if (k == 0) p->mapBase[t] = mid;
        }
        rcs[t] = mrp_ll_sync_maps(s->engines[t]);  // push the bitmaps to the device now, not at the first launch
      });
    for (auto& x : th) x.join();
  }
  for (int32_t t = 0; t < nEng; ++t)
    if (rcs[t] != MRP_LL_SUCCESS) {
      s->err = std::string("mrp_ll_upload_map / mrp_ll_sync_maps: ") + mrp_ll_last_error(s->engines[t]);
      delete p;
      return rcs[t];
    }
  s->nPreloaded += 1;
  *out = p;
  return MRP_LL_SUCCESS;
}

// The engines keep one map buffer for all preloaded batches alive at a time; when the last one goes, its maps go too
// (otherwise a persistent solver would grow its host and device map buffers with every batch).
void mrp_hl_preloaded_free(mrp_hl_preloaded* p) {
  if (!p) return;
  if (p->owner && --p->owner->nPreloaded == 0)
    for (auto* e : p->owner->engines) (void)mrp_ll_release_maps(e);
  delete p;
}

int mrp_hl_solver_solve(mrp_hl_solver* s, const mrp_hl_options* optIn, int32_t nInst, const mrp_hl_instance* instances,
                        mrp_hl_solution* solutions, mrp_hl_batch_stats* stats) {
  if (!s || !optIn || nInst < 0 || (nInst > 0 && (!instances || !solutions))) return MRP_LL_E_INVALID;
  mrp_hl_preloaded* p = nullptr;
  int rc = mrp_hl_solver_preload(s, optIn->n_threads, nInst, instances, &p);
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = mrp_hl_solver_solve_preloaded(s, optIn, p, solutions, stats);
  mrp_hl_preloaded_free(p);
  return rc;
}

int mrp_hl_solver_solve_preloaded(mrp_hl_solver* s, const mrp_hl_options* optIn, mrp_hl_preloaded* pre,
                                  mrp_hl_solution* solutions, mrp_hl_batch_stats* stats) {
  return mrp_hl_solver_solve_stream(s, optIn, 1, &pre, &solutions, stats);
}

// mrp_hl.h: n batches as one pool of instances.  One batch: every schedule of the drivers (rounds, static split, shared
// pool); several: the shared pool of the session driver (the others keep a barrier between batches by construction).
int mrp_hl_solver_solve_stream(mrp_hl_solver* s, const mrp_hl_options* optIn, int32_t nBatches, mrp_hl_preloaded* const* pres,
                               mrp_hl_solution* const* solsArr, mrp_hl_batch_stats* stats) {
  if (!s || !optIn || nBatches < 1 || !pres || !solsArr) return MRP_LL_E_INVALID;
  for (int32_t b = 0; b < nBatches; ++b)
    if (!pres[b] || pres[b]->owner != s || (pres[b]->nInst > 0 && !solsArr[b])) return MRP_LL_E_INVALID;
  mrp_hl_options opt = *optIn;
  mrp_hl_preloaded* pre = pres[0];
  StreamView view;  // (a single batch is a view of one batch)
  int64_t total = 0;
  for (int32_t b = 0; b < nBatches; ++b) {
    view.first.push_back(static_cast<int32_t>(total));
    view.inst.push_back(pres[b]->instances);
    view.sols.push_back(solsArr[b]);
    view.mapBase.push_back(&pres[b]->mapBase);
    total += pres[b]->nInst;
    if (total > INT32_MAX) {  // (checked before the next prefix is narrowed)
      s->err = "mrp_hl_solver_solve_stream: more than 2^31 - 1 instances in one stream";
      return MRP_LL_E_INVALID;
    }
  }
  view.first.push_back(static_cast<int32_t>(total));
  const bool streamed = nBatches > 1;
  // one pool of instances for all workers (MRP_HL_STATIC_SPLIT=1 restores the fixed interleaved split)
  const bool sharedPool = std::getenv("MRP_HL_STATIC_SPLIT") == nullptr;
  if (streamed && (opt.mode == 1 || !sharedPool)) {
    s->err = "mrp_hl_solver_solve_stream: several batches need the session driver's shared pool (mode 0, no MRP_HL_STATIC_SPLIT)";
    return MRP_LL_E_INVALID;
  }
  const int32_t nInst = static_cast<int32_t>(total);
  int32_t nThreads = static_cast<int32_t>(pre->idx.size());
  if (streamed) {  // engines that hold every batch's maps, and not more of them than there are instances
    nThreads = static_cast<int32_t>(pre->mapBase.size());
    for (int32_t b = 1; b < nBatches; ++b) nThreads = std::min(nThreads, static_cast<int32_t>(pres[b]->mapBase.size()));
    nThreads = std::max(1, std::min(nThreads, std::max(nInst, 1)));
  }
  const int32_t horizon = s->llOpt.max_horizon > 0 ? s->llOpt.max_horizon : 512;
  std::vector<GroupResult> gr(nThreads);
  // LDS tier sized for two resident searches per SIMD (8 per CU): one wavefront alone leaves about half of its SIMD's
  // issue slots idle (waiting on LDS / memory), a second one fills them.  The focal path table of a search is
  // [time][agents rounded up to 16] halfwords; 64 time steps of it are kept in LDS, the rest of a longer table lives in
  // the search's arena slot.
  int32_t maxAgents = 1;
  for (int32_t b = 0; b < nBatches; ++b)
    for (int32_t k = 0; k < pres[b]->nInst; ++k) maxAgents = std::max(maxAgents, pres[b]->instances[k].n_agents);
  const int32_t agentsPad = (maxAgents + 15) & ~15;
  int32_t occupancy = 4;
  if (s->llOpt.lds_nodes == 0 && opt.mode != 1) {  // the caller did not choose a geometry: pick one for this batch
    int32_t pathBytes = opt.algo == MRP_HL_ECBS ? std::min(16384, std::max(2048, agentsPad * 2 * 64)) : 32;
    int32_t tierNodes = 2048, tierRows = 64;  // the compact tier at its full size (open list: tierNodes / 2 entries)
    if (const char* e = std::getenv("MRP_HL_TIER")) {  // tuning knob: "nodes,rows,pathBytes"
      int a = 0, b = 0, c = 0;
      if (std::sscanf(e, "%d,%d,%d", &a, &b, &c) == 3) {
        tierNodes = a;
        tierRows = b;
        if (opt.algo == MRP_HL_ECBS) pathBytes = c;
      }
    }
    for (int32_t t = 0; t < nThreads; ++t)
      if (mrp_ll_configure_tiers(s->engines[t], tierNodes, tierRows, pathBytes, &occupancy) != MRP_LL_SUCCESS) {
        s->err = std::string("mrp_ll_configure_tiers: ") + mrp_ll_last_error(s->engines[t]);
        return MRP_LL_E_DEVICE;
      }
  }
  if (opt.mode != 1 && !s->engines.empty()) {  // what the runtime grants the kernel family of this batch's sessions
    int32_t occ = 0;
    if (mrp_ll_session_occupancy(s->engines[0], opt.algo == MRP_HL_ECBS ? MRP_LL_ASTAR_EPS : MRP_LL_ASTAR, &occ) == MRP_LL_SUCCESS && occ > 0)
      occupancy = occ;
  }
  // resident wavefronts per engine: the chip holds 256 CUs x `occupancy` workgroups of this kernel at once
  int32_t sessionWgs = std::max(16, std::min<int32_t>(s->llOpt.slots, (256 * occupancy) / nThreads));
  // ECBS: some of the device's LDS goes to heavy workgroups (wide LDS tier + arena tier: the searches that outgrow the
  // front tier — 6 % of the expansions at ten agents, 17 % at a hundred, scripts/search_stats.py).  One takes the LDS of
  // `displaced` front workgroups; five eighths / three quarters / all of the CUs get one.
  int32_t heavyPer = 0;
  const int32_t nRun = nThreads;  // engines of this batch
  if (opt.algo == MRP_HL_ECBS && opt.mode != 1 && !s->engines.empty() && s->llOpt.lds_nodes >= 0) {
    int32_t frontOcc = 0, frontLds = 0, heavyLds = 0;
    if (mrp_ll_session_tiers_geometry(s->engines[0], &frontOcc, &frontLds, &heavyLds) == MRP_LL_SUCCESS && frontOcc > 0 &&
        frontLds > 0) {
      // (measured, eight workers: ten agents 160 > 192 > 128 > 256; fifty 192 > 256 > 128; a hundred 256)
      int32_t heavyTotal = maxAgents <= 16 ? 160 : maxAgents <= 64 ? 192 : 256;
      if (const char* e = std::getenv("MRP_HL_HEAVY_WGS")) heavyTotal = std::max(0, std::atoi(e));  // tuning knob (0: one launch)
      heavyPer = heavyTotal / nRun + (heavyTotal % nRun ? 1 : 0);
      if (heavyPer > 0) {
        const int32_t granule = 512;  // LDS allocation granularity
        // (a window beyond 32 KB takes room as if it had 64 KB — measured, ll_compact.h MRP_CT_WIDE_GROUPS)
        const int32_t fl = (frontLds + granule - 1) / granule * granule;
        const int32_t hl = heavyLds > 32768 ? 65536 : (heavyLds + granule - 1) / granule * granule;
        const int32_t cuLds = 160 * 1024;
        const int32_t frontBeside = std::max(0, (cuLds - hl) / fl);          // front workgroups on a CU that hosts a heavy one
        // (beyond five heavy workgroups per eight CUs some CUs get two, and the second one costs more: measured, 192 / 224 /
        // 256 of them displace 3.6 front workgroups each, 160 exactly 3)
        const int32_t displaced = std::max(0, std::min(frontOcc, cuLds / fl) - frontBeside) + (heavyPer * nRun > 160 ? 1 : 0);
        const int32_t frontTotal = 256 * std::min(frontOcc, cuLds / fl) - displaced * heavyPer * nRun;
        // (never more than fits: a grid the device cannot place completely blocks its hardware pipe, and a launch queued
        // behind it — another worker's front workgroups — does not start until a resident kernel ends)
        sessionWgs = std::max(16, std::min<int32_t>(s->llOpt.slots - heavyPer, frontTotal / nRun - 2));
        if (sessionWgs + heavyPer > s->llOpt.slots || frontTotal <= 0) heavyPer = 0;  // (tiny engines: one launch serves all)
      }
    }
  }
  if (const char* e = std::getenv("MRP_HL_SESSION_WGS")) sessionWgs = std::max(1, std::atoi(e));  // tuning knob
  // f2: the engines' device-resident path stores (ECBS only: CBS's low level has no focal context).  A search leaves its
  // path there, and later jobs name the paths of their CT node by slot instead of shipping a [t][agent] table.
  // Used for conflict trees of up to 128 agents (MRP_HL_STORE_MAX_AGENTS; beyond that a table row no longer fits the
  // kernel's two 64-lane row loads and the job ships its table): bytes staged per search 1134 -> 134 (10 agents),
  // 5900 -> 303 (50), 12 087 -> 572 (100); steps 7 % / 3 % / 2 % faster.
  int32_t pathSlots = 0;
  int32_t storeMaxAgents = 128;
  if (const char* e = std::getenv("MRP_HL_STORE_MAX_AGENTS")) storeMaxAgents = std::atoi(e);
  if (opt.algo == MRP_HL_ECBS && opt.mode != 1 && maxAgents <= storeMaxAgents) {
    // every live conflict-tree node of every active instance holds one slot per replaced path: a worker with 16384
    // active instances (few threads, big batch) needs millions of them, and a slot is max_horizon halfwords
    pathSlots = std::max(1 << 18, std::min(1 << 22, (1 << 22) / std::max(nThreads, 1)));
    if (const char* e = std::getenv("MRP_HL_PATH_SLOTS")) pathSlots = std::max(0, std::atoi(e));  // 0 = ship tables (round 1)
    if (pathSlots != s->pathSlots) {
      for (int32_t t = 0; t < static_cast<int32_t>(s->engines.size()); ++t)
        if (mrp_ll_path_store_reserve(s->engines[t], pathSlots) != MRP_LL_SUCCESS) {
          pathSlots = 0;  // e.g. the CPU test build: fall back to tables everywhere
          for (int32_t u = 0; u <= t; ++u) (void)mrp_ll_path_store_reserve(s->engines[u], 0);
          break;
        }
      s->pathSlots = pathSlots;
    }
  }
  // MRP_HL_DEVICE_CONSTRAINTS=1 (session mode, CBS and ECBS): the engines' device-resident constraint stores.  A live
  // conflict-tree node holds one set slot per constraint it added, as it holds one path slot per path it replaced, so the
  // store has as many slots as the path store would; a set of more than MRP_HL_CONS_WORDS constraints (default 64: 256
  // bytes a slot, 64 MiB to 1 GiB per engine) ships flat.  Engines without the calls (weak references) leave the switch off.
  int32_t consSlots = 0, consWords = 0;
  if (opt.mode != 1 && std::getenv("MRP_HL_DEVICE_CONSTRAINTS") && std::atoi(std::getenv("MRP_HL_DEVICE_CONSTRAINTS")) != 0 &&
      engineHasConstraintStore()) {
    consSlots = std::max(1 << 18, std::min(1 << 22, (1 << 22) / std::max(nThreads, 1)));
    consWords = 64;
    if (const char* e = std::getenv("MRP_HL_CONS_SLOTS")) consSlots = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("MRP_HL_CONS_WORDS")) consWords = std::max(1, std::min(2048, std::atoi(e)));
    if (consSlots != s->consSlots || consWords != s->consWords) {
      for (int32_t t = 0; t < static_cast<int32_t>(s->engines.size()); ++t)
        if (reserveConstraintStore(s->engines[t], consSlots, consWords) != MRP_LL_SUCCESS) {
          for (int32_t u = 0; u <= t; ++u) (void)reserveConstraintStore(s->engines[u], 0, 0);
          consSlots = consWords = 0;  // every job ships its set, as with the switch off
          break;
        }
      s->consSlots = consSlots;
      s->consWords = consWords;
    }
  }
  std::atomic<int32_t> nextInstance(0);
  int32_t sessionGate = 0;
  auto t0 = std::chrono::steady_clock::now();
  {
    // session mode with the shared pool: worker threads beyond the engines join them as co-workers, two per engine
    int32_t nWork = nRun;
    if (opt.mode != 1 && sharedPool) {
      int32_t want = s->nWorkers;
      if (const char* e = std::getenv("MRP_HL_WORKERS")) want = std::max(1, std::atoi(e));  // tuning knob
      nWork = std::max(nRun, std::min(want, 2 * nRun));
      nWork = std::min(nWork, std::max(nRun, nInst));
    }
    gr.resize(static_cast<size_t>(nWork));
    SessionPlan plan;
    plan.opt = opt;
    plan.horizon = horizon;
    plan.workgroups = sessionWgs;
    plan.heavyWgs = heavyPer;
    plan.pathSlots = pathSlots;
    plan.consSlots = consSlots;
    plan.consWords = consWords;
    plan.gate = &sessionGate;
    plan.nEngines = nRun;
    plan.nWorkers = nWork;
    plan.view = &view;
    plan.pool = sharedPool ? &nextInstance : nullptr;
    plan.epoch = t0;
    plan.readKnobs();
    std::vector<CoSync> coSync(static_cast<size_t>(nRun));
    std::vector<std::thread> th;
    for (int32_t t = 0; t < nWork; ++t)
      th.emplace_back([&, t]() {
        pinWorker(t);
        if (opt.mode == 1) {
          runGroup(s->engines[t], opt, pre->instances, solsArr[0], pre->idx[t], pre->mapBase[t], horizon, gr[t]);
          return;
        }
        WorkerSeat seat;  // (static split: as many workers as engines, so worker t sits alone on engine t)
        seat.engineIdx = t % nRun;
        seat.coIndex = t / nRun;
        seat.coCount = 1 + (seat.engineIdx + nRun < nWork ? 1 : 0);
        seat.ctx = s->engines[seat.engineIdx];
        seat.co = seat.coCount > 1 ? &coSync[seat.engineIdx] : nullptr;
        seat.own = sharedPool ? nullptr : &pre->idx[t];
        SessionWorker(plan, seat, gr[t]).run();
      });
    for (auto& x : th) x.join();
  }
  auto t1 = std::chrono::steady_clock::now();
  mrp_hl_batch_stats st;
  std::memset(&st, 0, sizeof(st));
  st.wall_seconds = std::chrono::duration<double>(t1 - t0).count();
  for (auto& g : gr) {
    if (!g.err.empty()) {
      s->err = g.err;
      return MRP_LL_E_DEVICE;
    }
    st.rounds += g.rounds;
    st.ll_searches += g.searches;
    st.ll_expansions += g.expansions;
    st.speculative_searches += g.specSearches;
    st.wasted_ll_expansions += g.specWasted;
    st.root_solved += g.rootSolved;
    st.device_scans += g.deviceScans;
    st.build_seconds += g.buildS;
    st.ll_call_seconds += g.llS;
    st.consume_seconds += g.consumeS;
  }
  for (int32_t b = 0; b < nBatches; ++b)
    for (int32_t k = 0; k < pres[b]->nInst; ++k) st.solved += solsArr[b][k].status == MRP_HL_SOLVED ? 1 : 0;
  if (stats) *stats = st;
  return MRP_LL_SUCCESS;
}

namespace {

// The loop of mapf_prioritized_sipp.cpp:214-270 for instances idx[...] on one engine: round r plans agent r of every
// instance that still has one (agents of one instance are a chain — each plans against the intervals the earlier ones
// occupy — instances are independent).
// Test knob (MRP_HL_SIPP_MAX_EXPANSIONS): the expansion cap of every search of the prioritized-SIPP drivers, read per
// call; the reference has none (-1), and a capped search ends its instance with that status.
int64_t sippMaxExpansions() {
  const char* e = std::getenv("MRP_HL_SIPP_MAX_EXPANSIONS");
  return e && std::atoll(e) > 0 ? std::atoll(e) : -1;
}

// Uploads the map of a prioritized-SIPP instance and clears its solution; false (out.err set) if the engine refuses.
bool beginSippInstance(mrp_ll_ctx* ctx, const mrp_hl_instance& in, mrp_hl_sipp_solution& so, int32_t& mapId, GroupResult& out) {
  if (mrp_ll_upload_map(ctx, in.dimx, in.dimy, in.n_obstacles, in.obstacles_xy, &mapId) != MRP_LL_SUCCESS) {
    out.err = std::string("mrp_ll_upload_map: ") + mrp_ll_last_error(ctx);
    return false;
  }
  so.cost = 0;
  so.low_level_expanded = 0;
  so.n_planned = 0;
  so.status = 0;
  return true;
}

// The answer of agent `a`'s search goes into its instance's solution (mapf_prioritized_sipp.cpp:228-236, 249-262).  false: a
// capacity status (expansion cap, node arena, horizon), which is not the reference's answer for this agent, and every
// later agent of the instance would plan against the wrong intervals: THIS instance stops here and says so in its
// status; the other instances of the batch are not affected.
bool recordSippAnswer(const mrp_ll_result& r, int32_t a, mrp_hl_sipp_solution& so, GroupResult& out) {
  so.low_level_expanded += r.expanded;
  out.expansions += r.expanded;
  const bool ok = r.status == MRP_LL_OK, answered = ok || r.status == MRP_LL_NO_SOLUTION;
  if (!answered) so.status = r.status;
  if (so.planned) so.planned[a] = ok ? 1 : 0;
  if (so.n_states) so.n_states[a] = ok ? r.n_states : 0;
  if (ok) {
    so.n_planned += 1;
    so.cost += r.cost;
    const int32_t* S = r.states_txy;  // [t, x, y]
    if (so.states_xyt)
      for (int32_t i = 0; i < r.n_states && i < so.state_cap; ++i) {
        int32_t* dst = so.states_xyt + (static_cast<size_t>(a) * so.state_cap + i) * 3;
        dst[0] = S[3 * i + 1];
        dst[1] = S[3 * i + 2];
        dst[2] = S[3 * i];
      }
  }
  return answered;
}

void runSippGroup(mrp_ll_ctx* ctx, int32_t horizon, int32_t nTickets, const mrp_hl_instance* instances,
                  mrp_hl_sipp_solution* sols, const std::vector<int32_t>& idx, GroupResult& out) {
  struct Iv { int32_t s, e; };
  struct Prio {
    int32_t mapId = -1, agent = 0, dimx = 0;
    // allCollisionIntervals (mapf_prioritized_sipp.cpp:215): the reference keeps a std::map keyed by location and hands
    // every entry to setCollisionIntervals, whose result does not depend on the order of the locations; here: one list
    // per cell plus the cells that have one, in first-touch order
    std::vector<std::vector<Iv>> perCell;
    std::vector<int32_t> touched;
    std::vector<int32_t> xy, cnt, ivs;  // flattened for the job of the current round
    void add(int32_t x, int32_t y, Iv iv) {
      std::vector<Iv>& v = perCell[static_cast<size_t>(y) * dimx + x];
      if (v.empty()) touched.push_back(y * dimx + x);
      v.push_back(iv);
    }
  };
  const size_t n = idx.size();
  std::vector<Prio> st(n);
  for (size_t q = 0; q < n; ++q) {
    const mrp_hl_instance& in = instances[idx[q]];
    if (!beginSippInstance(ctx, in, sols[idx[q]], st[q].mapId, out)) return;
    st[q].dimx = in.dimx;
    st[q].perCell.assign(static_cast<size_t>(std::max(in.dimx, 0)) * std::max(in.dimy, 0), std::vector<Iv>());
  }
  const int32_t cap = std::max(horizon, 64);
  // Two halves of the instances take turns: while the searches of one half run on the GPU, the host consumes the
  // results of the other half and packs its next round (a round of a half still ends with its slowest search).
  struct Half {
    std::vector<size_t> members;
    std::vector<mrp_ll_job> jobs;
    std::vector<mrp_ll_result> results;
    std::vector<int32_t> owner, statesPool;
    int32_t ticket = -1;
    bool inflight = false;
  };
  Half half[2];
  for (size_t q = 0; q < n; ++q) half[(n >= 64 && nTickets >= 2) ? (q & 1) : 0].members.push_back(q);
  int64_t roundsOf[2] = {0, 0};

  // round of one half: agent p.agent of every member that still has one; returns false when there was nothing to do
  auto launch = [&](Half& H) -> bool {
    H.jobs.clear();
    H.owner.clear();
    for (size_t q : H.members) {
      Prio& p = st[q];
      const mrp_hl_instance& in = instances[idx[q]];
      if (p.agent >= in.n_agents) continue;
      p.xy.clear();
      p.cnt.clear();
      p.ivs.clear();
      for (int32_t cell : p.touched) {  // sipp.setCollisionIntervals(location, intervals) for every location (:224-226)
        const std::vector<Iv>& v = p.perCell[cell];
        p.xy.push_back(cell % p.dimx);
        p.xy.push_back(cell / p.dimx);
        p.cnt.push_back(static_cast<int32_t>(v.size()));
        for (const Iv& iv : v) {
          p.ivs.push_back(iv.s);
          p.ivs.push_back(iv.e);
        }
      }
      mrp_ll_job j;
      std::memset(&j, 0, sizeof(j));
      j.map_id = p.mapId;
      j.algo = MRP_LL_SIPP;
      j.w = 1.0f;
      j.start_x = in.starts_xy[2 * p.agent];
      j.start_y = in.starts_xy[2 * p.agent + 1];
      j.goal_x = in.goals_xy[2 * p.agent];
      j.goal_y = in.goals_xy[2 * p.agent + 1];
      j.max_expansions = sippMaxExpansions();
      j.n_collision_locations = static_cast<int32_t>(p.cnt.size());
      j.collision_xy = p.xy.data();
      j.collision_count = p.cnt.data();
      j.collision_intervals = p.ivs.data();
      H.jobs.push_back(j);
      H.owner.push_back(static_cast<int32_t>(q));
    }
    if (H.jobs.empty()) return false;
    H.results.assign(H.jobs.size(), mrp_ll_result());
    bindResults(H.results.data(), H.jobs.size(), H.statesPool, cap);
    int rc = mrp_ll_submit(ctx, static_cast<int32_t>(H.jobs.size()), H.jobs.data(), H.results.data(), &H.ticket);
    if (rc != MRP_LL_SUCCESS) {
      out.err = std::string("mrp_ll_submit: ") + mrp_ll_last_error(ctx);
      return false;
    }
    H.inflight = true;
    out.searches += static_cast<int64_t>(H.jobs.size());
    return true;
  };
  auto consume = [&](Half& H) -> bool {
    int rc = mrp_ll_wait(ctx, H.ticket);
    H.inflight = false;
    if (rc != MRP_LL_SUCCESS) {
      out.err = std::string("mrp_ll_wait: ") + mrp_ll_last_error(ctx);
      return false;
    }
    for (size_t jq = 0; jq < H.jobs.size(); ++jq) {
      Prio& p = st[H.owner[jq]];
      mrp_hl_sipp_solution& so = sols[idx[H.owner[jq]]];
      const mrp_ll_result& r = H.results[jq];
      if (!recordSippAnswer(r, p.agent, so, out)) {
        p.agent = instances[idx[H.owner[jq]]].n_agents;
        continue;
      }
      if (r.status == MRP_LL_OK) {
        const int32_t* S = r.states_txy;  // [t, x, y]
        // update collision intervals (:237-246): one interval per maximal stay on a cell
        int32_t lx = S[1], ly = S[2], lt = S[0];
        for (int32_t i = 1; i < r.n_states; ++i) {
          if (S[3 * i + 1] != lx || S[3 * i + 2] != ly) {
            p.add(lx, ly, Iv{lt, S[3 * i] - 1});
            lx = S[3 * i + 1];
            ly = S[3 * i + 2];
            lt = S[3 * i];
          }
        }
        const int32_t last = r.n_states - 1;
        p.add(S[3 * last + 1], S[3 * last + 2], Iv{S[3 * last], INT32_MAX});
      }
      p.agent += 1;
    }
    return true;
  };

  for (int hIdx = 0; hIdx < 2; ++hIdx)
    if (launch(half[hIdx])) roundsOf[hIdx] += 1;
  if (!out.err.empty()) return;
  for (int cur = 0; half[0].inflight || half[1].inflight; cur ^= 1) {
    Half& H = half[cur];
    if (!H.inflight) continue;
    if (!consume(H)) {
      if (half[cur ^ 1].inflight) (void)mrp_ll_wait(ctx, half[cur ^ 1].ticket);  // do not leave a batch behind
      return;
    }
    if (launch(H)) roundsOf[cur] += 1;
    if (!out.err.empty()) {
      if (half[cur ^ 1].inflight) (void)mrp_ll_wait(ctx, half[cur ^ 1].ticket);
      return;
    }
  }
  out.rounds = std::max(roundsOf[0], roundsOf[1]);
}

// The same loop in session mode: the SIPP kernel stays resident and every instance publishes its next agent's search the
// moment the previous one has come back — no round barrier, so an instance never waits for another instance's search.
void runSippGroupSession(mrp_ll_ctx* ctx, int32_t horizon, int32_t slots, int32_t nWorkers, const mrp_hl_instance* instances,
                         mrp_hl_sipp_solution* sols, const std::vector<int32_t>& idx, GroupResult& out) {
  struct Iv { int32_t s, e; };
  struct Prio {
    int32_t mapId = -1, agent = 0, ticket = -1;
    // allCollisionIntervals (mapf_prioritized_sipp.cpp:215) lives in the engine: an incrementally maintained table, so a
    // job is a copy of the current table instead of a rebuild from every interval of the instance
    mrp_ll_sipp_table* tab = nullptr;
    std::vector<int32_t> states;
    mrp_ll_result res;
  };
  const size_t n = idx.size();
  const int32_t cap = std::max(horizon, 64);
  std::vector<Prio> st(n);
  for (size_t q = 0; q < n; ++q) {
    const mrp_hl_instance& in = instances[idx[q]];
    if (!beginSippInstance(ctx, in, sols[idx[q]], st[q].mapId, out)) return;
    if (mrp_ll_sipp_table_create(ctx, st[q].mapId, &st[q].tab) != MRP_LL_SUCCESS) {
      out.err = "mrp_ll_sipp_table_create failed";
      return;
    }
  }
  struct TableGuard {  // the tables go when the group is done, whichever way it ends
    std::vector<Prio>& st;
    ~TableGuard() {
      for (Prio& p : st) mrp_ll_sipp_table_destroy(p.tab);
    }
  } tableGuard{st};
  // at most one wavefront per instance, and as many over all workers as the device holds (mrp_ll_session_occupancy:
  // sixteen per CU with the kernel's 9.2 KB LDS tier).  Round 2 found that more resident wavefronts only slowed each other
  // down; that was with cached tables and a fence pair per job — with uncached tables residency pays (ll_sipp.h,
  // MRP_LL_SIPP_LDS_NODES).
  int32_t occS = 6;
  if (mrp_ll_session_occupancy(ctx, MRP_LL_SIPP, &occS) != MRP_LL_SUCCESS || occS <= 0) occS = 6;
  const size_t perWorker = static_cast<size_t>(std::max(96, 256 * occS / std::max(nWorkers, 1)));
  int32_t wgs = static_cast<int32_t>(std::min<size_t>(std::min<size_t>(std::max<size_t>(n, 16), slots), perWorker));
  if (const char* e = std::getenv("MRP_HL_SIPP_WGS")) wgs = std::max(1, std::atoi(e));          // tuning knob
  if (mrp_ll_session_begin_sipp(ctx, wgs) != MRP_LL_SUCCESS) {
    out.err = std::string("mrp_ll_session_begin_sipp: ") + mrp_ll_last_error(ctx);
    return;
  }
  // 1 published, 0 no free job slot (retry later), -1 error
  auto submit = [&](size_t q) -> int {
    Prio& p = st[q];
    const mrp_hl_instance& in = instances[idx[q]];
    mrp_ll_job j;
    std::memset(&j, 0, sizeof(j));
    j.map_id = p.mapId;
    j.algo = MRP_LL_SIPP;
    j.w = 1.0f;
    j.start_x = in.starts_xy[2 * p.agent];
    j.start_y = in.starts_xy[2 * p.agent + 1];
    j.goal_x = in.goals_xy[2 * p.agent];
    j.goal_y = in.goals_xy[2 * p.agent + 1];
    j.max_expansions = sippMaxExpansions();
    j.sipp_table = p.tab;  // sipp.setCollisionIntervals(location, intervals) for every location (:224-226), kept up to date
    j.sipp_commit = 1;     // ... by the engine: the stays of the path it finds become collision intervals (:237-246)
    bindResults(&p.res, 1, p.states, cap);
    int rc = mrp_ll_submit(ctx, 1, &j, &p.res, &p.ticket);
    if (rc == MRP_LL_E_BUSY) return 0;
    if (rc != MRP_LL_SUCCESS) {
      out.err = std::string("mrp_ll_submit: ") + mrp_ll_last_error(ctx);
      return -1;
    }
    out.searches += 1;
    return 1;
  };
  std::vector<size_t> backlog, ticketOwner, doneOwners;
  std::vector<int32_t> doneTickets(64);
  for (size_t q = n; q-- > 0;)
    if (instances[idx[q]].n_agents > 0) backlog.push_back(q);
  size_t nInflight = 0;
  bool failed = false;
  int64_t maxAgents = 0;
  auto t0 = std::chrono::steady_clock::now();
  static const bool timing = std::getenv("MRP_HL_SIPP_TIMING") != nullptr;  // where a worker thread's time goes
  double tSubmit = 0, tPoll = 0, tConsume = 0;
  uint64_t nPolls = 0, nEmptyPolls = 0;
  ProgressWatchdog watchdog;
  while (!failed && (nInflight != 0 || !backlog.empty())) {
    bool progress = false;
    auto tA = timing ? clockNow() : t0;
    while (!backlog.empty()) {
      const size_t q = backlog.back();
      int r = submit(q);
      if (r < 0) failed = true;
      if (r <= 0) break;
      backlog.pop_back();
      if (static_cast<size_t>(st[q].ticket) >= ticketOwner.size()) ticketOwner.resize(st[q].ticket + 1, 0);
      ticketOwner[st[q].ticket] = q;
      nInflight += 1;
      progress = true;
    }
    if (failed) break;
    int32_t nDone = 0;
    auto tB = timing ? clockNow() : t0;
    if (mrp_ll_poll_any(ctx, doneTickets.data(), static_cast<int32_t>(doneTickets.size()), &nDone) != MRP_LL_SUCCESS) {
      out.err = std::string("mrp_ll_poll_any: ") + mrp_ll_last_error(ctx);
      failed = true;
      break;
    }
    auto tC = timing ? clockNow() : t0;
    if (timing) {
      tSubmit += secondsBetween(tA, tB);
      tPoll += secondsBetween(tB, tC);
      nPolls += 1;
      nEmptyPolls += nDone == 0 ? 1 : 0;
    }
    doneOwners.resize(nDone);
    for (int32_t d = 0; d < nDone; ++d) doneOwners[d] = ticketOwner[doneTickets[d]];
    for (int32_t d = 0; d < nDone && !failed; ++d) {
      const size_t q = doneOwners[d];
      Prio& p = st[q];
      const mrp_hl_instance& in = instances[idx[q]];
      mrp_hl_sipp_solution& so = sols[idx[q]];
      progress = true;
      nInflight -= 1;
      // (the collision intervals of a path found, :237-246 — one per maximal stay on a cell — are already in the table:
      // sipp_commit)
      if (!recordSippAnswer(p.res, p.agent, so, out)) {
        p.agent = in.n_agents;
        continue;
      }
      p.agent += 1;
      maxAgents = std::max<int64_t>(maxAgents, p.agent);
      if (p.agent < in.n_agents) {
        int rr = backlog.empty() ? submit(q) : 0;
        if (rr < 0) {
          failed = true;
        } else if (rr == 1) {
          if (static_cast<size_t>(p.ticket) >= ticketOwner.size()) ticketOwner.resize(p.ticket + 1, 0);
          ticketOwner[p.ticket] = q;
          nInflight += 1;
        } else {
          backlog.push_back(q);
        }
      }
    }
    if (timing) tConsume += secondsBetween(tC, clockNow());
    if (!watchdog.turn(progress)) {
      out.err = "prioritized SIPP session: no progress for too long";
      failed = true;
    }
  }
  if (mrp_ll_session_end(ctx) != MRP_LL_SUCCESS && out.err.empty())
    out.err = std::string("mrp_ll_session_end: ") + mrp_ll_last_error(ctx);
  if (timing)
    std::fprintf(stderr, "[mrp_hl] sipp worker: %.1f ms total; submit %.1f ms, poll_any %.1f ms (%llu calls, %llu empty), consume %.1f ms\n",
                 secondsBetween(t0, clockNow()) * 1e3, tSubmit * 1e3, tPoll * 1e3, (unsigned long long)nPolls,
                 (unsigned long long)nEmptyPolls, tConsume * 1e3);
  out.rounds = maxAgents;  // longest chain of dependent searches
}

}  // namespace

int mrp_hl_solver_prioritized_sipp(mrp_hl_solver* s, int32_t nInst, const mrp_hl_instance* instances,
                                   mrp_hl_sipp_solution* sols, mrp_hl_batch_stats* stats) {
  if (!s || nInst < 0 || (nInst > 0 && (!instances || !sols))) return MRP_LL_E_INVALID;
  const int32_t horizon = s->llOpt.max_horizon > 0 ? s->llOpt.max_horizon : 512;
  // instances are independent: one share per worker thread / engine, as for CBS and ECBS
  const int32_t nThreads = std::max(1, std::min<int32_t>(static_cast<int32_t>(s->engines.size()), std::max(nInst, 1)));
  std::vector<std::vector<int32_t>> idx(nThreads);
  for (int32_t k = 0; k < nInst; ++k) idx[k % nThreads].push_back(k);
  std::vector<GroupResult> gr(nThreads);
  const bool batchMode = std::getenv("MRP_HL_SIPP_BATCH") != nullptr;  // the round-based schedule, for comparison
  auto t0 = std::chrono::steady_clock::now();
  {
    std::vector<std::thread> th;
    for (int32_t t = 0; t < nThreads; ++t)
      th.emplace_back([&, t]() {
        if (batchMode)
          runSippGroup(s->engines[t], horizon, s->llOpt.n_tickets, instances, sols, idx[t], gr[t]);
        else
          runSippGroupSession(s->engines[t], horizon, s->llOpt.slots, nThreads, instances, sols, idx[t], gr[t]);
      });
    for (auto& x : th) x.join();
  }
  mrp_hl_batch_stats bs;
  std::memset(&bs, 0, sizeof(bs));
  bs.wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (auto& g : gr) {
    if (!g.err.empty()) {
      s->err = g.err;
      return MRP_LL_E_DEVICE;
    }
    bs.rounds = std::max(bs.rounds, g.rounds);  // rounds run concurrently on the worker threads: the longest chain
    bs.ll_searches += g.searches;
    bs.ll_expansions += g.expansions;
  }
  for (int32_t k = 0; k < nInst; ++k) bs.solved += sols[k].n_planned == instances[k].n_agents ? 1 : 0;
  if (stats) *stats = bs;
  return MRP_LL_SUCCESS;
}

int mrp_hl_solve_batch(int32_t device, const mrp_hl_options* opt, int32_t nInst, const mrp_hl_instance* instances,
                       mrp_hl_solution* solutions, mrp_hl_batch_stats* stats) {
  mrp_hl_solver* s = nullptr;
  int rc = mrp_hl_solver_create(device, opt ? opt->n_threads : 0, nullptr, &s);
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = mrp_hl_solver_solve(s, opt, nInst, instances, solutions, stats);
  mrp_hl_solver_destroy(s);
  return rc;
}

// ---- one conflict tree, stepped by the caller (include/mrp_hl.h "mrp_hl_ct_*") ---------------------------------
struct mrp_hl_ct {
  std::unique_ptr<Instance> inst;
  std::vector<LLRequest> req;
  JobBatch batch;
  void rebuild() {  // job views of the pending requests; arrays stay valid until the next deliver
    batch.clear();
    for (const LLRequest& r : req) batch.add(*inst, r);
    batch.patch();
  }
};

int mrp_hl_ct_create(const mrp_hl_instance* in, const mrp_hl_options* opt, int32_t mapId, int32_t specWidth,
                     mrp_hl_ct** out) {
  if (!in || !opt || !out || in->n_agents < 0) return MRP_LL_E_INVALID;
  auto* c = new mrp_hl_ct();
  c->inst.reset(new Instance(*in, mapId, *opt));
  c->inst->setSpecWidth(specWidth);
  c->inst->start(c->req);
  if (c->inst->done()) c->req.clear();
  c->rebuild();
  *out = c;
  return MRP_LL_SUCCESS;
}

void mrp_hl_ct_destroy(mrp_hl_ct* c) { delete c; }

int32_t mrp_hl_ct_n_requests(const mrp_hl_ct* c) { return c ? static_cast<int32_t>(c->req.size()) : 0; }

int mrp_hl_ct_request(const mrp_hl_ct* c, int32_t k, mrp_ll_job* job, int32_t* group, int32_t* slot) {
  if (!c || k < 0 || k >= static_cast<int32_t>(c->req.size()) || !job) return MRP_LL_E_INVALID;
  *job = c->batch.jobs[k];
  if (group) *group = c->req[k].group;
  if (slot) *slot = c->req[k].slot;
  return MRP_LL_SUCCESS;
}

int mrp_hl_ct_deliver(mrp_hl_ct* c, int32_t group, int32_t n, const mrp_ll_result* results) {
  if (!c || n < 0 || (n > 0 && !results)) return MRP_LL_E_INVALID;
  // the group's requests are consecutive in the pending list: take them out, keep the others
  size_t a = 0;
  while (a < c->req.size() && c->req[a].group != group) ++a;
  size_t b = a;
  while (b < c->req.size() && c->req[b].group == group) ++b;
  if (a == c->req.size() || static_cast<int32_t>(b - a) != n) return MRP_LL_E_INVALID;
  std::vector<LLAnswer> ans;
  for (int32_t k = 0; k < n; ++k) ans.push_back(answerOf(results[k]));
  c->req.erase(c->req.begin() + static_cast<std::ptrdiff_t>(a), c->req.begin() + static_cast<std::ptrdiff_t>(b));
  c->inst->deliver(group, ans, c->req);
  if (c->inst->done()) c->req.clear();  // requests of a finished instance point into freed CT nodes
  c->rebuild();
  return MRP_LL_SUCCESS;
}

int32_t mrp_hl_ct_done(const mrp_hl_ct* c) { return c && c->inst->done() ? 1 : 0; }

namespace {
constexpr int32_t kRowHdr = 8;
constexpr int32_t kFailedRound = INT32_MIN;  // group word of a failure row (group ids are >= -1: -1 is the root step)
// the pending groups in order, and which rank searches which (group j -> rank j % world)
void roundOwners(const mrp_hl_ct& c, int32_t world, std::vector<int32_t>& groups, std::vector<int32_t>& ownerOfReq) {
  groups.clear();
  ownerOfReq.assign(c.req.size(), 0);
  for (size_t k = 0; k < c.req.size(); ++k) {
    if (groups.empty() || groups.back() != c.req[k].group) groups.push_back(c.req[k].group);
    ownerOfReq[k] = static_cast<int32_t>((groups.size() - 1) % static_cast<size_t>(world));
  }
}
}  // namespace

int32_t mrp_hl_ct_round_mine(mrp_hl_ct* c, mrp_ll_ctx* ll, int32_t rank, int32_t world, int32_t maxStates, int32_t* rows,
                             int32_t capRows, int32_t* rowsPerRank) {
  if (!c || !ll || !rows || !rowsPerRank || world < 1 || rank < 0 || rank >= world || maxStates < 1 || capRows < 1)
    return MRP_LL_E_INVALID;
  const size_t rowWords = static_cast<size_t>(kRowHdr) + static_cast<size_t>(maxStates);
  std::vector<int32_t> groups, owner;
  roundOwners(*c, world, groups, owner);
  for (int32_t r = 0; r < world; ++r) rowsPerRank[r] = 0;
  std::vector<size_t> mine;
  for (size_t k = 0; k < c->req.size(); ++k) {
    rowsPerRank[owner[k]] += 1;
    if (owner[k] == rank) mine.push_back(k);
  }
  auto fail = [&](int rc) {
    std::memset(rows, 0, rowWords * sizeof(int32_t));
    rows[0] = kFailedRound;
    rows[2] = rc;
    return rc;
  };
  if (static_cast<int32_t>(mine.size()) > capRows) return fail(MRP_LL_E_INVALID);
  std::vector<mrp_ll_job> jobs(mine.size());
  std::vector<mrp_ll_result> res(mine.size());
  std::vector<int32_t> states;
  bindResults(res.data(), res.size(), states, maxStates);
  for (size_t q = 0; q < mine.size(); ++q) jobs[q] = c->batch.jobs[mine[q]];
  if (!mine.empty()) {
    const int rc = mrp_ll_search_batch(ll, static_cast<int32_t>(jobs.size()), jobs.data(), res.data());
    if (rc != MRP_LL_SUCCESS) return fail(rc);
  }
  for (size_t q = 0; q < mine.size(); ++q) {
    int32_t* row = rows + q * rowWords;
    const mrp_ll_result& r = res[q];
    if (r.status == MRP_LL_PATH_TRUNCATED || r.n_states > maxStates) return fail(MRP_LL_E_INVALID);  // max_states too small
    row[0] = c->req[mine[q]].group;
    row[1] = c->req[mine[q]].slot;
    row[2] = r.status;
    row[3] = r.cost;
    row[4] = r.fmin;
    row[5] = static_cast<int32_t>(r.expanded & 0x7FFFFFFF);
    row[6] = static_cast<int32_t>(r.expanded >> 31);
    row[7] = r.n_states;
    for (int32_t k = 0; k < r.n_states; ++k) row[kRowHdr + k] = r.states_txy[3 * k + 1] | (r.states_txy[3 * k + 2] << 16);
  }
  return static_cast<int32_t>(mine.size());
}

int mrp_hl_ct_deliver_rows(mrp_hl_ct* c, const int32_t* gathered, int32_t world, int32_t rowsStride, int32_t maxStates) {
  if (!c || !gathered || world < 1 || rowsStride < 1 || maxStates < 1) return MRP_LL_E_INVALID;
  const size_t rowWords = static_cast<size_t>(kRowHdr) + static_cast<size_t>(maxStates);
  std::vector<int32_t> groups, owner;
  roundOwners(*c, world, groups, owner);
  std::vector<int32_t> perRank(world, 0);
  for (size_t k = 0; k < c->req.size(); ++k) perRank[owner[k]] += 1;
  // a rank that failed sent one row marked kFailedRound: every rank stops here, together
  for (int32_t r = 0; r < world; ++r)
    if (gathered[static_cast<size_t>(r) * rowsStride * rowWords] == kFailedRound) return MRP_LL_E_DEVICE;
  struct Row {
    int32_t slot;
    const int32_t* w;
  };
  std::map<int32_t, std::vector<Row>> byGroup;
  for (int32_t r = 0; r < world; ++r) {
    if (perRank[r] > rowsStride) return MRP_LL_E_INVALID;
    for (int32_t q = 0; q < perRank[r]; ++q) {
      const int32_t* w = gathered + (static_cast<size_t>(r) * rowsStride + q) * rowWords;
      byGroup[w[0]].push_back(Row{w[1], w});
    }
  }
  std::vector<int32_t> states;
  std::vector<mrp_ll_result> res;
  for (int32_t g : groups) {  // the same order on every rank
    auto it = byGroup.find(g);
    if (it == byGroup.end()) return MRP_LL_E_INVALID;
    std::vector<Row>& rws = it->second;
    std::sort(rws.begin(), rws.end(), [](const Row& a, const Row& b) { return a.slot < b.slot; });
    res.assign(rws.size(), mrp_ll_result());
    bindResults(res.data(), res.size(), states, maxStates);
    for (size_t q = 0; q < rws.size(); ++q) {
      const int32_t* w = rws[q].w;
      mrp_ll_result& r = res[q];
      r.status = w[2];
      r.cost = w[3];
      r.fmin = w[4];
      r.expanded = static_cast<int64_t>(w[5]) | (static_cast<int64_t>(w[6]) << 31);
      r.n_states = w[7];
      if (r.n_states < 0 || r.n_states > maxStates) return MRP_LL_E_INVALID;
      for (int32_t k = 0; k < r.n_states; ++k) {
        r.states_txy[3 * k] = k;
        r.states_txy[3 * k + 1] = w[kRowHdr + k] & 0xFFFF;
        r.states_txy[3 * k + 2] = w[kRowHdr + k] >> 16;
      }
    }
    const int rc = mrp_hl_ct_deliver(c, g, static_cast<int32_t>(res.size()), res.data());
    if (rc != MRP_LL_SUCCESS) return rc;
    if (c->inst->done()) break;
  }
  return MRP_LL_SUCCESS;
}

int mrp_hl_ct_solution(const mrp_hl_ct* c, mrp_hl_solution* out) {
  if (!c || !out || !c->inst->done()) return MRP_LL_E_INVALID;
  writeSolution(*c->inst, *out);
  return MRP_LL_SUCCESS;
}

int32_t mrp_hl_astar_grid2d(int32_t dimx, int32_t dimy, const uint8_t* obstacle_mask, int32_t start_x, int32_t start_y,
                            int32_t goal_x, int32_t goal_y, int32_t* states_xy, int32_t cap, int32_t* cost,
                            int64_t* expanded) {
  if (dimx <= 0 || dimy <= 0 || !obstacle_mask || !cost || !expanded || (cap > 0 && !states_xy)) return -1;
  return astarGrid2d(dimx, dimy, obstacle_mask, start_x, start_y, goal_x, goal_y, states_xy, cap, cost, expanded);
}

int mrp_hl_generate_instance(uint64_t seed, int32_t dimx, int32_t dimy, int32_t nObst, int32_t nAgents,
                             int32_t* obstXY, int32_t* startsXY, int32_t* goalsXY) {
  return generateInstance(seed, dimx, dimy, nObst, nAgents, obstXY, startsXY, goalsXY);
}

int mrp_hl_generate_instances(uint64_t seed0, int32_t n, int32_t dimx, int32_t dimy, int32_t nObst, int32_t nAgents,
                              int32_t* obstXY, int32_t* startsXY, int32_t* goalsXY) {
  if (n < 0 || (n > 0 && (!obstXY || !startsXY || !goalsXY))) return -1;
  unsigned hc = std::thread::hardware_concurrency();
  const int32_t nThreads = std::max<int32_t>(1, std::min<int32_t>(static_cast<int32_t>(hc ? hc : 8), std::min(n, 64)));
  std::atomic<int32_t> next(0), bad(0);
  std::vector<std::thread> th;
  for (int32_t t = 0; t < nThreads; ++t)
    th.emplace_back([&]() {
      for (;;) {
        const int32_t k0 = next.fetch_add(64, std::memory_order_relaxed);
        if (k0 >= n) return;
        for (int32_t k = k0; k < std::min(n, k0 + 64); ++k)
          if (generateInstance(seed0 + static_cast<uint64_t>(k), dimx, dimy, nObst, nAgents,
                               obstXY + static_cast<size_t>(k) * nObst * 2, startsXY + static_cast<size_t>(k) * nAgents * 2,
                               goalsXY + static_cast<size_t>(k) * nAgents * 2) != 0)
            bad.fetch_add(1, std::memory_order_relaxed);
      }
    });
  for (auto& x : th) x.join();
  return bad.load() == 0 ? 0 : -1;
}

}  // extern "C"
