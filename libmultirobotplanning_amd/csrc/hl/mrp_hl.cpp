// C-ABI of the host-side conflict-tree drivers (include/mrp_hl.h).  This file keeps the solver and its preloaded batches
// (create / destroy / preload / stats), the solve entry points and the thin generator and A* exports; the one translation
// unit includes its subjects:
//   solve_knobs.hpp    the MRP_HL_* environment knobs of a solve call, read once per call
//   launch_plan.hpp    what a solve call decides before it starts threads: tiers, resident workgroups, stores, workers
//   ct_session.hpp     the default schedule (session mode): every worker keeps a resident kernel fed through the engine's
//                      job ring, draws instances from one shared pool and publishes an instance's next searches the
//                      moment its previous ones are back (SessionWorker)
//   rounds_driver.hpp  the round-based schedule (mode 1): a thread gathers the ready searches of its instances into one
//                      batch per round (runGroup)
//   sipp_drivers.hpp   prioritized SIPP in both schedules (runSippGroupSession, runSippGroup with MRP_HL_SIPP_BATCH)
//   ct_stepped.hpp     one conflict tree stepped by the caller (mrp_hl_ct_*)
// Worker threads each own one low-level engine context (mrp_ll_ctx is not thread-safe).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "../../../include/mrp_hl.h"
#include "ct_session.hpp"
#include "ct_solver.hpp"
#include "ct_stepped.hpp"
#include "grid2d_astar.hpp"
#include "instance_io.hpp"
#include "launch_plan.hpp"
#include "rounds_driver.hpp"
#include "sipp_drivers.hpp"

using namespace mrp_hl;

// mrp_ll_session_front_tables through a weak reference, as the constraint store's calls (ct_session.hpp): a low-level
// library without it still loads, and its front workgroups keep their tables in LDS.
extern "C" __attribute__((weak)) int mrp_ll_session_front_tables(mrp_ll_ctx* ctx, int32_t in_memory);

// mrp_ll_compute_heuristics likewise (mrp_hl_solve_batch_table_h): without it that call answers MRP_LL_E_INVALID.
extern "C" __attribute__((weak)) int mrp_ll_compute_heuristics(mrp_ll_ctx* ctx, int32_t n, const int32_t* map_ids, const int32_t* goals_xy,
                                                               int32_t* heuristic_ids);

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
  const mrp_hl_options opt = *optIn;
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
  LaunchInput in;
  in.knobs = SolveKnobs::read();
  const bool streamed = nBatches > 1, sharedPool = in.sharedPool();
  if (streamed && (opt.mode == 1 || !sharedPool)) {
    s->err = "mrp_hl_solver_solve_stream: several batches need the session driver's shared pool (mode 0, no MRP_HL_STATIC_SPLIT)";
    return MRP_LL_E_INVALID;
  }
  in.algo = opt.algo;
  in.mode = opt.mode;
  in.nInst = static_cast<int32_t>(total);
  in.nEngines = static_cast<int32_t>(pre->idx.size());
  if (streamed) {  // engines that hold every batch's maps, and not more of them than there are instances
    in.nEngines = static_cast<int32_t>(pre->mapBase.size());
    for (int32_t b = 1; b < nBatches; ++b) in.nEngines = std::min(in.nEngines, static_cast<int32_t>(pres[b]->mapBase.size()));
    in.nEngines = std::max(1, std::min(in.nEngines, std::max(in.nInst, 1)));
  }
  in.workersAsked = s->nWorkers;
  for (int32_t b = 0; b < nBatches; ++b)
    for (int32_t k = 0; k < pres[b]->nInst; ++k) in.maxAgents = std::max(in.maxAgents, pres[b]->instances[k].n_agents);
  in.slots = s->llOpt.slots;
  in.ldsNodes = s->llOpt.lds_nodes;
  in.engineHasConstraintStore = engineHasConstraintStore();
  const int32_t nRun = in.nEngines, nAll = static_cast<int32_t>(s->engines.size());
  const int32_t horizon = s->llOpt.max_horizon > 0 ? s->llOpt.max_horizon : 512;

  // the engine calls the plan asks for: tiers on this call's engines, then what the runtime grants the kernel family of
  // this call's sessions, then the stores on every engine of the solver
  const TierChoice tiers = tierChoice(in);
  EngineReport rep;
  if (tiers.configure)
    for (int32_t t = 0; t < nRun; ++t)
      if (mrp_ll_configure_tiers(s->engines[t], tiers.nodes, tiers.rows, tiers.pathBytes, &rep.occupancy) != MRP_LL_SUCCESS) {
        s->err = llError("mrp_ll_configure_tiers", s->engines[t]);
        return MRP_LL_E_DEVICE;
      }
  if (in.session()) {
    int32_t occ = 0;
    if (mrp_ll_session_occupancy(s->engines[0], opt.algo == MRP_HL_ECBS ? MRP_LL_ASTAR_EPS : MRP_LL_ASTAR, &occ) == MRP_LL_SUCCESS && occ > 0)
      rep.occupancy = occ;
  }
  // where the front workgroups keep their focal tables: asked of every engine of this call before the geometry, which
  // answers for the window that results (an engine without the call — an older one, the CPU tests' stand-in — keeps them in LDS)
  const bool frontInMemory = in.knobs.frontTables >= 0 ? in.knobs.frontTables != 0 : in.maxAgents <= 64;  // (solve_knobs.hpp)
  if (tiers.askGeometry && &mrp_ll_session_front_tables != nullptr)
    for (int32_t t = 0; t < nRun; ++t)
      if (mrp_ll_session_front_tables(s->engines[t], frontInMemory ? 1 : 0) != MRP_LL_SUCCESS) {
        s->err = llError("mrp_ll_session_front_tables", s->engines[t]);
        return MRP_LL_E_DEVICE;
      }
  if (tiers.askGeometry && mrp_ll_session_tiers_geometry(s->engines[0], &rep.frontOcc, &rep.frontLds, &rep.heavyLds) != MRP_LL_SUCCESS)
    rep.frontOcc = 0;
  Residency res = residency(in, rep);
  // A store is sized again only when its size changes; an engine that refuses (e.g. the CPU test build) takes the store
  // away from all of them: every job ships its tables / its constraint set, as with the switch off.
  auto reserveOnAll = [&](auto reserve) {  // reserve(engine, on)
    for (int32_t t = 0; t < nAll; ++t)
      if (reserve(s->engines[t], true) != MRP_LL_SUCCESS) {
        for (int32_t u = 0; u <= t; ++u) (void)reserve(s->engines[u], false);
        return false;
      }
    return true;
  };
  if (res.pathStore && res.pathSlots != s->pathSlots) {
    if (!reserveOnAll([&](mrp_ll_ctx* e, bool on) { return mrp_ll_path_store_reserve(e, on ? res.pathSlots : 0); })) res.pathSlots = 0;
    s->pathSlots = res.pathSlots;
  }
  if (res.consStore && (res.consSlots != s->consSlots || res.consWords != s->consWords)) {
    if (!reserveOnAll([&](mrp_ll_ctx* e, bool on) { return reserveConstraintStore(e, on ? res.consSlots : 0, on ? res.consWords : 0); }))
      res.consSlots = res.consWords = 0;
    s->consSlots = res.consSlots;
    s->consWords = res.consWords;
  }

  std::atomic<int32_t> nextInstance(0);
  int32_t sessionGate = 0;
  const int32_t nWork = res.nWork;
  std::vector<GroupResult> gr(static_cast<size_t>(nWork));
  auto t0 = std::chrono::steady_clock::now();
  {
    SessionPlan plan;
    plan.opt = opt;
    plan.horizon = horizon;
    plan.workgroups = res.sessionWgs;
    plan.heavyWgs = res.heavyPer;
    plan.pathSlots = res.pathSlots;
    plan.consSlots = res.consSlots;
    plan.consWords = res.consWords;
    plan.gate = &sessionGate;
    plan.nEngines = nRun;
    plan.nWorkers = nWork;
    plan.view = &view;
    plan.pool = sharedPool ? &nextInstance : nullptr;
    plan.epoch = t0;
    plan.knobs = in.knobs;
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
    st.incremental_scans += g.incrementalScans;
    st.build_seconds += g.buildS;
    st.ll_call_seconds += g.llS;
    st.consume_seconds += g.consumeS;
  }
  for (int32_t b = 0; b < nBatches; ++b)
    for (int32_t k = 0; k < pres[b]->nInst; ++k) st.solved += solsArr[b][k].status == MRP_HL_SOLVED ? 1 : 0;
  if (stats) *stats = st;
  return MRP_LL_SUCCESS;
}

int mrp_hl_solver_prioritized_sipp(mrp_hl_solver* s, int32_t nInst, const mrp_hl_instance* instances,
                                   mrp_hl_sipp_solution* sols, mrp_hl_batch_stats* stats) {
  if (!s || nInst < 0 || (nInst > 0 && (!instances || !sols))) return MRP_LL_E_INVALID;
  return prioritizedSipp(s->engines, s->llOpt, nInst, instances, sols, stats, s->err);
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

// mrp_hl.h: mrp_hl_solve_batch's contract with every search under MRP_LL_JOB_TABLE_H.  The rounds schedule whatever opt->mode
// says (the session schedule opens one-algorithm sessions, which take no such job); maps and tables are on the engines before
// the timed region starts: one mrp_ll_compute_heuristics per engine for the goals of all agents of that engine's instances.
int mrp_hl_solve_batch_table_h(int32_t device, const mrp_hl_options* optIn, int32_t nInst, const mrp_hl_instance* instances,
                               mrp_hl_solution* solutions, mrp_hl_batch_stats* stats) {
  if (!optIn || nInst < 0 || (nInst > 0 && (!instances || !solutions))) return MRP_LL_E_INVALID;
  if (&mrp_ll_compute_heuristics == nullptr) {
    std::fprintf(stderr, "mrp_hl_solve_batch_table_h: the low-level library has no mrp_ll_compute_heuristics\n");
    return MRP_LL_E_INVALID;
  }
  mrp_hl_options opt = *optIn;
  opt.mode = 1;
  mrp_hl_solver* s = nullptr;
  int rc = mrp_hl_solver_create(device, opt.n_threads, nullptr, &s);
  if (rc != MRP_LL_SUCCESS) return rc;
  mrp_hl_preloaded* pre = nullptr;
  rc = mrp_hl_solver_preload(s, opt.n_threads, nInst, instances, &pre);
  if (rc != MRP_LL_SUCCESS) {
    std::fprintf(stderr, "mrp_hl_solve_batch_table_h: %s\n", s->err.c_str());
    mrp_hl_solver_destroy(s);
    return rc;
  }
  const int32_t nRun = static_cast<int32_t>(pre->idx.size());
  std::vector<int64_t> agentFirst(static_cast<size_t>(nInst) + 1, 0);
  for (int32_t k = 0; k < nInst; ++k) agentFirst[k + 1] = agentFirst[k] + std::max(instances[k].n_agents, 0);
  const int64_t nTables = agentFirst[nInst];
  std::vector<std::vector<int32_t>> heurIds(static_cast<size_t>(nRun));
  std::vector<int> rcs(static_cast<size_t>(nRun), MRP_LL_SUCCESS);
  if (nTables > INT32_MAX) rc = MRP_LL_E_INVALID;
  if (rc == MRP_LL_SUCCESS) {
    std::vector<int32_t> goals(static_cast<size_t>(nTables) * 2);
    for (int32_t k = 0; k < nInst; ++k)
      if (instances[k].n_agents > 0)
        std::memcpy(goals.data() + agentFirst[k] * 2, instances[k].goals_xy, sizeof(int32_t) * 2 * static_cast<size_t>(instances[k].n_agents));
    std::vector<std::thread> th;
    for (int32_t t = 0; t < nRun; ++t)
      th.emplace_back([&, t]() {
        // the tables of THIS engine's instances (the rounds schedule's static split), one launch
        std::vector<int32_t> mapIds, goalsT, ids;
        for (int32_t k : pre->idx[t])
          for (int64_t q = agentFirst[k]; q < agentFirst[k + 1]; ++q) {
            mapIds.push_back(pre->mapBase[t] + k);
            goalsT.push_back(goals[2 * q]);
            goalsT.push_back(goals[2 * q + 1]);
          }
        ids.assign(mapIds.size(), -1);
        rcs[t] = mrp_ll_compute_heuristics(s->engines[t], static_cast<int32_t>(mapIds.size()), mapIds.data(), goalsT.data(), ids.data());
        heurIds[t].assign(static_cast<size_t>(nTables), -1);
        size_t n = 0;
        for (int32_t k : pre->idx[t])
          for (int64_t q = agentFirst[k]; q < agentFirst[k + 1]; ++q) heurIds[t][q] = ids[n++];
      });
    for (auto& x : th) x.join();
    for (int32_t t = 0; t < nRun && rc == MRP_LL_SUCCESS; ++t)
      if (rcs[t] != MRP_LL_SUCCESS) {  // MRP_LL_E_NOMEM: the tables do not fit the maps buffer — no fall-back to Manhattan
        rc = rcs[t];
        std::fprintf(stderr, "mrp_hl_solve_batch_table_h: %s\n", llError("mrp_ll_compute_heuristics", s->engines[t]).c_str());
      }
  }
  if (rc == MRP_LL_SUCCESS) {
    const int32_t horizon = s->llOpt.max_horizon > 0 ? s->llOpt.max_horizon : 512;
    std::vector<GroupResult> gr(static_cast<size_t>(nRun));
    auto t0 = std::chrono::steady_clock::now();
    {
      std::vector<std::thread> th;
      for (int32_t t = 0; t < nRun; ++t)
        th.emplace_back([&, t]() {
          pinWorker(t);
          runGroup(s->engines[t], opt, instances, solutions, pre->idx[t], pre->mapBase[t], horizon, gr[t], heurIds[t].data(),
                   agentFirst.data());
        });
      for (auto& x : th) x.join();
    }
    auto t1 = std::chrono::steady_clock::now();
    mrp_hl_batch_stats st;
    std::memset(&st, 0, sizeof(st));
    st.wall_seconds = std::chrono::duration<double>(t1 - t0).count();
    for (auto& g : gr) {
      if (!g.err.empty()) {
        std::fprintf(stderr, "mrp_hl_solve_batch_table_h: %s\n", g.err.c_str());
        rc = MRP_LL_E_DEVICE;
        break;
      }
      st.rounds += g.rounds;
      st.ll_searches += g.searches;
      st.ll_expansions += g.expansions;
      st.build_seconds += g.buildS;
      st.ll_call_seconds += g.llS;
      st.consume_seconds += g.consumeS;
    }
    if (rc == MRP_LL_SUCCESS) {
      for (int32_t k = 0; k < nInst; ++k) st.solved += solutions[k].status == MRP_HL_SOLVED ? 1 : 0;
      if (stats) *stats = st;
    }
  }
  mrp_hl_preloaded_free(pre);
  mrp_hl_solver_destroy(s);
  return rc;
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
