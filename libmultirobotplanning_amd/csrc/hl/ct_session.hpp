// The CBS / ECBS session driver (mrp_hl.h mrp_hl_solver_solve_stream, mode 0) and the helpers it shares with the other
// drivers (rounds_driver.hpp, sipp_drivers.hpp, ct_stepped.hpp; mrp_hl.cpp includes them all).  One SessionWorker per host
// thread: it keeps its engine's resident kernel fed through the job ring, draws instances from an InstanceSource and
// publishes an instance's next searches the moment its previous ones are back.  What one solve call fixes for every
// worker is a SessionPlan (sized by launch_plan.hpp, knobs from solve_knobs.hpp), what differs per thread a WorkerSeat.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mrp_hl.h"
#include "ct_solver.hpp"
#include "solve_knobs.hpp"

namespace mrp_hl {

typedef std::chrono::steady_clock::time_point TimePoint;
inline TimePoint clockNow() { return std::chrono::steady_clock::now(); }
inline double secondsBetween(TimePoint a, TimePoint b) { return std::chrono::duration<double>(b - a).count(); }

// A session loop gives up when nothing at all has come back for this long (a dead resident kernel is reported much
// sooner by mrp_ll_poll_any's own liveness check).
constexpr double kNoProgressLimitS = 600.0;
struct ProgressWatchdog {
  uint64_t idleSpins = 0;
  bool sinceProgress = false;
  TimePoint lastProgress;
  // One turn of a session loop; false: the limit has passed.  It measures the time since the LAST progress, not since
  // the start of the batch, and reads the clock only every 65 536th idle turn.
  bool turn(bool progress) {
    if (progress) {
      idleSpins = 0;
      sinceProgress = false;
    } else if ((++idleSpins & 0xFFFF) == 0) {
      const TimePoint t = clockNow();
      if (!sinceProgress) {
        sinceProgress = true;
        lastProgress = t;
      } else if (secondsBetween(lastProgress, t) > kNoProgressLimitS) {
        return false;
      }
    }
    return true;
  }
};

// Two workers on one engine ("co-workers", mrp_ll.h mrp_ll_submit_tagged): the leader (index 0) begins and ends the
// session, the other one waits for it on both sides.
struct CoSync {
  std::atomic<int32_t> begun{0};     // 1: the session runs, -1: it could not be started
  std::atomic<int32_t> finished{0};  // co-workers that have left their loops
};

// "<call>: <the engine's last error>", what every driver reports when a call of the low-level engine fails
inline std::string llError(const char* call, const mrp_ll_ctx* ctx) { return std::string(call) + ": " + mrp_ll_last_error(ctx); }

struct GroupResult {
  int64_t rounds = 0, searches = 0, expansions = 0;  // expansions: of the searches the conflict trees CONSUMED
  int64_t specSearches = 0, specWasted = 0;          // searches issued ahead of their node's pop; expansions that were run but never consumed
  int64_t rootSolved = 0;                            // instances whose root node was conflict-free, written out without a conflict tree
  int64_t deviceScans = 0;                           // conflict-tree nodes whose conflicts came with their low-level search
  int64_t incrementalScans = 0;                      // ... those scanned from what their parent's scan established (mrp_ll_submit_node)
  double buildS = 0, llS = 0, consumeS = 0;
  std::string err;
};

// Several preloaded batches as ONE pool of instances (mrp_hl.h mrp_hl_solver_solve_stream): global index k names instance
// k - first[b] of batch b; its map id on engine e is mapBase[b][e] + that.
struct StreamView {
  std::vector<int32_t> first;                      // first[b] = global index of batch b's instance 0; first[nBatches] = total
  std::vector<const mrp_hl_instance*> inst;        // per batch
  std::vector<mrp_hl_solution*> sols;              // per batch
  std::vector<const std::vector<int32_t>*> mapBase;  // per batch: per engine
  int32_t total() const { return first.back(); }
  int32_t batchOf(int32_t k) const {
    return static_cast<int32_t>(std::upper_bound(first.begin(), first.end(), k) - first.begin()) - 1;
  }
  mrp_hl_solution& sol(int32_t k) const {
    const int32_t b = batchOf(k);
    return sols[b][k - first[b]];
  }
};

// Where a worker's next instance comes from: one counter shared by all workers (a worker whose instances turn out easy
// takes more of them) or, with MRP_HL_STATIC_SPLIT, the worker's own list.  Either way the indices only grow, so the
// batch of the next instance is found by walking forward.
struct InstanceSource {
  const StreamView* view = nullptr;
  std::atomic<int32_t>* pool = nullptr;      // the shared counter (nullptr: static split)
  const std::vector<int32_t>* own = nullptr;  // static split: this worker's instances, ascending
  int32_t engineIdx = 0;
  size_t nextOwn = 0;  // static split: position in `own`
  int32_t batch = 0;   // of the instance handed out last
  struct Item {
    int32_t g = 0;  // global index (StreamView)
    const mrp_hl_instance* inst = nullptr;
    int32_t mapId = 0;  // on this worker's engine
  };
  bool next(Item& it) {
    if (pool) {
      it.g = pool->fetch_add(1, std::memory_order_relaxed);
      if (it.g >= view->total()) return false;
    } else {
      if (nextOwn >= own->size()) return false;
      it.g = (*own)[nextOwn++];
    }
    while (it.g >= view->first[batch + 1]) ++batch;
    const int32_t k = it.g - view->first[batch];
    it.inst = view->inst[batch] + k;
    it.mapId = (*view->mapBase[batch])[engineIdx] + k;
    return true;
  }
};

// Low-level jobs of the C-ABI whose focal-context arrays live in pools: add() the jobs, then patch() the pointers in (the
// pools may reallocate while they grow).
struct JobBatch {
  std::vector<mrp_ll_job> jobs;
  std::vector<int32_t> pathLenPool, idPool;
  std::vector<const int32_t*> pathPtrPool;
  std::vector<size_t> poolOff;  // per job: where its context starts in the pools
  std::vector<uint8_t> idOk;  // per job: every context path it needs has a device path-store slot
  std::vector<uint8_t> ownOk;  // per job: ... and the path it replaces has one too, and is named in the searching agent's entry
  void clear() {
    ownOk.clear();
    jobs.clear();
    pathLenPool.clear();
    idPool.clear();
    pathPtrPool.clear();
    poolOff.clear();
    idOk.clear();
  }
  // One job for request `r` of instance `I`.  `withIds`: also name the context paths by their device path-store slots (f2).
  // `withOwn`: the searching agent's entry names the slot of the path the search replaces (mrp_ll_submit_node; every other
  // entry point ignores that entry).
  mrp_ll_job& add(const Instance& I, const LLRequest& r, bool withIds = false, bool withOwn = false) {
    jobs.emplace_back();
    mrp_ll_job& j = jobs.back();
    std::memset(&j, 0, sizeof(j));
    j.map_id = I.mapId();
    j.algo = I.algo() == MRP_HL_ECBS ? MRP_LL_ASTAR_EPS : MRP_LL_ASTAR;
    j.w = I.w();
    j.agent_idx = r.agent;
    j.start_x = I.start(r.agent)[0];
    j.start_y = I.start(r.agent)[1];
    j.goal_x = I.goal(r.agent)[0];
    j.goal_y = I.goal(r.agent)[1];
    j.n_vertex_constraints = static_cast<int32_t>(r.constraints->vertex.size() / 3);
    j.vertex_constraints = r.constraints->vertex.data();
    j.n_edge_constraints = static_cast<int32_t>(r.constraints->edge.size() / 5);
    j.edge_constraints = r.constraints->edge.data();
    j.max_expansions = I.remainingLL();
    j.result_path_id = -1;
    poolOff.push_back(pathLenPool.size());
    bool all = false, own = false;
    if (r.context) {
      j.n_agents = static_cast<int32_t>(r.context->size());
      all = withIds;
      int32_t a = 0;
      for (const PathPtr& p : *r.context) {
        pathLenPool.push_back(p->len());
        pathPtrPool.push_back(p->xy.data());
        if (withIds) {
          const bool needed = a != r.agent && p->len() > 0;
          idPool.push_back(needed ? p->devSlot : -1);
          if (needed && p->devSlot < 0) all = false;
        }
        ++a;
      }
      if (withOwn && all && r.replaced && r.parentCount >= 0 && r.cleanBefore >= 0) {
        // (the context still holds the parent's path of the searching agent: the one this search replaces)
        const PathPtr& p = (*r.context)[r.agent];
        own = p.get() == r.replaced && p->len() > 0 && p->devSlot >= 0;
        if (own) idPool[poolOff.back() + static_cast<size_t>(r.agent)] = p->devSlot;
      }
    }
    idOk.push_back(all ? 1 : 0);
    ownOk.push_back(all && own ? 1 : 0);
    return j;
  }
  void patch() {
    for (size_t q = 0; q < jobs.size(); ++q)
      if (jobs[q].n_agents > 0) {
        jobs[q].path_len = pathLenPool.data() + poolOff[q];
        jobs[q].path_xy = pathPtrPool.data() + poolOff[q];
        if (idOk[q]) jobs[q].path_ids = idPool.data() + poolOff[q];
      }
  }
};

// mrp_ll_submit_scan through a weak reference: a low-level library without it (an older engine, the CPU tests' stand-in)
// still loads, and the driver keeps scanning on the host.
extern "C" __attribute__((weak)) int mrp_ll_submit_scan(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs,
                                                        mrp_ll_result* results, mrp_ll_conflict* conflicts, int32_t* ticket);

// mrp_ll_submit_sets likewise: without it (or without mrp_ll_constraint_store_reserve) every job ships its whole
// constraint set, as before.
extern "C" __attribute__((weak)) int mrp_ll_submit_sets(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs,
                                                        mrp_ll_result* results, mrp_ll_conflict* conflicts,
                                                        const mrp_ll_constraint_ref* sets, int32_t* ticket);
extern "C" __attribute__((weak)) int mrp_ll_constraint_store_reserve(mrp_ll_ctx* ctx, int32_t n_slots, int32_t words_per_slot);
// mrp_ll_submit_node likewise: without it MRP_HL_DEVICE_SCAN_INCREMENTAL changes nothing.
extern "C" __attribute__((weak)) int mrp_ll_submit_node(mrp_ll_ctx* ctx, int32_t tag, int32_t n_jobs, const mrp_ll_job* jobs,
                                                        mrp_ll_result* results, mrp_ll_conflict* conflicts,
                                                        const mrp_ll_constraint_ref* sets, const mrp_ll_scan_base* bases, int32_t* ticket);
inline bool engineHasConstraintStore() { return &mrp_ll_submit_sets != nullptr && &mrp_ll_constraint_store_reserve != nullptr; }
// mrp_ll_constraint_store_reserve, or MRP_LL_E_INVALID on an engine without it
inline int reserveConstraintStore(mrp_ll_ctx* ctx, int32_t nSlots, int32_t wordsPerSlot) {
  return engineHasConstraintStore() ? mrp_ll_constraint_store_reserve(ctx, nSlots, wordsPerSlot) : MRP_LL_E_INVALID;
}

// Zeroes `n` results and gives each its own `cap` states of `states`.
inline void bindResults(mrp_ll_result* res, size_t n, std::vector<int32_t>& states, int32_t cap) {
  states.resize(n * static_cast<size_t>(cap) * 3);
  for (size_t q = 0; q < n; ++q) {
    std::memset(&res[q], 0, sizeof(mrp_ll_result));
    res[q].states_txy = states.data() + q * static_cast<size_t>(cap) * 3;
    res[q].states_cap = cap;
  }
}

// `slot` / `pool`: the path-store slot the job was given for its result path (-1: none)
inline LLAnswer answerOf(const mrp_ll_result& r, int32_t slot = -1, SlotPool* pool = nullptr) {
  LLAnswer a;
  a.status = r.status;
  a.cost = r.cost;
  a.fmin = r.fmin;
  a.expanded = r.expanded;
  if (r.status == MRP_LL_OK) {
    auto p = std::make_shared<Path>();
    p->xy.resize(static_cast<size_t>(r.n_states) * 2);
    uint32_t orAll = 0;
    for (int32_t s = 0; s < r.n_states; ++s) {
      p->xy[2 * s] = r.states_txy[3 * s + 1];
      p->xy[2 * s + 1] = r.states_txy[3 * s + 2];
      orAll |= static_cast<uint32_t>(p->xy[2 * s]) | static_cast<uint32_t>(p->xy[2 * s + 1]);
    }
    p->fits8 = orAll < 256u;
    if (p->fits8) p->packCells();
    p->cost = r.cost;
    p->fmin = r.fmin;
    if (pool && slot >= 0) {
      p->devSlot = slot;
      p->pool = pool;
    }
    a.path = p;
  } else if (pool) {
    pool->give(slot);  // no path came out of this search
  }
  return a;
}

// mrp_hl_solution.schedule_digest: FNV-1a over the low byte of every x and y, 0xFF behind every agent's path
struct ScheduleDigest {
  uint64_t h = 14695981039346656037ull;
  void byte(uint32_t b) { h = (h ^ (b & 0xFFu)) * 1099511628211ull; }
  void cell(uint32_t x, uint32_t y) {
    byte(x);
    byte(y);
  }
  void endOfPath() { byte(0xFFu); }
};

inline void writeSolution(const Instance& I, mrp_hl_solution& s) {
  s.status = I.status();
  s.n_ll_searches = I.llSearches();
  s.high_level_expanded = I.hlExpanded();
  s.low_level_expanded = I.llExpanded();
  s.cost = 0;
  s.makespan = 0;
  s.schedule_digest = 0;
  if (I.status() != MRP_HL_SOLVED) return;
  const auto& sol = I.finalSolution();
  ScheduleDigest d;
  for (int32_t a = 0; a < I.nAgents(); ++a) {
    const int32_t* q = sol[a]->xy.data();
    const int32_t n = sol[a]->len();
    for (int32_t k = 0; k < n; ++k) d.cell(static_cast<uint32_t>(q[2 * k]), static_cast<uint32_t>(q[2 * k + 1]));
    d.endOfPath();
    s.cost += sol[a]->cost;
    s.makespan = std::max<int64_t>(s.makespan, sol[a]->cost);
    if (s.path_len) s.path_len[a] = n;
    if (s.paths_xy)
      std::memcpy(s.paths_xy + static_cast<size_t>(a) * s.path_cap * 2, q, sizeof(int32_t) * 2 * std::min(n, s.path_cap));
  }
  s.schedule_digest = d.h;
}

// The solution of an instance whose ROOT node has no conflict, written straight from the results of its root chain
// (mrp_ll.h MRP_LL_JOB_ROOT_CHAIN: the workgroup that planned the agents also scanned their paths): what ECBS::search
// returns when the first node it pops is conflict-free (ecbs.hpp:227-240) — cost = sum of the agents' costs, one
// high-level expansion — without building a single conflict-tree object.  Returns the searches' expansions.
inline int64_t writeRootSolution(const std::vector<mrp_ll_result>& r, mrp_hl_solution& s) {
  s.status = MRP_HL_SOLVED;
  s.n_ll_searches = static_cast<int32_t>(r.size());
  s.high_level_expanded = 1;
  s.low_level_expanded = 0;
  s.cost = 0;
  s.makespan = 0;
  ScheduleDigest d;
  for (size_t a = 0; a < r.size(); ++a) {
    s.cost += r[a].cost;
    s.makespan = std::max<int64_t>(s.makespan, r[a].cost);
    s.low_level_expanded += r[a].expanded;
    const int32_t n = r[a].n_states;
    const int32_t* q = r[a].states_txy;
    if (s.path_len) s.path_len[a] = n;
    int32_t* dst = s.paths_xy ? s.paths_xy + a * static_cast<size_t>(s.path_cap) * 2 : nullptr;
    for (int32_t k = 0; k < n; ++k) {
      d.cell(static_cast<uint32_t>(q[3 * k + 1]), static_cast<uint32_t>(q[3 * k + 2]));
      if (dst && k < s.path_cap) {
        dst[2 * k] = q[3 * k + 1];
        dst[2 * k + 1] = q[3 * k + 2];
      }
    }
    d.endOfPath();
  }
  s.schedule_digest = d.h;
  return s.low_level_expanded;
}

// What one solve call fixes for all of its session workers (launch_plan.hpp decides the sizes, mrp_hl.cpp fills this in).
struct SessionPlan {
  mrp_hl_options opt;
  int32_t horizon = 0;     // states a result path may have
  int32_t workgroups = 0;  // resident (front) wavefronts per engine
  int32_t heavyWgs = 0;    // ECBS: heavy workgroups per engine, which take over the searches that outgrow the LDS tier
  int32_t pathSlots = 0;   // slots of every engine's device path store (0: jobs ship their context as tables)
  int32_t consSlots = 0, consWords = 0;  // the constraint store every engine reserved (0: none, sets ship flat)
  int32_t* gate = nullptr;  // mrp_ll_session_begin_tiers_gated: every worker's heavy launch before anybody's front launch
  int32_t nEngines = 1, nWorkers = 1;
  const StreamView* view = nullptr;
  std::atomic<int32_t>* pool = nullptr;  // the instance counter all workers draw from (nullptr: static split)
  TimePoint epoch;                       // MRP_HL_TIMING only: the moment the solve call started
  SolveKnobs knobs;                      // the environment knobs, read once per call (solve_knobs.hpp)
};

// One worker thread's place in the call: its engine and, when two workers share that engine, which of the two it is.
struct WorkerSeat {
  mrp_ll_ctx* ctx = nullptr;
  int32_t engineIdx = 0;
  int32_t coIndex = 0, coCount = 1;
  CoSync* co = nullptr;                       // coCount > 1 only
  const std::vector<int32_t>* own = nullptr;  // static split only: this worker's instances
};

// Session mode: the engine keeps `workgroups` wavefronts resident (mrp_ll_session_begin_tiers_gated) and every instance
// submits its next searches the moment the ones they depend on have finished — no instance ever waits for another one's
// search.  Every group of requests (the two children of one CT node, or a root step) is one ticket.  While fewer searches
// are in flight than the engine has resident wavefronts, the conflict-tree machines look ahead (ct_solver.hpp,
// "speculative expansion"): idle wavefronts pre-compute the children of the nodes that will probably be popped next.
class SessionWorker {
 public:
  SessionWorker(const SessionPlan& plan, const WorkerSeat& seat, GroupResult& out)
      : plan_(plan), seat_(seat), out_(out), tagged_(seat.coCount > 1 && seat.co != nullptr),
        rootChains_(plan.pathSlots > 0 && plan.opt.algo == MRP_HL_ECBS && plan.knobs.rootChains),
        scanFromParent_(plan.knobs.deviceScanIncremental && plan.pathSlots > 0 && plan.opt.algo == MRP_HL_ECBS &&
                        &mrp_ll_submit_node != nullptr),
        deviceScan_(scanFromParent_ ||
                    (plan.knobs.deviceScan && plan.pathSlots > 0 && plan.opt.algo == MRP_HL_ECBS && &mrp_ll_submit_scan != nullptr)),
        deviceCons_(plan.consSlots > 0 && plan.consWords > 0),  // (reserved only with MRP_HL_DEVICE_CONSTRAINTS on an engine that has the store)
        // this worker's share of the engine's resident wavefronts
        myWorkgroups_(std::max(1, plan.workgroups / std::max(seat.coCount, 1))),
        source_{plan.view, plan.pool, seat.own, seat.engineIdx} {
    tm_.on = plan.knobs.timing;
    const int32_t share = plan.pathSlots / seat.coCount;  // co-workers split the engine's path store
    slotPool_.next = tagged_ ? seat.coIndex * share : 0;
    slotPool_.cap = tagged_ ? slotPool_.next + share : plan.pathSlots;
    const int32_t consShare = plan.consSlots / seat.coCount;  // ... and its constraint store
    consPool_.next = tagged_ ? seat.coIndex * consShare : 0;
    consPool_.cap = !deviceCons_ ? 0 : tagged_ ? consPool_.next + consShare : plan.consSlots;
    ringTarget_ = plan.knobs.ringDepth > 0 ? plan.knobs.ringDepth : std::max<int64_t>(2 * static_cast<int64_t>(myWorkgroups_), 32);
    // Admission control: at most `activeLimit_` instances of this worker are active at a time; the rest wait in the pool.
    // With the job slots recycled in completion order it costs nothing (measured 1536..3584 at the bench shape: same step
    // time as "everything at once"), and with a shared pool it is what lets the workers balance: no worker may hold more
    // than its fair share at a time, or a small batch is drained by the first few.
    const size_t nW = static_cast<size_t>(std::max(plan.nWorkers, 1));
    activeLimit_ = plan.pool ? std::max<size_t>(1, std::min<size_t>(16384, (static_cast<size_t>(plan.view->total()) + nW - 1) / nW))
                             : seat.own->size();
    if (plan.knobs.activeLimit > 0) activeLimit_ = static_cast<size_t>(plan.knobs.activeLimit);
  }

  void run() {
    tm_.tg0 = clockNow();
    if (!begin()) return;
    tm_.tg1 = tm_.tg2 = clockNow();
    const bool ok = loop();
    tm_.tg3 = clockNow();
    end();
    tm_.tg4 = clockNow();
    finish(ok);
  }

 private:
  struct Live {
    std::unique_ptr<Instance> inst;  // empty once the instance has been retired
    std::vector<LLRequest> req;   // not submitted yet: req[reqHead..)
    size_t reqHead = 0;
    bool queued = false;          // in `backlog_`
    bool counted = false;         // its completion has been taken off nActive_
    double tAdmit = 0, tDone = 0;  // MRP_HL_TIMING only: seconds since the worker started
    int32_t noChainAgent = -1;    // root agent whose search outgrew the compact tier inside a chain: it goes as its own job
    int64_t hl = 0, ll = 0, spec = 0;  // ... and what the instance had consumed when it was retired
    int32_t searches = 0;
  };
  struct Pending {                // one ticket in flight
    size_t live = 0;
    int32_t group = 0;
    std::vector<mrp_ll_result> res;
    std::vector<int32_t> states;
    std::vector<int32_t> outSlot;  // per job: the path-store slot its result path also goes to (-1: none)
    std::vector<mrp_ll_conflict> conf;  // per job, when the ticket went through mrp_ll_submit_scan (else empty): its node's conflicts
    // per job, when some job of the ticket names its constraint set by slot (mrp_ll_submit_sets; else empty) — and the sets
    // those jobs name: a set (and with it its slot) outlives every unfinished job that reads or writes the slot
    std::vector<mrp_ll_constraint_ref> sets;
    std::vector<ConsPtr> consHold;
    // per job, when the ticket went through mrp_ll_submit_node (else empty): what the parent's scan established; the paths
    // the jobs replace stay alive, and with them their slots, until the ticket is back
    std::vector<mrp_ll_scan_base> bases;
    std::vector<PathPtr> replacedHold;
    std::vector<uint8_t> flagged;  // per job: it carried MRP_LL_JOB_SCAN_FROM_PARENT
    bool fromParent(size_t q) const { return q < flagged.size() && flagged[q] != 0; }
    // a root chain (MRP_LL_JOB_ROOT_CHAIN): ONE job whose result fans out into chainRes, one per agent from chainFirst on
    std::vector<mrp_ll_result> chainRes;
    int32_t chainFirst = -1;
    int32_t chainCount = 0;           // agents the job was asked to plan (MRP_LL_NOT_RUN behind them is not a tier overflow)
    std::vector<LLRequest> chainReq;  // the request the chain was made from (restored if the chain ran nothing)
  };
  // MRP_HL_TIMING: where this worker's time went
  struct Timing {
    bool on = false;
    TimePoint tg0, tg1, tg2, tg3, tg4;
    double submit = 0, pollEmpty = 0, pollHit = 0, unpack = 0, advance = 0;
    uint64_t nPollEmpty = 0, nPollHit = 0;
    TimePoint clock() const { return on ? clockNow() : TimePoint(); }  // (per-ticket clock reads only when somebody will look at them)
    double sinceStart() const { return secondsBetween(tg0, clockNow()); }
    static double ms(TimePoint a, TimePoint b) { return secondsBetween(a, b) * 1e3; }
    void report(mrp_ll_ctx* ctx, const std::deque<Live>& live, const std::vector<int32_t>& gidx, const GroupResult& out) const {
      mrp_ll_stats ls;
      mrp_ll_get_stats(ctx, &ls);
      std::fprintf(stderr, "[mrp_hl] group of %zu: session_begin %.2f ms, build instances %.2f ms, loop %.2f ms, session_end %.2f ms; "
                   "cumulative: active wgs %lld, busy %.0f ms, idle %.0f ms, heavy wgs %lld busy %.0f ms idle %.0f ms, searches %lld, "
                   "expansions %lld\n", live.size(),
                   ms(tg0, tg1), ms(tg1, tg2), ms(tg2, tg3), ms(tg3, tg4), (long long)ls.session_active_wgs,
                   ls.session_busy_ms, ls.session_idle_ms, (long long)ls.heavy_active_wgs, ls.heavy_busy_ms, ls.heavy_idle_ms,
                   (long long)ls.jobs, (long long)ls.expansions);
      std::fprintf(stderr, "[mrp_hl]   host ms: admit+submit %.1f, poll empty %.1f (%llu), poll hit %.1f (%llu), "
                   "unpack %.1f, advance %.1f; tickets %lld searches %lld\n", submit * 1e3, pollEmpty * 1e3,
                   (unsigned long long)nPollEmpty, pollHit * 1e3, (unsigned long long)nPollHit, unpack * 1e3,
                   advance * 1e3, (long long)out.rounds, (long long)out.searches);
      std::vector<size_t> order(live.size());  // the instances this worker finished last
      for (size_t k = 0; k < order.size(); ++k) order[k] = k;
      std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return live[a].tDone > live[b].tDone; });
      for (size_t q = 0; q < std::min<size_t>(3, order.size()); ++q) {
        const Live& L = live[order[q]];
        std::fprintf(stderr, "[mrp_hl]     last #%zu: instance %d admitted %.1f ms done %.1f ms, HL %lld, LL %lld, searches %d (+%lld ahead)\n", q,
                     gidx[order[q]], L.tAdmit * 1e3, L.tDone * 1e3, (long long)L.hl, (long long)L.ll, L.searches,
                     (long long)L.spec);
      }
    }
    void reportFreed(TimePoint epoch, TimePoint written, TimePoint freed) const {
      std::fprintf(stderr, "[mrp_hl]   thread began %.1f ms after the batch, loop ended at %.1f ms, solutions written at %.1f ms, "
                   "instances freed at %.1f ms\n", ms(epoch, tg0), ms(epoch, tg3), ms(epoch, written), ms(epoch, freed));
    }
  };

  bool leader() const { return !tagged_ || seat_.coIndex == 0; }
  bool fail(const std::string& what) {
    out_.err = what;
    return false;
  }
  bool failLL(const char* call) { return fail(llError(call, seat_.ctx)); }

  // ECBS: front workgroups (the LDS tier alone) + heavy workgroups that take over the searches that outgrow it; all
  // workers' heavy launches go first (the gate), then the front ones (mrp_ll.h mrp_ll_session_begin_tiers_gated).  The
  // leader of an engine starts its session and says so; a co-worker waits for that.
  bool begin() {
    const bool ecbs = plan_.opt.algo == MRP_HL_ECBS;
    if (leader()) {
      const int rc = mrp_ll_session_begin_tiers_gated(seat_.ctx, ecbs ? MRP_LL_ASTAR_EPS : MRP_LL_ASTAR, plan_.workgroups,
                                                      ecbs ? plan_.heavyWgs : 0, plan_.gate, plan_.nEngines);
      if (seat_.co) seat_.co->begun.store(rc == MRP_LL_SUCCESS ? 1 : -1, std::memory_order_release);
      return rc == MRP_LL_SUCCESS || failLL("mrp_ll_session_begin_tiers");
    }
    int32_t b;
    while ((b = seat_.co->begun.load(std::memory_order_acquire)) == 0) std::this_thread::yield();
    return b > 0 || fail("the engine's session could not be started (see the leading worker)");
  }

  int32_t acquirePending(size_t k, int32_t group) {
    int32_t pi;
    if (!pendFree_.empty()) {
      pi = pendFree_.back();
      pendFree_.pop_back();
    } else {
      pend_.emplace_back();  // (a deque: the references to the other tickets stay valid)
      pi = static_cast<int32_t>(pend_.size()) - 1;
    }
    pend_[pi].live = k;
    pend_[pi].group = group;
    return pi;  // (chainFirst is -1: releasePending)
  }
  void releasePending(int32_t pi) {
    pend_[pi].chainFirst = -1;
    pend_[pi].conf.clear();
    pend_[pi].sets.clear();
    pend_[pi].consHold.clear();
    pend_[pi].bases.clear();
    pend_[pi].replacedHold.clear();
    pend_[pi].flagged.clear();
    pend_[pi].chainReq.clear();
    pendFree_.push_back(pi);
  }
  void giveSlots(const Pending& P, size_t from = 0) {
    for (size_t q = from; q < P.outSlot.size(); ++q) slotPool_.give(P.outSlot[q]);
  }

  // Hands the jobs of ticket `pi` to the engine.  Returns 1 published, 0 ring full (retry later), -1 error; unless
  // published, the ticket's path-store slots and the ticket itself have been taken back.
  int publish(int32_t pi, int32_t nJobs, const mrp_ll_job* jobs, const char* what) {
    Pending& P = pend_[pi];
    int32_t ticket = -1;
    const int rc = !P.bases.empty() ? mrp_ll_submit_node(seat_.ctx, tagged_ ? seat_.coIndex : 0, nJobs, jobs, P.res.data(), P.conf.data(),
                                                         P.sets.empty() ? nullptr : P.sets.data(), P.bases.data(), &ticket)
                   : !P.sets.empty() ? mrp_ll_submit_sets(seat_.ctx, tagged_ ? seat_.coIndex : 0, nJobs, jobs, P.res.data(),
                                                        P.conf.empty() ? nullptr : P.conf.data(), P.sets.data(), &ticket)
                   : !P.conf.empty() ? mrp_ll_submit_scan(seat_.ctx, tagged_ ? seat_.coIndex : 0, nJobs, jobs, P.res.data(), P.conf.data(), &ticket)
                   : tagged_      ? mrp_ll_submit_tagged(seat_.ctx, seat_.coIndex, nJobs, jobs, P.res.data(), &ticket)
                                  : mrp_ll_submit(seat_.ctx, nJobs, jobs, P.res.data(), &ticket);
    if (rc != MRP_LL_SUCCESS) {
      giveSlots(P);
      releasePending(pi);
      if (rc == MRP_LL_E_BUSY) return 0;
      failLL(what);
      return -1;
    }
    if (static_cast<size_t>(ticket) >= ticketPend_.size()) ticketPend_.resize(ticket + 1, -1);
    ticketPend_[ticket] = pi;
    ticketsOut_ += 1;
    jobsOut_ += nJobs;
    out_.rounds += 1;
    return 1;
  }

  // The root step of an ECBS tree goes out as a chain when the engine takes chains, the request is the only one waiting
  // and the agent count is one at which chains pay (SolveKnobs::chainChunkFrom).
  bool chainable(const Live& L) const {
    const Instance& I = *L.inst;
    const LLRequest& r = L.req[L.reqHead];
    return rootChains_ && r.group == kRootGroup && I.algo() == MRP_HL_ECBS && r.context && L.reqHead + 1 == L.req.size() &&
           I.nAgents() >= 2 && I.nAgents() <= 128 && (I.nAgents() <= 32 || I.nAgents() >= plan_.knobs.chainChunkFrom) &&
           r.agent != L.noChainAgent;
  }
  // The root step of an ECBS tree as ONE job (MRP_LL_JOB_ROOT_CHAIN): the workgroup plans this agent and every later one
  // against the paths before them and keeps the focal table in LDS; the host sees one completion instead of ten.  Only
  // when every existing path sits in the device store and there are slots for the new ones: kNoChain otherwise
  // (else as publish()).
  static constexpr int kNoChain = 2;
  int submitChain(size_t k) {
    Live& L = live_[k];
    const Instance& I = *L.inst;
    const LLRequest& r = L.req[L.reqHead];
    const int32_t nA = I.nAgents(), first = r.agent;
    chainIds_.assign(nA, -1);
    bool ok = true;
    for (int32_t a = 0; a < first && ok; ++a) {
      chainIds_[a] = (*r.context)[a]->devSlot;
      ok = chainIds_[a] >= 0;
    }
    for (int32_t a = first; a < nA && ok; ++a) {
      chainIds_[a] = slotPool_.take();
      ok = chainIds_[a] >= 0;
    }
    if (!ok) {
      for (int32_t a = first; a < nA; ++a) slotPool_.give(chainIds_[a]);
      return kNoChain;
    }
    chainXy_.resize(static_cast<size_t>(nA) * 4);
    for (int32_t a = 0; a < nA; ++a) {
      chainXy_[4 * a] = I.start(a)[0];
      chainXy_[4 * a + 1] = I.start(a)[1];
      chainXy_[4 * a + 2] = I.goal(a)[0];
      chainXy_[4 * a + 3] = I.goal(a)[1];
    }
    mrp_ll_job j;
    std::memset(&j, 0, sizeof(j));
    j.map_id = I.mapId();
    j.algo = MRP_LL_ASTAR_EPS;
    j.w = I.w();
    j.agent_idx = first;
    j.n_agents = nA;
    j.path_ids = chainIds_.data();
    j.chain_starts_goals_xy = chainXy_.data();
    j.max_expansions = I.remainingLL();
    j.result_path_id = -1;
    j.flags = MRP_LL_JOB_ROOT_CHAIN;
    // many agents: jobs of at most eight searches — a root step of fifty searches in ONE job holds its wavefront for
    // tens of milliseconds, and the two-search rounds of deep conflict trees queue behind such jobs (measured at fifty
    // agents: the step 26 % longer than with one job per root search)
    j.chain_count = nA >= plan_.knobs.chainChunkFrom ? plan_.knobs.chainChunk : 0;
    const int32_t pi = acquirePending(k, kRootGroup);
    Pending& P = pend_[pi];
    const int32_t cnt = nA - first;
    P.chainFirst = first;
    P.chainCount = j.chain_count > 0 ? std::min(j.chain_count, cnt) : cnt;
    P.outSlot.assign(chainIds_.begin() + first, chainIds_.end());
    P.chainRes.assign(static_cast<size_t>(cnt), mrp_ll_result());
    bindResults(P.chainRes.data(), P.chainRes.size(), P.states, plan_.horizon);
    P.res.assign(1, mrp_ll_result());
    std::memset(&P.res[0], 0, sizeof(mrp_ll_result));
    P.res[0].chain_results = P.chainRes.data();
    const int rc = publish(pi, 1, &j, "mrp_ll_submit (root chain)");
    if (rc == 1) {
      P.chainReq.assign(1, r);
      L.req.clear();
      L.reqHead = 0;
    }
    return rc;
  }
  // The first group of live_[k]'s unsent requests, one job per request (as publish()).
  int submitJobs(size_t k) {
    Live& L = live_[k];
    const int32_t group = L.req[L.reqHead].group;
    batch_.clear();
    size_t end = L.reqHead;
    for (; end < L.req.size() && L.req[end].group == group; ++end) {
      mrp_ll_job& j = batch_.add(*L.inst, L.req[end], plan_.pathSlots > 0, scanFromParent_ && group != kRootGroup);
      // a root search that ended a chain outgrows the LDS tier: no second attempt there
      if (group == kRootGroup && L.req[end].agent == L.noChainAgent) j.flags |= MRP_LL_JOB_HEAVY;
    }
    batch_.patch();
    std::vector<mrp_ll_job>& jobs = batch_.jobs;
    const int32_t pi = acquirePending(k, group);
    Pending& P = pend_[pi];
    P.outSlot.assign(jobs.size(), -1);
    if (plan_.pathSlots > 0)
      for (size_t q = 0; q < jobs.size(); ++q) {
        jobs[q].result_path_id = P.outSlot[q] = slotPool_.take();  // -1: store full, later jobs ship this path as a table
        if (P.outSlot[q] >= 0) jobs[q].flags |= MRP_LL_JOB_STORE_RESULT;
      }
    P.res.assign(jobs.size(), mrp_ll_result());
    bindResults(P.res.data(), jobs.size(), P.states, plan_.horizon);
    if (deviceScan_ && group != kRootGroup) {  // the children whose whole context is named by slot: their conflicts come back too
      bool any = false;
      for (size_t q = 0; q < jobs.size(); ++q)
        if (batch_.idOk[q]) {
          jobs[q].flags |= MRP_LL_JOB_SCAN_CONFLICTS;
          any = true;
        }
      if (any) P.conf.assign(jobs.size(), mrp_ll_conflict{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0});
      if (any && scanFromParent_) {
        P.bases.assign(jobs.size(), mrp_ll_scan_base{0, 0});
        P.flagged.assign(jobs.size(), 0);
        for (size_t q = 0; q < jobs.size(); ++q)
          if (batch_.ownOk[q]) {
            const LLRequest& r = L.req[L.reqHead + q];
            jobs[q].flags |= MRP_LL_JOB_SCAN_FROM_PARENT;
            P.bases[q] = mrp_ll_scan_base{r.parentCount, r.cleanBefore};
            P.replacedHold.push_back((*r.context)[r.agent]);
            P.flagged[q] = 1;
          }
      }
    }
    if (deviceCons_ && group != kRootGroup) nameSets(L, P, jobs);
    const int rc = publish(pi, static_cast<int32_t>(jobs.size()), jobs.data(), "mrp_ll_submit");
    if (rc != 1) {  // the sets that were given a slot for this attempt give it back (the ticket is gone: publish)
      for (const ConstraintSet* S : slotted_) {
        consPool_.give(S->devSlot);
        S->devSlot = -1;
        S->pool = nullptr;
        S->devWords = 0;
      }
    }
    slotted_.clear();
    if (rc == 1) {
      for (size_t q = L.reqHead; q < end; ++q) L.req[q].constraints->parent.reset();  // (the ticket holds what its jobs name)
      L.reqHead = end;
      if (L.reqHead == L.req.size()) {
        L.req.clear();
        L.reqHead = 0;
      }
      out_.searches += static_cast<int64_t>(jobs.size());
    }
    return rc;
  }

  // MRP_HL_DEVICE_CONSTRAINTS: the jobs of a conflict-tree node's children name their agents' constraint sets in the engine's
  // store.  A child's set S was made from its parent's set by one addition (ConstraintSet::parent, addVertex / addEdge):
  // the job names the parent's slot as its base, ships the addition and leaves the union in a fresh slot, which becomes
  // S's.  A parent without a slot (the root's empty set, a set that went flat) is no base: the job ships S whole, as today,
  // and still leaves it in a slot for S's own children.  The job goes flat, and S gets no slot, when the pool is empty or S
  // would not fit a slot (counted with duplicates, which the store keeps: an upper bound of the packed words).
  void nameSets(const Live& L, Pending& P, std::vector<mrp_ll_job>& jobs) {
    for (size_t q = 0; q < jobs.size(); ++q) {
      const ConstraintSet& S = *L.req[L.reqHead + q].constraints;
      if (S.devSlot >= 0) continue;  // (its search has been submitted before)
      const ConstraintSet* base = S.parent && S.parent->devSlot >= 0 ? S.parent.get() : nullptr;
      const int32_t words = base ? base->devWords + static_cast<int32_t>(S.addVertex.size() / 3 + S.addEdge.size() / 5)
                                 : static_cast<int32_t>(S.vertex.size() / 3 + S.edge.size() / 5);
      if (words > plan_.consWords) continue;
      const int32_t slot = consPool_.take();
      if (slot < 0) continue;
      S.devSlot = slot;
      S.pool = &consPool_;
      S.devWords = words;
      slotted_.push_back(&S);
      if (P.sets.empty()) P.sets.assign(jobs.size(), mrp_ll_constraint_ref{-1, -1});
      P.sets[q] = mrp_ll_constraint_ref{base ? base->devSlot : -1, slot};
      P.consHold.push_back(L.req[L.reqHead + q].constraints);
      jobs[q].flags |= MRP_LL_JOB_CONSTRAINT_SET;
      if (base) {
        P.consHold.push_back(S.parent);
        jobs[q].n_vertex_constraints = static_cast<int32_t>(S.addVertex.size() / 3);
        jobs[q].vertex_constraints = S.addVertex.data();
        jobs[q].n_edge_constraints = static_cast<int32_t>(S.addEdge.size() / 5);
        jobs[q].edge_constraints = S.addEdge.data();
      }
    }
  }

  // Scheduling.  The device queue is kept SHALLOW — at most `ringTarget_` searches published per worker, enough to hand
  // every resident wavefront its next job the moment it finishes one — and everything else waits in a host-side
  // priority queue.  An instance deep in its conflict tree (or stuck with one huge search) is a long chain of dependent
  // rounds; served first, each of its rounds starts within one job time instead of queueing behind thousands of searches
  // of easy instances, so the chain costs its compute time and not rounds x queue length (that, not throughput, bounded
  // a step before).  Fresh instances have priority 0 and are admitted only when nothing older is waiting.
  void enqueue(size_t k) {
    Live& L = live_[k];
    if (L.queued) return;
    L.queued = true;
    // priority: the work an instance has consumed so far, in searches — a long chain of tiny searches (a deadlocked
    // pair of agents grows its conflict tree by two 10-expansion searches per round, thousands of rounds deep) is as
    // latency-critical as one huge search, and its expansions alone would never say so
    backlog_.push(Waiting(L.inst->llExpanded() / 64 + L.inst->llSearches(), k));
  }
  // Submits groups of live_[k] while the device queue has room; false on error.  Leaves it in the backlog if some remain.
  bool submitAll(size_t k) {
    Live& L = live_[k];
    while (L.reqHead < L.req.size()) {
      int r = jobsOut_ >= ringTarget_ ? 0 : chainable(L) ? submitChain(k) : kNoChain;
      if (r == kNoChain) r = submitJobs(k);
      if (r < 0) return false;
      if (r == 0) {
        enqueue(k);
        return true;
      }
    }
    return true;
  }
  // Publishes the follow-up searches of live_[k] at once: a long conflict-tree chain must not wait for the rest of a
  // harvest pass.  false on error.
  bool followUp(size_t k) {
    Live& L = live_[k];
    return !(L.reqHead < L.req.size() && !L.queued) || submitAll(k);
  }

  // look ahead only while the engine has idle wavefronts: speculative searches must not queue in front of real ones
  int32_t specNow() const { return jobsOut_ < static_cast<int64_t>(myWorkgroups_) ? plan_.knobs.specWidth : 1; }

  bool admit() {  // next instance of the pool, false when it is empty
    InstanceSource::Item it;
    if (!source_.next(it)) {
      exhausted_ = true;
      return false;
    }
    live_.emplace_back();  // (a deque: the references to the other instances stay valid)
    gidx_.push_back(it.g);
    live_.back().inst.reset(new Instance(*it.inst, it.mapId, plan_.opt));
    live_.back().inst->setLinkSets(deviceCons_);
    if (tm_.on) live_.back().tAdmit = tm_.sinceStart();
    return true;
  }
  // The bookkeeping of an instance that is finished, with what it consumed.  It is FREED here, inside the loop, where the
  // host has slack and the device is busy: the paths, constraint sets and heaps of 16 384 instances are ~1e6 heap blocks
  // per worker, and freeing them after the loop was 70-130 ms of a 930 ms step with the GPU idle (measured,
  // MRP_HL_TIMING).  Searches of the instance that are still in flight (look-ahead) find `inst` empty when they return
  // and are dropped.
  void finishLive(Live& L, int64_t hl, int64_t ll, int64_t spec, int32_t searches) {
    L.counted = true;
    nActive_ -= 1;
    L.req.clear();  // requests of a finished instance point into freed CT nodes
    L.reqHead = 0;
    if (tm_.on) L.tDone = tm_.sinceStart();
    L.hl = hl;
    L.ll = ll;
    L.spec = spec;
    L.searches = searches;
    out_.expansions += ll;
    out_.specSearches += spec;
    L.inst.reset();
  }
  void retire(size_t k) {
    Live& L = live_[k];
    if (L.counted || !L.inst->done()) return;
    writeSolution(*L.inst, plan_.view->sol(gidx_[k]));
    out_.deviceScans += L.inst->deviceScans();
    out_.incrementalScans += L.inst->incrementalScans();
    finishLive(L, L.inst->hlExpanded(), L.inst->llExpanded(), L.inst->specSearches(), L.inst->llSearches());
  }

  // publish waiting searches, deepest instance first, while the device queue has room; false on error
  bool drainBacklog() {
    while (!backlog_.empty() && jobsOut_ < ringTarget_) {
      const size_t k = backlog_.top().second;
      backlog_.pop();
      live_[k].queued = false;
      const size_t before = ticketsOut_;
      if (!submitAll(k)) return false;
      if (ticketsOut_ != before) progress_ = true;
      if (live_[k].queued) break;  // the ring itself is full
    }
    return true;
  }
  // nothing older is waiting: start fresh instances; false on error
  bool admitFresh() {
    while (!exhausted_ && backlog_.empty() && jobsOut_ < ringTarget_ && nActive_ < activeLimit_ && admit()) {
      const size_t k = live_.size() - 1;
      Live& L = live_[k];
      nActive_ += 1;
      L.inst->setSpecWidth(specNow());
      L.inst->start(L.req);
      retire(k);
      progress_ = true;
      if (!submitAll(k)) return false;
    }
    return true;
  }

  // A root chain is back: its answers are delivered one by one, exactly like ten separate jobs.  false on error.
  bool harvestChain(int32_t pi) {
    Pending& P = pend_[pi];
    const size_t k = P.live;
    Live& L = live_[k];
    if (P.res[0].status == MRP_LL_BAD_JOB) {
      // chains are unavailable on this engine (mrp_ll.h MRP_LL_JOB_ROOT_CHAIN: needs the compact tier and room for the
      // focal table): nothing ran; the request goes out again as an ordinary job, and so does every later root search
      // of this worker
      rootChains_ = false;
      giveSlots(P);
      if (L.inst) {
        L.req = P.chainReq;
        L.reqHead = 0;
      }
      releasePending(pi);
      return followUp(k);
    }
    if (P.res[0].status != MRP_LL_OK) return fail("root chain failed on the engine (status " + std::to_string(P.res[0].status) + ")");
    const size_t cnt = P.chainRes.size();
    // The chain planned every agent and its workgroup found no conflict among the paths: the root node is the
    // solution.  Seven ten-agent instances in ten end here, without a path object, a conflict-tree node or a scan.
    if (plan_.knobs.rootFast && P.chainFirst == 0 && L.inst && !L.counted && static_cast<size_t>(P.res[0].n_states) == cnt &&
        P.res[0].cost == 0 && static_cast<int32_t>(cnt) == L.inst->nAgents() && L.inst->llSearches() == 0 &&
        (plan_.opt.max_hl_expansions < 0 || plan_.opt.max_hl_expansions >= 1)) {
      const int64_t ll = writeRootSolution(P.chainRes, plan_.view->sol(gidx_[k]));
      ranExpansions_ += ll;
      out_.searches += static_cast<int64_t>(cnt);
      out_.rootSolved += 1;
      finishLive(L, 1, ll, 0, static_cast<int32_t>(cnt));
      giveSlots(P);
      releasePending(pi);
      return true;
    }
    size_t q = 0;
    for (; q < cnt; ++q) {
      const mrp_ll_result& r = P.chainRes[q];
      if (plan_.knobs.chainDebug)
        std::fprintf(stderr, "[chain] inst %d agent %d: status %d cost %d fmin %d n %d expanded %lld\n", gidx_[k],
                     P.chainFirst + static_cast<int>(q), r.status, r.cost, r.fmin, r.n_states, (long long)r.expanded);
      if (r.status == MRP_LL_NOT_RUN || !L.inst) break;
      ranExpansions_ += r.expanded;
      out_.searches += 1;
      ans_.clear();
      ans_.push_back(answerOf(r, P.outSlot[q], &slotPool_));
      L.req.clear();  // (the request for the next root agent, which the chain has already answered — or not, below)
      L.reqHead = 0;
      L.inst->setSpecWidth(specNow());
      L.inst->deliver(P.group, ans_, L.req);
      ans_.clear();
      retire(k);
    }
    if (L.inst && q < cnt && static_cast<int32_t>(q) < P.chainCount && P.chainRes[q].status == MRP_LL_NOT_RUN) {
      // the search of this agent did not fit the compact tier: it goes as an ordinary job (any tier), chains resume behind it
      L.noChainAgent = P.chainFirst + static_cast<int32_t>(q);
      if (q == 0) {  // nothing was delivered, so nothing re-created the request
        L.req = P.chainReq;
        L.reqHead = 0;
      }
    }
    giveSlots(P, q);  // agents the chain did not reach
    releasePending(pi);
    return followUp(k);
  }
  // An ordinary ticket is back: its answers go to the instance's machine.  false on error.
  bool harvestJobs(int32_t pi) {
    Pending& P = pend_[pi];
    const size_t k = P.live;
    Live& L = live_[k];
    const TimePoint tu0 = tm_.clock();
    ans_.clear();
    for (size_t q = 0; q < P.res.size(); ++q) {
      ranExpansions_ += P.res[q].expanded;
      ans_.push_back(answerOf(P.res[q], P.outSlot[q], &slotPool_));
      if (!P.conf.empty() && P.res[q].status == MRP_LL_OK) {
        ans_.back().scan = P.conf[q];
        ans_.back().scanFromParent = P.fromParent(q);
      }
    }
    const int32_t group = P.group;
    releasePending(pi);
    const TimePoint tu1 = tm_.clock();
    if (L.inst) {  // (else: a pre-computed expansion that came back after its instance had finished)
      L.inst->setSpecWidth(specNow());
      L.inst->deliver(group, ans_, L.req);
      retire(k);
    }
    ans_.clear();   // the paths nobody took go back to the slot pool now
    const TimePoint tu2 = tm_.clock();
    tm_.unpack += secondsBetween(tu0, tu1);
    tm_.advance += secondsBetween(tu1, tu2);
    return followUp(k);
  }

  bool loop() {
    std::vector<int32_t> doneTickets(64);  // small harvest chunks keep the latency of any one instance's chain low
    std::vector<int32_t> donePend;
    ProgressWatchdog watchdog;
    while (ticketsOut_ != 0 || !backlog_.empty() || !exhausted_) {
      progress_ = false;
      const TimePoint tA = clockNow();
      if (!drainBacklog() || !admitFresh()) return false;
      const TimePoint tB = clockNow();
      tm_.submit += secondsBetween(tA, tB);
      // harvest: one pass over the ring's completion words, whatever the number of instances in flight
      int32_t nDone = 0;
      const int32_t room = static_cast<int32_t>(doneTickets.size());
      if ((tagged_ ? mrp_ll_poll_any_tagged(seat_.ctx, seat_.coIndex, doneTickets.data(), room, &nDone)
                   : mrp_ll_poll_any(seat_.ctx, doneTickets.data(), room, &nDone)) != MRP_LL_SUCCESS) {
        return failLL("mrp_ll_poll_any");
      }
      const TimePoint tC = clockNow();
      (nDone ? tm_.pollHit : tm_.pollEmpty) += secondsBetween(tB, tC);
      (nDone ? tm_.nPollHit : tm_.nPollEmpty) += 1;
      // resolve the owners first: a ticket id freed by this harvest can be handed out again by a resubmission below
      donePend.resize(nDone);
      for (int32_t d = 0; d < nDone; ++d) donePend[d] = ticketPend_[doneTickets[d]];
      for (int32_t pi : donePend) {
        progress_ = true;
        ticketsOut_ -= 1;
        jobsOut_ -= static_cast<int64_t>(pend_[pi].res.size());
        if (!(pend_[pi].chainFirst >= 0 ? harvestChain(pi) : harvestJobs(pi))) return false;
      }
      const TimePoint tD = clockNow();
      out_.buildS += secondsBetween(tA, tB);
      out_.llS += secondsBetween(tB, tC);
      out_.consumeS += secondsBetween(tC, tD);
      if (!watchdog.turn(progress_)) return fail("session: no progress for too long");
    }
    return true;
  }

  // Co-workers first: every one of them, failed or not, says that it has left its loop; then the leader closes the session.
  void end() {
    if (tagged_) {
      seat_.co->finished.fetch_add(1, std::memory_order_acq_rel);
      if (seat_.coIndex == 0)
        while (seat_.co->finished.load(std::memory_order_acquire) < seat_.coCount) std::this_thread::yield();
    }
    if (leader() && mrp_ll_session_end(seat_.ctx) != MRP_LL_SUCCESS && out_.err.empty()) failLL("mrp_ll_session_end");
  }

  // The worker's timing lines and, unless its loop failed, its totals.
  void finish(bool loopOk) {
    if (tm_.on && leader()) tm_.report(seat_.ctx, live_, gidx_, out_);
    if (!loopOk) return;
    for (size_t k = 0; k < live_.size(); ++k)
      if (live_[k].inst) {  // (none: the loop ends when every instance has been retired)
        writeSolution(*live_[k].inst, plan_.view->sol(gidx_[k]));
        out_.expansions += live_[k].inst->llExpanded();
        out_.specSearches += live_[k].inst->specSearches();
        out_.deviceScans += live_[k].inst->deviceScans();
        out_.incrementalScans += live_[k].inst->incrementalScans();
      }
    out_.specWasted += ranExpansions_ - out_.expansions;
    if (tm_.on) {
      const TimePoint written = clockNow();
      live_.clear();
      tm_.reportFreed(plan_.epoch, written, clockNow());
    }
  }

  const SessionPlan& plan_;
  const WorkerSeat seat_;
  GroupResult& out_;
  const bool tagged_;  // this engine has two workers: tagged calls only
  // not const: an engine that cannot run chains — no compact tier, a window too small for the chain's focal table —
  // rejects the first one, and this worker goes on with one job per root search
  bool rootChains_;
  // children go out through mrp_ll_submit_node and say what their parent's scan established (SolveKnobs::deviceScanIncremental,
  // and the engine has the call)
  bool scanFromParent_;
  bool deviceScan_;  // children go out through mrp_ll_submit_scan (SolveKnobs::deviceScan, and the engine has the call) — or as above
  const bool deviceCons_;  // children name their constraint sets by slot (the call reserved a constraint store: SolveKnobs::deviceCons)
  const int32_t myWorkgroups_;
  // f2: slots of the engine's device-resident path store, handed to the searches of this worker for their result paths.
  // Declared before every member that can hold a Path (live_, pend_ via its tickets' instances, ans_): members are
  // destroyed in reverse order, so the pool outlives every Path that returns its slot to it.
  SlotPool slotPool_;
  SlotPool consPool_;  // slots of the engine's constraint store, likewise (it outlives every ConstraintSet)
  std::vector<const ConstraintSet*> slotted_;  // submitJobs: the sets that were given a slot for the ticket being published
  InstanceSource source_;
  std::deque<Live> live_;        // grows as instances are admitted; references stay valid
  std::vector<int32_t> gidx_;    // live entry -> global instance index
  std::deque<Pending> pend_;
  std::vector<int32_t> pendFree_;
  std::vector<int32_t> ticketPend_;  // session ticket id -> pend entry
  std::vector<LLAnswer> ans_;
  JobBatch batch_;
  std::vector<int32_t> chainIds_, chainXy_;
  typedef std::pair<int64_t, size_t> Waiting;  // (priority, live index)
  std::priority_queue<Waiting> backlog_;
  int64_t ringTarget_ = 0;
  size_t activeLimit_ = 0, nActive_ = 0, ticketsOut_ = 0;
  int64_t jobsOut_ = 0, ranExpansions_ = 0;
  bool exhausted_ = false, progress_ = false;
  Timing tm_;
};

}  // namespace mrp_hl
