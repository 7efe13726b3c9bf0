// The prioritized-SIPP drivers (mrp_hl.h mrp_hl_solver_prioritized_sipp): the loop of mapf_prioritized_sipp.cpp:214-270 for
// many instances at once.  Agents of one instance are a chain — each plans against the intervals the earlier ones occupy —
// instances are independent.  Two schedules: in session mode (default) the SIPP kernel stays resident and an instance
// publishes its next agent's search the moment the previous one is back; the round-based one (MRP_HL_SIPP_BATCH) plans
// agent r of every instance in round r.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ct_session.hpp"

namespace mrp_hl {

// The environment knobs of a prioritized-SIPP call, read once per call.
struct SippKnobs {
  bool batch = false;          // MRP_HL_SIPP_BATCH (set): the round-based schedule, for comparison
  int32_t wgs = 0;             // MRP_HL_SIPP_WGS: resident wavefronts per engine, at least 1 (0 unset: what the device holds)
  // MRP_HL_SIPP_MAX_EXPANSIONS (test knob): the expansion cap of every search; the reference has none (-1), and a capped
  // search ends its instance with that status.
  int64_t maxExpansions = -1;
  bool timing = false;         // MRP_HL_SIPP_TIMING (set): where every session worker's time went, on stderr
  static SippKnobs read() {
    SippKnobs k;
    k.batch = std::getenv("MRP_HL_SIPP_BATCH") != nullptr;
    if (const char* e = std::getenv("MRP_HL_SIPP_WGS")) k.wgs = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("MRP_HL_SIPP_MAX_EXPANSIONS")) k.maxExpansions = std::atoll(e) > 0 ? std::atoll(e) : -1;
    k.timing = std::getenv("MRP_HL_SIPP_TIMING") != nullptr;
    return k;
  }
};

struct SippInterval { int32_t s, e; };  // a collision interval [s, e] on a cell

// The search of agent `a` of instance `in` (map `mapId` on its engine); the caller adds the collision intervals, as
// arrays or as a table.
inline mrp_ll_job sippJob(const mrp_hl_instance& in, int32_t mapId, int32_t a, const SippKnobs& knobs) {
  mrp_ll_job j;
  std::memset(&j, 0, sizeof(j));
  j.map_id = mapId;
  j.algo = MRP_LL_SIPP;
  j.w = 1.0f;
  j.start_x = in.starts_xy[2 * a];
  j.start_y = in.starts_xy[2 * a + 1];
  j.goal_x = in.goals_xy[2 * a];
  j.goal_y = in.goals_xy[2 * a + 1];
  j.max_expansions = knobs.maxExpansions;
  return j;
}

// Uploads the map of a prioritized-SIPP instance and clears its solution; false (out.err set) if the engine refuses.
inline bool beginSippInstance(mrp_ll_ctx* ctx, const mrp_hl_instance& in, mrp_hl_sipp_solution& so, int32_t& mapId, GroupResult& out) {
  if (mrp_ll_upload_map(ctx, in.dimx, in.dimy, in.n_obstacles, in.obstacles_xy, &mapId) != MRP_LL_SUCCESS) {
    out.err = llError("mrp_ll_upload_map", ctx);
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
inline bool recordSippAnswer(const mrp_ll_result& r, int32_t a, mrp_hl_sipp_solution& so, GroupResult& out) {
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

// The round-based schedule for instances idx[...] on one engine: round r plans agent r of every instance that still has one.
inline void runSippGroup(mrp_ll_ctx* ctx, const SippKnobs& knobs, int32_t horizon, int32_t nTickets, const mrp_hl_instance* instances,
                         mrp_hl_sipp_solution* sols, const std::vector<int32_t>& idx, GroupResult& out) {
  typedef SippInterval Iv;
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
      mrp_ll_job j = sippJob(in, p.mapId, p.agent, knobs);
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
      out.err = llError("mrp_ll_submit", ctx);
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
      out.err = llError("mrp_ll_wait", ctx);
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
inline void runSippGroupSession(mrp_ll_ctx* ctx, const SippKnobs& knobs, int32_t horizon, int32_t slots, int32_t nWorkers,
                                const mrp_hl_instance* instances, mrp_hl_sipp_solution* sols, const std::vector<int32_t>& idx,
                                GroupResult& out) {
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
  if (knobs.wgs > 0) wgs = knobs.wgs;
  if (mrp_ll_session_begin_sipp(ctx, wgs) != MRP_LL_SUCCESS) {
    out.err = llError("mrp_ll_session_begin_sipp", ctx);
    return;
  }
  // 1 published, 0 no free job slot (retry later), -1 error
  auto submit = [&](size_t q) -> int {
    Prio& p = st[q];
    mrp_ll_job j = sippJob(instances[idx[q]], p.mapId, p.agent, knobs);
    j.sipp_table = p.tab;  // sipp.setCollisionIntervals(location, intervals) for every location (:224-226), kept up to date
    j.sipp_commit = 1;     // ... by the engine: the stays of the path it finds become collision intervals (:237-246)
    bindResults(&p.res, 1, p.states, cap);
    int rc = mrp_ll_submit(ctx, 1, &j, &p.res, &p.ticket);
    if (rc == MRP_LL_E_BUSY) return 0;
    if (rc != MRP_LL_SUCCESS) {
      out.err = llError("mrp_ll_submit", ctx);
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
  const bool timing = knobs.timing;  // where a worker thread's time goes
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
      out.err = llError("mrp_ll_poll_any", ctx);
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
  if (mrp_ll_session_end(ctx) != MRP_LL_SUCCESS && out.err.empty()) out.err = llError("mrp_ll_session_end", ctx);
  if (timing)
    std::fprintf(stderr, "[mrp_hl] sipp worker: %.1f ms total; submit %.1f ms, poll_any %.1f ms (%llu calls, %llu empty), consume %.1f ms\n",
                 secondsBetween(t0, clockNow()) * 1e3, tSubmit * 1e3, tPoll * 1e3, (unsigned long long)nPolls,
                 (unsigned long long)nEmptyPolls, tConsume * 1e3);
  out.rounds = maxAgents;  // longest chain of dependent searches
}

// mrp_hl_solver_prioritized_sipp on the solver's engines.  Returns MRP_LL_SUCCESS, or MRP_LL_E_DEVICE with `err` set.
inline int prioritizedSipp(const std::vector<mrp_ll_ctx*>& engines, const mrp_ll_options& llOpt, int32_t nInst,
                           const mrp_hl_instance* instances, mrp_hl_sipp_solution* sols, mrp_hl_batch_stats* stats, std::string& err) {
  const SippKnobs knobs = SippKnobs::read();
  const int32_t horizon = llOpt.max_horizon > 0 ? llOpt.max_horizon : 512;
  // instances are independent: one share per worker thread / engine, as for CBS and ECBS
  const int32_t nThreads = std::max(1, std::min<int32_t>(static_cast<int32_t>(engines.size()), std::max(nInst, 1)));
  std::vector<std::vector<int32_t>> idx(nThreads);
  for (int32_t k = 0; k < nInst; ++k) idx[k % nThreads].push_back(k);
  std::vector<GroupResult> gr(nThreads);
  auto t0 = std::chrono::steady_clock::now();
  {
    std::vector<std::thread> th;
    for (int32_t t = 0; t < nThreads; ++t)
      th.emplace_back([&, t]() {
        if (knobs.batch)
          runSippGroup(engines[t], knobs, horizon, llOpt.n_tickets, instances, sols, idx[t], gr[t]);
        else
          runSippGroupSession(engines[t], knobs, horizon, llOpt.slots, nThreads, instances, sols, idx[t], gr[t]);
      });
    for (auto& x : th) x.join();
  }
  mrp_hl_batch_stats bs;
  std::memset(&bs, 0, sizeof(bs));
  bs.wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (auto& g : gr) {
    if (!g.err.empty()) {
      err = g.err;
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

}  // namespace mrp_hl
