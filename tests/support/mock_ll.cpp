// TEST INFRASTRUCTURE ONLY — never shipped, never built into libmultirobotplanning_amd/lib.
// Implements the C-ABI of include/mrp_ll.h on top of the ORACLE's low-level searches (oracle_ll_search; oracle_sipp_single_at
// for MRP_LL_SIPP jobs) so that the host-side drivers (csrc/hl/) can be exercised on a machine without a GPU (`-m "not gpu"`
// tests).
// The product library has no such path: libmrp_ll.so fails with MRP_LL_E_DEVICE when no HIP device exists.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <string>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/mrp_ll.h"

extern "C" void oracle_conflict_scan(int nAgents, const int32_t* pathLen, const int32_t* pathXY, int32_t* out);
extern "C" int oracle_sipp_single_at(int dimx, int dimy, int nObst, const int32_t* obstXY, int sx, int sy, int gx, int gy, int nCI,
                                     const int32_t* ci, int startTime, int32_t* statesXYT, int cap, int64_t* expanded,
                                     int32_t* costFmin);
extern "C" int oracle_ll_search(int algo, float w, int dimx, int dimy, int nObst, const int32_t* obstXY, int agentIdx,
                                int startX, int startY, int goalX, int goalY, int nVC, const int32_t* vc, int nEC,
                                const int32_t* ec, int nCtx, const int32_t* ctxLen, const int32_t* ctxXY,
                                int64_t capExpansions, int32_t* out, int64_t* expanded, int32_t* statesTXY,
                                int32_t* actions, int cap);

struct MockMap {
  int dimx, dimy;
  std::vector<int32_t> obst;
};
struct mrp_ll_ctx {
  std::vector<MockMap> maps;
  mrp_ll_stats stats;
  std::string err;
  int32_t pendingJobs = 0;
  std::vector<int32_t> doneTickets;  // completed (synchronously in mrp_ll_submit), not yet reported by poll_any
  int32_t nextTicket = 0;
  const mrp_ll_job* jobs = nullptr;
  mrp_ll_result* results = nullptr;
  std::vector<std::vector<int32_t>> store;  // MRP_MOCK_PATH_STORE=1: the "device" path store, slot -> x, y, x, y, ...
  int32_t index = 0;      // how many contexts this process had created before this one (MRP_MOCK_CALL_LOG)
  uint32_t tagsSeen = 0;  // bit t: a worker with tag t has made a tagged call since the last mrp_ll_session_end
};

// MRP_MOCK_CALL_LOG=<file>: the calls that size and start a solve — tiers, occupancy, geometry, session begin / end, store
// reserves — append one line each, "<context index> <call> <integer arguments>", so that a test can pin what a driver asks
// of every engine (tests/test_launch_plan_cpu.py).  Engines race each other in the file; the lines of one engine are in
// call order.
namespace {
std::mutex g_logMu;
int32_t g_created = 0;  // (under g_logMu)
void callLog(const mrp_ll_ctx* c, const char* fmt, ...) {
  const char* file = std::getenv("MRP_MOCK_CALL_LOG");
  if (!file) return;
  std::lock_guard<std::mutex> lock(g_logMu);
  if (FILE* f = std::fopen(file, "a")) {
    std::fprintf(f, "%d ", c->index);
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(f, fmt, ap);
    va_end(ap);
    std::fputc('\n', f);
    std::fclose(f);
  }
}
// MRP_MOCK_GEOMETRY="occ,frontOcc,frontLds,heavyLds": what mrp_ll_configure_tiers / mrp_ll_session_occupancy (occ) and
// mrp_ll_session_tiers_geometry (the other three) report.  Unset: 4, 12, 12928, 31360.
struct MockGeometry {
  int occ = 4, frontOcc = 12, frontLds = 12928, heavyLds = 31360;
};
MockGeometry mockGeometry() {
  MockGeometry g;
  if (const char* e = std::getenv("MRP_MOCK_GEOMETRY")) {
    MockGeometry h;
    if (std::sscanf(e, "%d,%d,%d,%d", &h.occ, &h.frontOcc, &h.frontLds, &h.heavyLds) == 4) g = h;
  }
  return g;
}
}  // namespace

extern "C" {
const char* mrp_ll_version(void) { return "mrp_ll MOCK (oracle-backed, tests only)"; }
const char* mrp_ll_last_error(const mrp_ll_ctx* c) { return c ? c->err.c_str() : "null"; }
int mrp_ll_create(const mrp_ll_options*, mrp_ll_ctx** out) {
  *out = new mrp_ll_ctx();
  std::memset(&(*out)->stats, 0, sizeof(mrp_ll_stats));
  {
    std::lock_guard<std::mutex> lock(g_logMu);
    (*out)->index = g_created++;
  }
  callLog(*out, "create");
  return MRP_LL_SUCCESS;
}
void mrp_ll_destroy(mrp_ll_ctx* c) { delete c; }
int mrp_ll_upload_map(mrp_ll_ctx* c, int32_t dimx, int32_t dimy, int32_t n, const int32_t* xy, int32_t* id) {
  MockMap m{dimx, dimy, std::vector<int32_t>(xy, xy + 2 * n)};
  c->maps.push_back(m);
  *id = static_cast<int32_t>(c->maps.size()) - 1;
  return MRP_LL_SUCCESS;
}
// MRP_LL_JOB_ROOT_CHAIN on the mock: agent after agent through the oracle, contexts from the mock's path store.
// MRP_MOCK_CHAIN_BREAK=K: a search of more than K expansions "does not fit the LDS tier" and ends the chain in front of it.
static void mockChain(mrp_ll_ctx* c, const mrp_ll_job& j, mrp_ll_result& r) {
  const MockMap& m = c->maps[j.map_id];
  const int n = j.n_agents, first = j.agent_idx;
  const int end = j.chain_count > 0 ? std::min(n, first + j.chain_count) : n;
  const char* bk = std::getenv("MRP_MOCK_CHAIN_BREAK");
  const int64_t breakAt = bk ? std::atoll(bk) : -1;
  int64_t budget = j.max_expansions, total = 0;
  int done = 0;
  bool stopped = false;
  r.status = MRP_LL_OK;
  for (int a = first; a < n; ++a) {
    mrp_ll_result& ri = r.chain_results[a - first];
    ri.status = MRP_LL_NOT_RUN;
    ri.cost = ri.fmin = ri.n_states = 0;
    ri.expanded = 0;
    if (stopped || a >= end) continue;
    std::vector<int32_t> ctxLen, ctxXY;
    for (int b = 0; b < n; ++b) {
      const std::vector<int32_t>* p = b < a ? &c->store[j.path_ids[b]] : nullptr;
      ctxLen.push_back(p ? static_cast<int32_t>(p->size() / 2) : 0);
      if (p) ctxXY.insert(ctxXY.end(), p->begin(), p->end());
    }
    const int32_t* q = j.chain_starts_goals_xy + 4 * a;
    int32_t out[4];
    int64_t expanded = 0;
    std::vector<int32_t> st(3 * 2048), ac(2048);
    int rc = oracle_ll_search(MRP_LL_ASTAR_EPS, j.w, m.dimx, m.dimy, static_cast<int>(m.obst.size() / 2), m.obst.data(), a, q[0],
                              q[1], q[2], q[3], 0, nullptr, 0, nullptr, n, ctxLen.data(), ctxXY.data(), budget, out, &expanded,
                              st.data(), ac.data(), 2048);
    if (breakAt >= 0 && expanded > breakAt) {  // (the device would have found out on the way; the answer is not used)
      stopped = true;
      continue;
    }
    ri.expanded = expanded;
    ri.tier = 0;
    total += expanded;
    done += 1;
    c->stats.jobs += 1;
    c->stats.expansions += expanded;
    if (rc == -1) {
      ri.status = MRP_LL_CAP_EXPANSIONS;
      stopped = true;
      continue;
    }
    ri.status = out[0] ? MRP_LL_OK : MRP_LL_NO_SOLUTION;
    ri.cost = out[1];
    ri.fmin = out[2];
    ri.n_states = out[0] ? out[3] : 0;
    if (!out[0]) {
      stopped = true;
      continue;
    }
    std::vector<int32_t>& slot = c->store[j.path_ids[a]];
    slot.clear();
    for (int k = 0; k < ri.n_states; ++k) {
      if (ri.states_txy && k < ri.states_cap) std::memcpy(ri.states_txy + 3 * k, st.data() + 3 * k, 12);
      slot.push_back(st[3 * k + 1]);
      slot.push_back(st[3 * k + 2]);
    }
    if (budget >= 0) budget = budget > expanded ? budget - expanded : 0;
  }
  r.n_states = done;
  r.expanded = total;
  // the root node's conflicts (mrp_ll.h): the oracle's getFirstConflict + focalHeuristic over the chain's paths
  r.cost = r.fmin = -1;
  if (first == 0 && end == n && done == n && !stopped) {
    std::vector<int32_t> len, xy;
    for (int a = 0; a < n; ++a) {
      const std::vector<int32_t>& p = c->store[j.path_ids[a]];
      len.push_back(static_cast<int32_t>(p.size() / 2));
      xy.insert(xy.end(), p.begin(), p.end());
    }
    int32_t o[10];
    oracle_conflict_scan(n, len.data(), xy.data(), o);
    r.cost = o[9];
    r.fmin = o[0] ? (o[1] << 24) | (o[4] << 16) | (o[2] << 8) | o[3] : -1;
  }
}

}  // extern "C"

// An incrementally maintained SIPP table (mrp_ll.h mrp_ll_sipp_table_*): per cell the collision intervals added so far, and
// the cells that have some in first-touch order (the order does not matter to SIPP::setCollisionIntervals).
struct mrp_ll_sipp_table {
  std::map<std::pair<int32_t, int32_t>, std::vector<std::pair<int32_t, int32_t>>> perCell;
  std::vector<std::pair<int32_t, int32_t>> touched;
  void add(int32_t x, int32_t y, int32_t s, int32_t e) {
    std::vector<std::pair<int32_t, int32_t>>& v = perCell[{x, y}];
    if (v.empty()) touched.push_back({x, y});
    v.push_back({s, e});
  }
};

// An MRP_LL_SIPP job through the oracle's single-agent SIPP search, in either form: the collision_* arrays (a location given
// twice keeps the later list) or a sipp_table, to which a committed search adds the stays of the path it found.  The oracle
// has no expansion cap: a search that needed more than max_expansions > 0 expansions comes back as MRP_LL_CAP_EXPANSIONS.
static void mockSipp(mrp_ll_ctx* c, const mrp_ll_job& j, mrp_ll_result& r) {
  const MockMap& m = c->maps[j.map_id];
  mrp_ll_sipp_table arrays;
  if (!j.sipp_table) {
    const int32_t* iv = j.collision_intervals;
    for (int32_t l = 0; l < j.n_collision_locations; ++l) {
      const std::pair<int32_t, int32_t> cell{j.collision_xy[2 * l], j.collision_xy[2 * l + 1]};
      if (arrays.perCell.count(cell)) arrays.perCell[cell].clear();
      for (int32_t k = 0; k < j.collision_count[l]; ++k, iv += 2) arrays.add(cell.first, cell.second, iv[0], iv[1]);
    }
  }
  mrp_ll_sipp_table* table = j.sipp_table ? const_cast<mrp_ll_sipp_table*>(j.sipp_table) : &arrays;
  std::vector<int32_t> ci;
  for (const auto& cell : table->touched)
    for (const auto& iv : table->perCell[cell]) ci.insert(ci.end(), {cell.first, cell.second, iv.first, iv.second});
  const int cap = 4096;
  std::vector<int32_t> xyt(3 * cap);
  int64_t expanded = 0;
  int32_t costFmin[2] = {0, 0};
  const int n = oracle_sipp_single_at(m.dimx, m.dimy, static_cast<int>(m.obst.size() / 2), m.obst.data(), j.start_x, j.start_y,
                                      j.goal_x, j.goal_y, static_cast<int>(ci.size() / 4), ci.data(), j.initial_cost, xyt.data(),
                                      cap, &expanded, costFmin);
  r.tier = 0;
  c->stats.jobs += 1;
  if (j.max_expansions > 0 && expanded > j.max_expansions) {
    r.status = MRP_LL_CAP_EXPANSIONS;
    r.expanded = j.max_expansions;
    c->stats.expansions += r.expanded;
    return;
  }
  r.expanded = expanded;
  c->stats.expansions += expanded;
  r.status = n > 0 ? MRP_LL_OK : MRP_LL_NO_SOLUTION;
  r.cost = costFmin[0];
  r.fmin = costFmin[1];
  r.n_states = std::min(n, cap);
  if (n == 0) return;
  if (r.n_states > r.states_cap) r.status = MRP_LL_PATH_TRUNCATED;
  for (int k = 0; k < r.n_states && k < r.states_cap && r.states_txy; ++k) {
    r.states_txy[3 * k] = xyt[3 * k + 2];
    r.states_txy[3 * k + 1] = xyt[3 * k];
    r.states_txy[3 * k + 2] = xyt[3 * k + 1];
  }
  if (j.sipp_table && j.sipp_commit && r.status == MRP_LL_OK) {  // one interval per maximal stay, the last one open-ended
    int first = 0;
    for (int k = 1; k <= n; ++k)
      if (k == n || xyt[3 * k] != xyt[3 * first] || xyt[3 * k + 1] != xyt[3 * first + 1]) {
        table->add(xyt[3 * first], xyt[3 * first + 1], xyt[3 * first + 2], k == n ? INT32_MAX : xyt[3 * k + 2] - 1);
        first = k;
      }
  }
}

extern "C" {
int mrp_ll_search_batch(mrp_ll_ctx* c, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res) {
  for (int i = 0; i < n; ++i) {
    const mrp_ll_job& j = jobs[i];
    mrp_ll_result& r = res[i];
    if (j.algo == MRP_LL_SIPP && j.map_id >= 0 && j.map_id < static_cast<int>(c->maps.size())) {
      mockSipp(c, j, r);
      continue;
    }
    // MRP_MOCK_CHAIN_REJECT=1: an engine that cannot run root chains (mrp_ll.h MRP_LL_JOB_ROOT_CHAIN): nothing is run
    if ((j.flags & MRP_LL_JOB_ROOT_CHAIN) && std::getenv("MRP_MOCK_CHAIN_REJECT")) {
      r.status = MRP_LL_BAD_JOB;
      continue;
    }
    if ((j.flags & MRP_LL_JOB_ROOT_CHAIN) && j.map_id >= 0 && j.map_id < static_cast<int>(c->maps.size()) && !c->store.empty()) {
      mockChain(c, j, r);
      continue;
    }
    if (j.map_id < 0 || j.map_id >= static_cast<int>(c->maps.size())) {
      r.status = MRP_LL_BAD_JOB;
      continue;
    }
    const MockMap& m = c->maps[j.map_id];
    std::vector<int32_t> ctxLen, ctxXY;
    int nCtx = j.algo == MRP_LL_ASTAR_EPS ? j.n_agents : 0;
    for (int a = 0; a < nCtx; ++a) {
      int len = a == j.agent_idx ? 0 : j.path_len[a];
      ctxLen.push_back(len);
      for (int k = 0; k < 2 * len; ++k) ctxXY.push_back(j.path_xy[a][k]);
    }
    int32_t out[4];
    int64_t expanded = 0;
    std::vector<int32_t> st(3 * 2048), ac(2048);
    int rc = oracle_ll_search(j.algo, j.w, m.dimx, m.dimy, static_cast<int>(m.obst.size() / 2), m.obst.data(),
                              j.agent_idx, j.start_x, j.start_y, j.goal_x, j.goal_y, j.n_vertex_constraints,
                              j.vertex_constraints, j.n_edge_constraints, j.edge_constraints, nCtx, ctxLen.data(),
                              ctxXY.data(), j.max_expansions, out, &expanded, st.data(), ac.data(), 2048);
    r.expanded = expanded;
    r.tier = 0;
    if (rc == -1) {
      r.status = MRP_LL_CAP_EXPANSIONS;
      continue;
    }
    r.status = out[0] ? MRP_LL_OK : MRP_LL_NO_SOLUTION;
    r.cost = out[1];
    r.fmin = out[2];
    r.n_states = out[0] ? out[3] : 0;
    for (int k = 0; k < r.n_states && k < r.states_cap; ++k) {
      if (r.states_txy) std::memcpy(r.states_txy + 3 * k, st.data() + 3 * k, 12);
      if (r.actions && k + 1 < r.n_states) r.actions[k] = ac[k];
    }
    if ((j.flags & MRP_LL_JOB_STORE_RESULT) && j.result_path_id >= 0 && j.result_path_id < static_cast<int>(c->store.size())) {
      std::vector<int32_t>& slot = c->store[j.result_path_id];
      slot.clear();
      for (int k = 0; k < r.n_states; ++k) {
        slot.push_back(st[3 * k + 1]);
        slot.push_back(st[3 * k + 2]);
      }
    }
    c->stats.jobs += 1;
    c->stats.expansions += expanded;
  }
  c->stats.launches += 1;
  return MRP_LL_SUCCESS;
}
// MRP_MOCK_TRACE=<file>: every submission appends one line, a 64-bit FNV-1a over what the driver asked for — the jobs'
// values and the arrays they point to, never a pointer or a ticket id — so that a test can pin the ORDER in which a
// driver publishes its searches (results do not depend on it).
namespace {
std::mutex g_traceMu;
void traceSubmit(int32_t n, const mrp_ll_job* jobs) {
  const char* file = std::getenv("MRP_MOCK_TRACE");
  if (!file) return;
  uint64_t h = 14695981039346656037ull;
  auto mix = [&h](int64_t v) {
    for (int b = 0; b < 8; ++b) h = (h ^ ((static_cast<uint64_t>(v) >> (8 * b)) & 0xFFu)) * 1099511628211ull;
  };
  auto mixAll = [&mix](const int32_t* p, int64_t cnt) {
    for (int64_t k = 0; k < cnt; ++k) mix(p[k]);
  };
  mix(n);
  for (int32_t i = 0; i < n; ++i) {
    const mrp_ll_job& j = jobs[i];
    int32_t wBits;
    std::memcpy(&wBits, &j.w, 4);
    const int64_t head[] = {j.map_id, j.algo, wBits, j.agent_idx, j.start_x, j.start_y, j.goal_x, j.goal_y, j.n_agents,
                            j.flags, j.chain_count, j.result_path_id, j.max_expansions, j.n_vertex_constraints,
                            j.n_edge_constraints};
    for (int64_t v : head) mix(v);
    mixAll(j.vertex_constraints, 3 * static_cast<int64_t>(j.n_vertex_constraints));
    mixAll(j.edge_constraints, 5 * static_cast<int64_t>(j.n_edge_constraints));
    mix(j.path_len ? 1 : 0);
    if (j.path_len) mixAll(j.path_len, j.n_agents);
    mix(j.path_ids ? 1 : 0);
    if (j.path_ids) mixAll(j.path_ids, j.n_agents);
    mix(j.path_xy ? 1 : 0);
    mix(j.chain_starts_goals_xy ? 1 : 0);
    if (j.chain_starts_goals_xy) mixAll(j.chain_starts_goals_xy, 4 * static_cast<int64_t>(j.n_agents));
  }
  std::lock_guard<std::mutex> lock(g_traceMu);
  if (FILE* f = std::fopen(file, "a")) {
    std::fprintf(f, "%016llx\n", static_cast<unsigned long long>(h));
    std::fclose(f);
  }
}
// MRP_MOCK_BUSY=N: the job ring is "full" while N finished tickets wait to be polled (0: never)
bool mockBusy(size_t waiting) {
  const char* e = std::getenv("MRP_MOCK_BUSY");
  return e && std::atoi(e) > 0 && waiting >= static_cast<size_t>(std::atoi(e));
}
}  // namespace
int mrp_ll_submit(mrp_ll_ctx* c, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res, int32_t* ticket) {
  traceSubmit(n, jobs);
  if (mockBusy(c->doneTickets.size())) return MRP_LL_E_BUSY;
  *ticket = c->nextTicket++ & 0xFFFF;
  c->doneTickets.push_back(*ticket);
  return mrp_ll_search_batch(c, n, jobs, res);
}
int mrp_ll_submit_lane(mrp_ll_ctx* c, int32_t, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res, int32_t* ticket) {
  return mrp_ll_submit(c, n, jobs, res, ticket);
}
// co-workers: two host threads on one context (mrp_ll.h); finished tickets wait per tag
namespace {
std::mutex g_coMu;
std::map<mrp_ll_ctx*, std::vector<int32_t>> g_coDone[4];
}  // namespace
int mrp_ll_submit_tagged(mrp_ll_ctx* c, int32_t tag, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res, int32_t* ticket) {
  if (tag < 0 || tag > 3) return MRP_LL_E_INVALID;
  traceSubmit(n, jobs);
  std::lock_guard<std::mutex> lock(g_coMu);
  c->tagsSeen |= 1u << tag;
  if (mockBusy(g_coDone[tag][c].size())) return MRP_LL_E_BUSY;
  *ticket = c->nextTicket++ & 0xFFFF;
  g_coDone[tag][c].push_back(*ticket);
  return mrp_ll_search_batch(c, n, jobs, res);
}
int mrp_ll_poll_any_tagged(mrp_ll_ctx* c, int32_t tag, int32_t* tickets, int32_t cap, int32_t* n) {
  if (tag < 0 || tag > 3) return MRP_LL_E_INVALID;
  std::lock_guard<std::mutex> lock(g_coMu);
  // (a co-worker that finds the pool of instances empty never submits, but it always polls once: counting both calls keeps
  // the tag count of the call log independent of which worker thread started first)
  c->tagsSeen |= 1u << tag;
  std::vector<int32_t>& d = g_coDone[tag][c];
  int32_t k = 0;
  while (!d.empty() && k < cap && k < 3) {  // a few at a time, newest first: out of submission order
    tickets[k++] = d.back();
    d.pop_back();
  }
  *n = k;
  return MRP_LL_SUCCESS;
}
// MRP_MOCK_SHUFFLE=<seed>: completed tickets are reported a few at a time in a pseudo-random order, so that the drivers
// see the groups of one instance come back out of submission order (as they do on the GPU).
int mrp_ll_poll_any(mrp_ll_ctx* c, int32_t* tickets, int32_t cap, int32_t* n) {
  int32_t k = 0;
  const char* sh = std::getenv("MRP_MOCK_SHUFFLE");
  if (sh) {
    static thread_local uint64_t x = 0;
    if (x == 0) x = 0x9E3779B97F4A7C15ull ^ static_cast<uint64_t>(std::atoll(sh) + 1) ^ reinterpret_cast<uintptr_t>(c);
    auto rnd = [&]() {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      return x;
    };
    if (!c->doneTickets.empty() && (rnd() & 3) == 0) {  // sometimes report nothing: work stays in flight
      *n = 0;
      return MRP_LL_SUCCESS;
    }
    const int32_t lim = 1 + static_cast<int32_t>(rnd() % 3);
    while (!c->doneTickets.empty() && k < cap && k < lim) {
      const size_t i = rnd() % c->doneTickets.size();
      tickets[k++] = c->doneTickets[i];
      c->doneTickets[i] = c->doneTickets.back();
      c->doneTickets.pop_back();
    }
    *n = k;
    return MRP_LL_SUCCESS;
  }
  while (!c->doneTickets.empty() && k < cap) {
    tickets[k++] = c->doneTickets.back();
    c->doneTickets.pop_back();
  }
  *n = k;
  return MRP_LL_SUCCESS;
}
int mrp_ll_wait(mrp_ll_ctx* c, int32_t ticket) {  // (it ran inside mrp_ll_submit; a ticket waited for is not polled later)
  auto it = std::find(c->doneTickets.begin(), c->doneTickets.end(), ticket);
  if (it != c->doneTickets.end()) c->doneTickets.erase(it);
  return MRP_LL_SUCCESS;
}
int mrp_ll_sync_maps(mrp_ll_ctx*) { return MRP_LL_SUCCESS; }
int mrp_ll_release_maps(mrp_ll_ctx* c) {
  c->maps.clear();
  return MRP_LL_SUCCESS;
}
int mrp_ll_configure_tiers(mrp_ll_ctx* c, int32_t nodes, int32_t rows, int32_t pathBytes, int32_t* occ) {
  callLog(c, "configure_tiers %d %d %d", nodes, rows, pathBytes);
  if (occ) *occ = mockGeometry().occ;
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_occupancy(mrp_ll_ctx* c, int32_t algo, int32_t* occ) {
  callLog(c, "session_occupancy %d", algo);
  if (occ) *occ = mockGeometry().occ;
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_begin(mrp_ll_ctx* c, int32_t wgs) {
  callLog(c, "session_begin %d", wgs);
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_begin_sipp(mrp_ll_ctx* c, int32_t wgs) {
  callLog(c, "session_begin_sipp %d", wgs);
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_begin_algo(mrp_ll_ctx* c, int32_t algo, int32_t wgs) {
  callLog(c, "session_begin_algo %d %d", algo, wgs);
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_begin_tiers(mrp_ll_ctx* c, int32_t algo, int32_t wgs, int32_t heavy) {
  callLog(c, "session_begin_tiers %d %d %d", algo, wgs, heavy);
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_begin_tiers_gated(mrp_ll_ctx* c, int32_t algo, int32_t wgs, int32_t heavy, int32_t* gate, int32_t nGate) {
  callLog(c, "session_begin_tiers_gated %d %d %d %d", algo, wgs, heavy, nGate);
  if (gate) __atomic_fetch_add(gate, 1, __ATOMIC_ACQ_REL);
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_tiers_geometry(mrp_ll_ctx* c, int32_t* occ, int32_t* front, int32_t* heavy) {
  callLog(c, "session_tiers_geometry");
  const MockGeometry g = mockGeometry();
  if (occ) *occ = g.frontOcc;
  if (front) *front = g.frontLds;
  if (heavy) *heavy = g.heavyLds;
  return MRP_LL_SUCCESS;
}
int mrp_ll_session_end(mrp_ll_ctx* c) {
  int tags = 0;
  {
    std::lock_guard<std::mutex> lock(g_coMu);
    for (int t = 0; t < 4; ++t) tags += (c->tagsSeen >> t) & 1u;
    c->tagsSeen = 0;
  }
  callLog(c, "session_end tags=%d", tags);
  return MRP_LL_SUCCESS;
}
int mrp_ll_poll(mrp_ll_ctx*, int32_t, int32_t* done) {
  *done = 1;  // the mock runs every job synchronously inside mrp_ll_submit
  return MRP_LL_SUCCESS;
}
int mrp_ll_conflict_scan(mrp_ll_ctx*, int32_t, const int32_t*, const int32_t*, const int32_t*, mrp_ll_conflict*) {
  return MRP_LL_E_DEVICE;  // the scan kernel has no stand-in: the host drivers do not call it
}
// no store by default: the drivers fall back to tables.  MRP_MOCK_PATH_STORE=1: a host-side one, so that the drivers' path
// ids and root chains run on the CPU too
int mrp_ll_path_store_reserve(mrp_ll_ctx* c, int32_t n) {
  const char* e = std::getenv("MRP_MOCK_PATH_STORE");
  const bool have = e && *e == '1';
  callLog(c, "path_store_reserve %d -> %d", n, have ? MRP_LL_SUCCESS : MRP_LL_E_DEVICE);
  if (!have) return MRP_LL_E_DEVICE;
  c->store.assign(static_cast<size_t>(std::max(n, 0)), std::vector<int32_t>());
  return MRP_LL_SUCCESS;
}
int mrp_ll_sipp_table_create(mrp_ll_ctx*, int32_t, mrp_ll_sipp_table** out) {
  *out = new mrp_ll_sipp_table();
  return MRP_LL_SUCCESS;
}
int mrp_ll_sipp_table_add(mrp_ll_sipp_table* t, int32_t x, int32_t y, int32_t s, int32_t e) {
  t->add(x, y, s, e);
  return MRP_LL_SUCCESS;
}
void mrp_ll_sipp_table_destroy(mrp_ll_sipp_table* t) { delete t; }
int mrp_ll_get_stats(const mrp_ll_ctx* c, mrp_ll_stats* out) {
  *out = c->stats;
  return MRP_LL_SUCCESS;
}
int mrp_ll_reset_stats(mrp_ll_ctx* c) {
  std::memset(&c->stats, 0, sizeof(c->stats));
  return MRP_LL_SUCCESS;
}
}
