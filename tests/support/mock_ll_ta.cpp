// TEST INFRASTRUCTURE ONLY — mock_ll.cpp plus the engine calls the CBS-TA driver (csrc/hl/mrp_hl_ta.cpp) makes, on the CPU:
//   mrp_ll_compute_heuristics / _heuristic_lookup   the oracle's shortest-path tables (oracle/ta_restated.hpp)
//   mrp_ll_assign_batch / _assign_series_*          the engine's own host-side series (csrc/host/assign_series.h), its problems
//                                                   solved by the assignment wave program on the CPU (ta_series_emu.h); a
//                                                   gather-form problem is turned into its cost rows first
//   mrp_ll_search_batch                             MRP_LL_ASTAR_TA jobs through oracle_ta_ll_search, the rest through mock_ll.cpp
//   mrp_ll_ta_root_batch                            agent after agent through the same search, budget shared, the root ended
//                                                   behind the first agent without a path, conflicts by oracle_conflict_scan
// MRP_MOCK_TA_CALLS=<file>: every call appends its name (a test counts the three calls of a round).
#define mrp_ll_search_batch mock_base_search_batch
#include "mock_ll.cpp"
#undef mrp_ll_search_batch

#include <climits>
#include <unordered_set>

#include "ta_restated.hpp"

// mock_ll_ta_assign.cpp (a translation unit of its own: the engine's packer headers define mrp_ll_sipp_table, and so does
// mock_ll.cpp): problems in the matrix form through the series of csrc/host/assign_series.h and the emulated wave program
extern "C" int mock_ta_solve_batch(int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results);
extern "C" int mock_ta_series_create(const void* owner, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_series** out);
extern "C" int mock_ta_series_next(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results);
extern "C" void mock_ta_series_destroy(mrp_ll_assign_series* s);

extern "C" int oracle_ta_ll_search(int dimx, int dimy, int nObst, const int32_t* obstXY, int startX, int startY, int hasGoal, int goalX,
                                   int goalY, int nVC, const int32_t* vc, int nEC, const int32_t* ec, int64_t capExpansions,
                                   int32_t* out, int64_t* expanded, int32_t* statesTXY, int32_t* actions, int32_t* actionCosts, int cap);

namespace {

struct TaTable {
  int32_t mapId;
  int32_t gx, gy;
  std::vector<int> dist;
};
std::mutex g_taMu;
std::map<const mrp_ll_ctx*, std::vector<TaTable>> g_tables;  // (mock_ll.cpp's context has no room for them)

void taCall(const char* name) {
  if (const char* file = std::getenv("MRP_MOCK_TA_CALLS"))
    if (FILE* f = std::fopen(file, "a")) {
      std::fprintf(f, "%s\n", name);
      std::fclose(f);
    }
}
std::vector<TaTable>& tablesOf(const mrp_ll_ctx* c) {
  std::lock_guard<std::mutex> lock(g_taMu);
  return g_tables[c];
}

void taSearch(mrp_ll_ctx* c, const mrp_ll_job& j, mrp_ll_result& r) {
  const MockMap& m = c->maps[j.map_id];
  const bool hasGoal = !(j.flags & MRP_LL_JOB_NO_GOAL);
  int32_t out[4] = {0, 0, 0, 0};
  int64_t expanded = 0;
  const int cap = 2048;
  std::vector<int32_t> st(3 * cap), ac(cap), co(cap);
  const int rc = oracle_ta_ll_search(m.dimx, m.dimy, static_cast<int>(m.obst.size() / 2), m.obst.data(), j.start_x, j.start_y,
                                     hasGoal ? 1 : 0, j.goal_x, j.goal_y, j.n_vertex_constraints, j.vertex_constraints,
                                     j.n_edge_constraints, j.edge_constraints, j.max_expansions, out, &expanded, st.data(), ac.data(),
                                     co.data(), cap);
  r.expanded = expanded;
  r.tier = 0;
  r.cost = r.fmin = r.n_states = 0;
  c->stats.jobs += 1;
  c->stats.expansions += expanded;
  if (rc == -1) {
    r.status = MRP_LL_CAP_EXPANSIONS;
    return;
  }
  r.status = out[0] ? MRP_LL_OK : MRP_LL_NO_SOLUTION;
  if (!out[0]) return;
  r.cost = out[1];
  r.fmin = out[2];
  r.n_states = out[3];
  for (int k = 0; k < r.n_states && k < r.states_cap; ++k) {
    if (r.states_txy) std::memcpy(r.states_txy + 3 * k, st.data() + 3 * k, 12);
    if (r.actions && k + 1 < r.n_states) r.actions[k] = ac[k];
    if (r.action_costs && k + 1 < r.n_states) r.action_costs[k] = co[k];
  }
  if (r.n_states > r.states_cap && (r.states_txy || r.actions)) r.status = MRP_LL_PATH_TRUNCATED;
}

// a problem in the matrix form (`cost` owns the rows of a gather-form one)
mrp_ll_assign_problem asMatrix(const mrp_ll_ctx* c, const mrp_ll_assign_problem& p, std::vector<int32_t>& cost) {
  if (p.cost) return p;
  const std::vector<TaTable>& tabs = tablesOf(c);
  cost.assign(static_cast<size_t>(p.n_agents) * p.n_tasks + 1, 0);
  for (int t = 0; t < p.n_tasks; ++t) {
    const TaTable& tab = tabs[p.heuristic_ids[t]];
    const int dimx = c->maps[tab.mapId].dimx;
    for (int a = 0; a < p.n_agents; ++a) {  // (ta_series_emu.h edge(): unreachable or not allowed is no edge)
      const int d = tab.dist[p.starts_xy[2 * a] + dimx * p.starts_xy[2 * a + 1]];
      const bool ok = !p.allowed || ((p.allowed[a] >> t) & 1);
      cost[static_cast<size_t>(a) * p.n_tasks + t] = (!ok || d == INT_MAX || d > 0xFFFE) ? MRP_LL_ASSIGN_NO_EDGE : d;
    }
  }
  mrp_ll_assign_problem q = p;
  q.cost = cost.data();
  q.heuristic_ids = nullptr;
  q.starts_xy = nullptr;
  q.allowed = nullptr;
  return q;
}

}  // namespace

extern "C" {

int mrp_ll_search_batch(mrp_ll_ctx* c, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res) {
  taCall("search_batch");
  for (int i = 0; i < n; ++i) {
    if (jobs[i].algo == MRP_LL_ASTAR_TA && jobs[i].map_id >= 0 && jobs[i].map_id < static_cast<int>(c->maps.size()))
      taSearch(c, jobs[i], res[i]);
    else
      mock_base_search_batch(c, 1, jobs + i, res + i);
  }
  return MRP_LL_SUCCESS;
}

int mrp_ll_compute_heuristics(mrp_ll_ctx* c, int32_t n, const int32_t* mapIds, const int32_t* goalsXY, int32_t* ids) {
  taCall("compute_heuristics");
  std::vector<TaTable>& tabs = tablesOf(c);
  for (int k = 0; k < n; ++k) {
    const MockMap& m = c->maps[mapIds[k]];
    std::unordered_set<oracle::mapf::Cell, oracle::mapf::CellHash> obst;
    for (size_t i = 0; i + 1 < m.obst.size(); i += 2) obst.insert(oracle::mapf::Cell{m.obst[i], m.obst[i + 1]});
    const oracle::mapf::Cell g{goalsXY[2 * k], goalsXY[2 * k + 1]};
    tabs.push_back(TaTable{mapIds[k], g.x, g.y, oracle::ta::shortestPathTable(m.dimx, m.dimy, obst, g)});
    ids[k] = static_cast<int32_t>(tabs.size()) - 1;
  }
  return MRP_LL_SUCCESS;
}
int mrp_ll_heuristic_lookup(mrp_ll_ctx* c, int32_t n, const int32_t* ids, const int32_t* cellsXY, int32_t* out) {
  const std::vector<TaTable>& tabs = tablesOf(c);
  for (int k = 0; k < n; ++k) out[k] = tabs[ids[k]].dist[cellsXY[2 * k] + c->maps[tabs[ids[k]].mapId].dimx * cellsXY[2 * k + 1]];
  return MRP_LL_SUCCESS;
}

int mrp_ll_assign_batch(mrp_ll_ctx* c, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results) {
  std::vector<std::vector<int32_t>> rows(static_cast<size_t>(n));
  std::vector<mrp_ll_assign_problem> ps;
  for (int k = 0; k < n; ++k) ps.push_back(asMatrix(c, problems[k], rows[k]));
  return mock_ta_solve_batch(n, ps.data(), results);
}
int mrp_ll_assign_series_create(mrp_ll_ctx* c, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_series** out) {
  taCall("assign_series_create");
  std::vector<std::vector<int32_t>> rows(static_cast<size_t>(n));
  std::vector<mrp_ll_assign_problem> ps;
  for (int k = 0; k < n; ++k) ps.push_back(asMatrix(c, problems[k], rows[k]));
  return mock_ta_series_create(c, n, ps.data(), out);
}
int mrp_ll_assign_series_next(mrp_ll_ctx*, int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results) {
  taCall("assign_series_next");
  return mock_ta_series_next(n, series, results);
}
void mrp_ll_assign_series_destroy(mrp_ll_assign_series* s) { mock_ta_series_destroy(s); }

int mrp_ll_ta_root_batch(mrp_ll_ctx* c, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts) {
  taCall("ta_root_batch");
  for (int r = 0; r < nRoots; ++r) {
    const mrp_ll_ta_root& R = roots[r];
    std::memset(&conflicts[r], 0, sizeof(mrp_ll_conflict));
    conflicts[r].found = -1;
    planned[r] = 0;
    int64_t budget = R.max_expansions;
    bool all = true;
    std::vector<int32_t> len, xy;
    for (int a = 0; a < R.n_agents; ++a) {
      mrp_ll_result& res = R.results[a];
      if (!all) {
        res.status = MRP_LL_NOT_RUN;
        res.cost = res.fmin = res.n_states = 0;
        res.expanded = 0;
        res.tier = 0;
        continue;
      }
      mrp_ll_job j;
      std::memset(&j, 0, sizeof(j));
      j.map_id = R.map_id;
      j.algo = MRP_LL_ASTAR_TA;
      j.start_x = R.starts_xy[2 * a];
      j.start_y = R.starts_xy[2 * a + 1];
      j.max_expansions = budget;
      if (R.heuristic_ids[a] >= 0) {
        j.goal_x = R.goals_xy[2 * a];
        j.goal_y = R.goals_xy[2 * a + 1];
      } else {
        j.flags = MRP_LL_JOB_NO_GOAL;
      }
      taSearch(c, j, res);
      planned[r] += 1;
      if (budget >= 0) budget = budget > res.expanded ? budget - res.expanded : 0;
      if (res.status != MRP_LL_OK) {
        all = false;
        continue;
      }
      len.push_back(res.n_states);
      for (int k = 0; k < res.n_states; ++k) {
        xy.push_back(res.states_txy[3 * k + 1]);
        xy.push_back(res.states_txy[3 * k + 2]);
      }
    }
    if (all) {
      int32_t o[10];
      oracle_conflict_scan(R.n_agents, len.data(), xy.data(), o);
      std::memcpy(&conflicts[r], o, sizeof(o));
    }
  }
  return MRP_LL_SUCCESS;
}

}  // extern "C"
