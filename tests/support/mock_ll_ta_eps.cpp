// TEST INFRASTRUCTURE ONLY — mock_ll_ta.cpp plus what the ECBS-TA driver (csrc/hl/mrp_hl_ecbs_ta.cpp) asks of the engine
// beyond it:
//   MRP_LL_ASTAR_EPS_TA jobs      through the checker's single search (ecbs_ta_check.cpp's ecbs_ta_ll_search, a translation
//                                 unit of its own) with the job's shipped focal context
//   mrp_ll_ta_eps_root_batch      agent after agent through the same search, each with the paths before it, budget shared, the
//                                 root ended behind the first agent without a path, conflicts by oracle_conflict_scan
// mock_ll_ta.cpp defines mrp_ll_search_batch itself, so this file cannot define it again: the test links with
// -Wl,--wrap=mrp_ll_search_batch, which sends the driver's calls to __wrap_mrp_ll_search_batch below; every other job goes on
// to mock_ll_ta.cpp's own.
#include "mock_ll_ta.cpp"

extern "C" int ecbs_ta_ll_search(int dimx, int dimy, int nObst, const int32_t* obstXY, int startX, int startY, int hasGoal, int goalX,
                                 int goalY, int nVC, const int32_t* vc, int nEC, const int32_t* ec, float w, int agentIdx, int nAgents,
                                 const int32_t* pathLen, const int32_t* pathXY, int64_t capExpansions, int32_t* out, int64_t* expanded,
                                 int32_t* statesTXY, int32_t* actions, int32_t* actionCosts, int cap);

namespace {

void taEpsSearch(mrp_ll_ctx* c, const mrp_ll_job& j, mrp_ll_result& r) {
  const MockMap& m = c->maps[j.map_id];
  const bool hasGoal = !(j.flags & MRP_LL_JOB_NO_GOAL);
  std::vector<int32_t> len, xy;
  for (int a = 0; a < j.n_agents; ++a) {
    len.push_back(j.path_len[a]);
    for (int k = 0; k < 2 * j.path_len[a]; ++k) xy.push_back(j.path_xy[a][k]);
  }
  xy.push_back(0);
  int32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int64_t expanded = 0;
  const int cap = 2048;
  std::vector<int32_t> st(3 * cap), ac(cap), co(cap);
  const int rc = ecbs_ta_ll_search(m.dimx, m.dimy, static_cast<int>(m.obst.size() / 2), m.obst.data(), j.start_x, j.start_y,
                                   hasGoal ? 1 : 0, j.goal_x, j.goal_y, j.n_vertex_constraints, j.vertex_constraints,
                                   j.n_edge_constraints, j.edge_constraints, j.w, j.agent_idx, j.n_agents, len.data(), xy.data(),
                                   j.max_expansions, out, &expanded, st.data(), ac.data(), co.data(), cap);
  r.expanded = expanded;
  r.tier = 1;
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

}  // namespace

extern "C" int __wrap_mrp_ll_search_batch(mrp_ll_ctx* c, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res) {
  taCall("search_batch");
  for (int i = 0; i < n; ++i) {
    if (jobs[i].algo == MRP_LL_ASTAR_EPS_TA && jobs[i].map_id >= 0 && jobs[i].map_id < static_cast<int>(c->maps.size())) {
      taEpsSearch(c, jobs[i], res[i]);
    } else {
      mrp_ll_search_batch(c, 1, jobs + i, res + i);
    }
  }
  return MRP_LL_SUCCESS;
}

extern "C" int mrp_ll_ta_eps_root_batch(mrp_ll_ctx* c, float w, int32_t nRoots, const mrp_ll_ta_root* roots, mrp_ll_conflict* conflicts,
                                        int32_t* planned) {
  taCall("ta_eps_root_batch");
  for (int r = 0; r < nRoots; ++r) {
    const mrp_ll_ta_root& R = roots[r];
    std::memset(&conflicts[r], 0, sizeof(mrp_ll_conflict));
    conflicts[r].found = -1;
    planned[r] = 0;
    int64_t budget = R.max_expansions;
    bool all = true;
    std::vector<std::vector<int32_t>> paths(R.n_agents);
    std::vector<int32_t> len(R.n_agents, 0);
    std::vector<const int32_t*> xy(R.n_agents, nullptr);
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
      j.algo = MRP_LL_ASTAR_EPS_TA;
      j.w = w;
      j.agent_idx = a;
      j.start_x = R.starts_xy[2 * a];
      j.start_y = R.starts_xy[2 * a + 1];
      j.max_expansions = budget;
      j.n_agents = R.n_agents;
      j.path_len = len.data();
      j.path_xy = xy.data();
      if (R.heuristic_ids[a] >= 0) {
        j.goal_x = R.goals_xy[2 * a];
        j.goal_y = R.goals_xy[2 * a + 1];
      } else {
        j.flags = MRP_LL_JOB_NO_GOAL;
      }
      taEpsSearch(c, j, res);
      planned[r] += 1;
      if (budget >= 0) budget = budget > res.expanded ? budget - res.expanded : 0;
      if (res.status != MRP_LL_OK) {
        all = false;
        continue;
      }
      for (int k = 0; k < res.n_states; ++k) paths[a].insert(paths[a].end(), {res.states_txy[3 * k + 1], res.states_txy[3 * k + 2]});
      len[a] = res.n_states;
      xy[a] = paths[a].data();
    }
    if (all) {
      std::vector<int32_t> flat;
      for (const auto& p : paths) flat.insert(flat.end(), p.begin(), p.end());
      int32_t o[10];
      oracle_conflict_scan(R.n_agents, len.data(), flat.data(), o);
      std::memcpy(&conflicts[r], o, sizeof(o));
    }
  }
  return MRP_LL_SUCCESS;
}
