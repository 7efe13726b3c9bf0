// TEST INFRASTRUCTURE ONLY — the oracle-backed stand-in for libmrp_ll.so (mock_ll.cpp) plus mrp_ll_submit_scan: a flagged job
// is answered like any other, and its node's conflicts come from the oracle's getFirstConflict / focalHeuristic over the
// solution the engine would scan — the path the search found in place of agent_idx's, the MOCK'S PATH STORE for everybody
// else (not the tables the driver ships beside the ids: a driver that names a wrong slot gets a wrong answer here too).
#include "mock_ll.cpp"

extern "C" int mrp_ll_submit_scan(mrp_ll_ctx* c, int32_t tag, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res,
                                  mrp_ll_conflict* conflicts, int32_t* ticket) {
  if (tag < 0 || tag > 3 || (n > 0 && !conflicts)) return MRP_LL_E_INVALID;
  // The engine keeps one book of finished tickets and stamps the tag on the ticket; mock_ll.cpp keeps two, one per poll call
  // (doneTickets for mrp_ll_poll_any, g_coDone for mrp_ll_poll_any_tagged), and tag 0 is both a lone worker's and a leading
  // co-worker's.  So the ticket has to go into the book its owner polls: the tagged one once any co-worker has used this
  // context (every worker's first submissions are its root steps, which go through mrp_ll_submit_tagged there).
  bool tagged = false;
  {
    std::lock_guard<std::mutex> lock(g_coMu);
    for (int t = 0; t < 4; ++t) tagged = tagged || g_coDone[t].count(c) != 0;
  }
  const int rc = tagged ? mrp_ll_submit_tagged(c, tag, n, jobs, res, ticket) : mrp_ll_submit(c, n, jobs, res, ticket);
  if (rc != MRP_LL_SUCCESS) return rc;
  for (int32_t i = 0; i < n; ++i) {
    const mrp_ll_job& j = jobs[i];
    if (!(j.flags & MRP_LL_JOB_SCAN_CONFLICTS)) continue;
    mrp_ll_conflict& o = conflicts[i];
    std::memset(&o, 0, sizeof(o));
    o.found = -1;
    bool valid = j.algo == MRP_LL_ASTAR_EPS && j.path_ids && j.path_len && !c->store.empty() && j.n_agents >= 1 &&
                 j.agent_idx >= 0 && j.agent_idx < j.n_agents && !(j.flags & MRP_LL_JOB_ROOT_CHAIN);
    for (int a = 0; valid && a < j.n_agents; ++a)
      if (a != j.agent_idx)
        valid = j.path_ids[a] >= 0 && j.path_ids[a] < static_cast<int>(c->store.size()) && j.path_len[a] >= 1 &&
                !c->store[j.path_ids[a]].empty();
    if (!valid) {
      res[i].status = MRP_LL_BAD_JOB;
      continue;
    }
    if (res[i].status != MRP_LL_OK) continue;
    std::vector<int32_t> len, xy;
    for (int a = 0; a < j.n_agents; ++a) {
      if (a == j.agent_idx) {
        len.push_back(res[i].n_states);
        for (int k = 0; k < res[i].n_states; ++k) {
          xy.push_back(res[i].states_txy[3 * k + 1]);
          xy.push_back(res[i].states_txy[3 * k + 2]);
        }
      } else {
        const std::vector<int32_t>& p = c->store[j.path_ids[a]];
        len.push_back(static_cast<int32_t>(p.size() / 2));
        xy.insert(xy.end(), p.begin(), p.end());
      }
    }
    int32_t w[10];
    oracle_conflict_scan(j.n_agents, len.data(), xy.data(), w);
    std::memcpy(&o, w, sizeof(o));
  }
  return MRP_LL_SUCCESS;
}
