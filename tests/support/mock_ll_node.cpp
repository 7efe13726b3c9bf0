// TEST INFRASTRUCTURE ONLY — the oracle-backed stand-in for libmrp_ll.so with mrp_ll_submit_scan (mock_ll_scan.cpp) plus
// mrp_ll_submit_node.  The answers are mock_ll_scan.cpp's — the oracle's scan of the child, which is what a truthful
// MRP_LL_JOB_SCAN_FROM_PARENT job returns —; what this file adds is a CHECK OF WHAT THE DRIVER SENT with every flagged job,
// against the parent node assembled from the slots the job names in the mock's path store:
//   parent_count  == the oracle's conflict count of the parent solution,
//   clean_before  <= the time of the parent's first conflict (nothing in the parent conflicts before it),
//   path_ids[agent_idx] holds the replaced path (the one the driver still ships as the agent's table entry).
// A mismatch aborts the process, and with it the test.  mock_ll_node_counts reports how many calls and flagged jobs came.
#include "mock_ll_scan.cpp"

#include <atomic>

namespace {
std::atomic<int64_t> g_nodeCalls{0}, g_nodeFlagged{0};

[[noreturn]] void nodeFail(const char* what, const mrp_ll_job& j, long got, long want) {
  std::fprintf(stderr, "mock_ll_node: %s (agent %d of %d): got %ld, want %ld\n", what, j.agent_idx, j.n_agents, got, want);
  std::abort();
}
}  // namespace

extern "C" void mock_ll_node_counts(int64_t* calls, int64_t* flagged) {
  *calls = g_nodeCalls.load();
  *flagged = g_nodeFlagged.load();
}

extern "C" int mrp_ll_submit_node(mrp_ll_ctx* c, int32_t tag, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res,
                                  mrp_ll_conflict* conflicts, const mrp_ll_constraint_ref* sets, const mrp_ll_scan_base* bases,
                                  int32_t* ticket) {
  (void)sets;  // (the mock has no constraint store: the drivers never name a set here)
  g_nodeCalls += 1;
  std::vector<uint8_t> bad(static_cast<size_t>(std::max(n, 0)), 0);
  for (int32_t i = 0; i < n; ++i) {
    const mrp_ll_job& j = jobs[i];
    if (!(j.flags & MRP_LL_JOB_SCAN_FROM_PARENT)) continue;
    g_nodeFlagged += 1;
    const int nStore = static_cast<int>(c->store.size());
    bool valid = bases && conflicts && (j.flags & MRP_LL_JOB_SCAN_CONFLICTS) && j.path_ids && j.path_len && j.n_agents >= 1 &&
                 j.agent_idx >= 0 && j.agent_idx < j.n_agents && bases[i].parent_count >= 0 && bases[i].clean_before >= 0;
    for (int a = 0; valid && a < j.n_agents; ++a)
      valid = j.path_ids[a] >= 0 && j.path_ids[a] < nStore && j.path_len[a] >= 1 && !c->store[j.path_ids[a]].empty();
    if (!valid) {
      bad[i] = 1;
      continue;
    }
    // the parent node, from the slots the job names
    std::vector<int32_t> len, xy;
    for (int a = 0; a < j.n_agents; ++a) {
      const std::vector<int32_t>& p = c->store[j.path_ids[a]];
      len.push_back(static_cast<int32_t>(p.size() / 2));
      xy.insert(xy.end(), p.begin(), p.end());
    }
    int32_t w[10];
    oracle_conflict_scan(j.n_agents, len.data(), xy.data(), w);
    if (bases[i].parent_count != w[9]) nodeFail("parent_count is not the parent's conflict count", j, bases[i].parent_count, w[9]);
    if (w[0] && bases[i].clean_before > w[1]) nodeFail("the parent conflicts before clean_before", j, bases[i].clean_before, w[1]);
    const std::vector<int32_t>& old = c->store[j.path_ids[j.agent_idx]];
    const int a = j.agent_idx;
    if (static_cast<int32_t>(old.size() / 2) != j.path_len[a]) nodeFail("the slot does not hold the replaced path (length)", j, old.size() / 2, j.path_len[a]);
    if (j.path_xy && j.path_xy[a] && std::memcmp(old.data(), j.path_xy[a], old.size() * sizeof(int32_t)) != 0)
      nodeFail("the slot does not hold the replaced path (cells)", j, 0, 0);
  }
  const int rc = mrp_ll_submit_scan(c, tag, n, jobs, res, conflicts, ticket);
  if (rc != MRP_LL_SUCCESS) return rc;
  for (int32_t i = 0; i < n; ++i)
    if (bad[i]) {
      res[i].status = MRP_LL_BAD_JOB;
      std::memset(&conflicts[i], 0, sizeof(conflicts[i]));
      conflicts[i].found = -1;
    }
  return MRP_LL_SUCCESS;
}
