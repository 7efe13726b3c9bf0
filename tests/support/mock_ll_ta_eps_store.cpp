// TEST INFRASTRUCTURE ONLY — mock_ll_ta_eps.cpp plus a path store that keeps a path per slot, for the ECBS-TA driver under
// MRP_HL_TA_DEVICE_PATHS (csrc/hl/mrp_hl_ecbs_ta.cpp):
//   mrp_ll_path_store_reserve             n empty slots
//   MRP_LL_ASTAR_EPS_TA jobs              a job with path_ids is resolved to the slots' paths and run as mock_ll_ta_eps.cpp runs a
//                                         shipped one; with MRP_LL_JOB_STORE_RESULT a found path stays in slot result_path_id
//   mrp_ll_ta_eps_root_batch_stored       mock_ll_ta_eps.cpp's root, then the planned agents' paths into their slots
// A slot-lifetime bug is loud: MRP_LL_BAD_JOB for a job that names a slot outside the store, a slot nobody has written, a slot
// whose path has another length than the job's path_len says (it was written again since), or a slot that a job of the same
// batch writes (on the device the two would race).
// MRP_MOCK_TA_CALLS=<file> also receives one line per MRP_LL_ASTAR_EPS_TA job with a context: job_by_id or job_shipped.
// mock_ll_ta_eps.cpp's own entry points are included under other names (the trick mock_ll_ta.cpp uses on mock_ll.cpp); the
// test links with -Wl,--wrap=mrp_ll_search_batch as for mock_ll_ta_eps.cpp.
#define __wrap_mrp_ll_search_batch mock_eps_search_batch
#define mrp_ll_ta_eps_root_batch mock_eps_root_batch
#define mrp_ll_path_store_reserve mock_base_path_store_reserve
#include "mock_ll_ta_eps.cpp"
#undef __wrap_mrp_ll_search_batch
#undef mrp_ll_ta_eps_root_batch
#undef mrp_ll_path_store_reserve

#include <set>

namespace {

struct SlotStore {
  std::vector<std::vector<int32_t>> xy;  // per slot x, y, x, y, ...
  std::vector<char> written;
};
std::map<const mrp_ll_ctx*, SlotStore> g_slotStores;

SlotStore& slotsOf(const mrp_ll_ctx* c) {
  std::lock_guard<std::mutex> lock(g_taMu);
  return g_slotStores[c];
}

void refuse(mrp_ll_result& r) {
  r.status = MRP_LL_BAD_JOB;
  r.cost = r.fmin = r.n_states = 0;
  r.expanded = 0;
  r.tier = 0;
}

void keepPath(SlotStore& S, int32_t slot, const mrp_ll_result& r) {
  std::vector<int32_t>& p = S.xy[static_cast<size_t>(slot)];
  p.clear();
  for (int k = 0; k < r.n_states; ++k) p.insert(p.end(), {r.states_txy[3 * k + 1], r.states_txy[3 * k + 2]});
  S.written[static_cast<size_t>(slot)] = 1;
}

}  // namespace

extern "C" int mrp_ll_path_store_reserve(mrp_ll_ctx* c, int32_t n) {
  taCall("path_store_reserve");
  if (n < 1) return MRP_LL_E_INVALID;
  SlotStore& S = slotsOf(c);
  S.xy.assign(static_cast<size_t>(n), std::vector<int32_t>());
  S.written.assign(static_cast<size_t>(n), 0);
  return MRP_LL_SUCCESS;
}

extern "C" int __wrap_mrp_ll_search_batch(mrp_ll_ctx* c, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res) {
  SlotStore& S = slotsOf(c);
  const int32_t nSlots = static_cast<int32_t>(S.xy.size());
  std::set<int32_t> writtenHere;
  for (int i = 0; i < n; ++i)
    if (jobs[i].algo == MRP_LL_ASTAR_EPS_TA && (jobs[i].flags & MRP_LL_JOB_STORE_RESULT)) writtenHere.insert(jobs[i].result_path_id);
  taCall("search_batch");
  std::vector<std::pair<int32_t, int>> toStore;  // (slot, job): the stores happen behind every search of the batch
  for (int i = 0; i < n; ++i) {
    const mrp_ll_job& j = jobs[i];
    if (j.algo != MRP_LL_ASTAR_EPS_TA || j.map_id < 0 || j.map_id >= static_cast<int>(c->maps.size())) {
      mrp_ll_search_batch(c, 1, jobs + i, res + i);
      continue;
    }
    if ((j.flags & MRP_LL_JOB_STORE_RESULT) && (j.result_path_id < 0 || j.result_path_id >= nSlots)) {
      refuse(res[i]);
      continue;
    }
    mrp_ll_job one = j;
    std::vector<const int32_t*> xy;
    bool ok = true, hasContext = false;
    for (int a = 0; a < j.n_agents; ++a) hasContext = hasContext || (a != j.agent_idx && j.path_len[a] > 0);
    if (j.path_ids) {
      static const int32_t none[2] = {0, 0};
      xy.assign(static_cast<size_t>(j.n_agents), none);
      for (int a = 0; a < j.n_agents && ok; ++a) {
        if (a == j.agent_idx || j.path_len[a] <= 0) continue;
        const int32_t s = j.path_ids[a];
        ok = s >= 0 && s < nSlots && S.written[static_cast<size_t>(s)] && !writtenHere.count(s) &&
             static_cast<int32_t>(S.xy[static_cast<size_t>(s)].size()) == 2 * j.path_len[a];
        if (ok) xy[static_cast<size_t>(a)] = S.xy[static_cast<size_t>(s)].data();
      }
      one.path_xy = xy.data();
      one.path_ids = nullptr;
    }
    if (!ok) {
      refuse(res[i]);
      continue;
    }
    if (hasContext) taCall(j.path_ids ? "job_by_id" : "job_shipped");
    one.flags &= ~MRP_LL_JOB_STORE_RESULT;
    taEpsSearch(c, one, res[i]);
    if ((j.flags & MRP_LL_JOB_STORE_RESULT) && res[i].status == MRP_LL_OK) toStore.push_back({j.result_path_id, i});
  }
  for (const auto& w : toStore) keepPath(S, w.first, res[w.second]);
  return MRP_LL_SUCCESS;
}

extern "C" int mrp_ll_ta_eps_root_batch_stored(mrp_ll_ctx* c, float w, int32_t nRoots, const mrp_ll_ta_root* roots,
                                               mrp_ll_conflict* conflicts, int32_t* planned, const int32_t* const* ids) {
  SlotStore& S = slotsOf(c);
  const int32_t nSlots = static_cast<int32_t>(S.xy.size());
  const int rc = mock_eps_root_batch(c, w, nRoots, roots, conflicts, planned);  // (logs ta_eps_root_batch)
  if (rc != MRP_LL_SUCCESS) return rc;
  for (int r = 0; r < nRoots; ++r) {
    if (!ids || !ids[r]) continue;
    bool good = true;
    for (int a = 0; a < roots[r].n_agents; ++a) good = good && ids[r][a] >= -1 && ids[r][a] < nSlots;
    if (!good) {  // refused: nothing is told, no slot touched
      for (int a = 0; a < roots[r].n_agents; ++a) refuse(roots[r].results[a]);
      std::memset(&conflicts[r], 0, sizeof(mrp_ll_conflict));
      conflicts[r].found = -1;
      planned[r] = 0;
      continue;
    }
    for (int a = 0; a < planned[r]; ++a)
      if (ids[r][a] >= 0 && roots[r].results[a].status == MRP_LL_OK) keepPath(S, ids[r][a], roots[r].results[a]);
  }
  return MRP_LL_SUCCESS;
}

extern "C" int mrp_ll_ta_eps_root_batch(mrp_ll_ctx* c, float w, int32_t nRoots, const mrp_ll_ta_root* roots, mrp_ll_conflict* conflicts,
                                        int32_t* planned) {
  return mrp_ll_ta_eps_root_batch_stored(c, w, nRoots, roots, conflicts, planned, nullptr);
}
