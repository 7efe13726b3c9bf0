// TEST INFRASTRUCTURE ONLY — the oracle-backed stand-in for libmrp_ll.so (mock_ll.cpp, with mock_ll_scan.cpp's
// mrp_ll_submit_scan) plus the constraint store: mrp_ll_constraint_store_reserve / mrp_ll_submit_sets.  Sets are kept on the
// host, per context; a job that names its set is answered with the oracle's search over the UNION — the contents of its base
// slot followed by the job's own arrays — so a driver that names a wrong slot, or ships a wrong addition, gets a wrong
// answer here too.  The rejections are the engine's (include/mrp_ll.h), except that the mock runs every job inside the
// submit call, so no writer is ever still in flight.
#include "mock_ll_scan.cpp"

namespace {
struct MockSet {
  bool written = false;
  int32_t mapId = -1, gx = 0, gy = 0;
  std::vector<int32_t> vertex, edge;
};
struct MockSetStore {
  int32_t wordsPerSlot = 0;
  std::vector<MockSet> slots;
};
std::mutex g_setMu;
std::map<mrp_ll_ctx*, MockSetStore> g_setStores;
int64_t g_maxWords = 0;  // the largest union (in constraints) an accepted job had
int64_t g_flaggedJobs = 0, g_bySetJobs = 0;  // accepted MRP_LL_JOB_CONSTRAINT_SET jobs; those of them that named a base
}  // namespace

extern "C" {
// Since the last reset: the accepted jobs that arrived BY SET — they named a base slot and shipped only their additions —
// and all accepted jobs with MRP_LL_JOB_CONSTRAINT_SET (the others shipped their whole set and only left it in a slot).
int64_t mock_ll_sets_jobs(void) {
  std::lock_guard<std::mutex> lock(g_setMu);
  return g_bySetJobs;
}
int64_t mock_ll_sets_flagged_jobs(void) {
  std::lock_guard<std::mutex> lock(g_setMu);
  return g_flaggedJobs;
}
int64_t mock_ll_sets_max_words(void) {
  std::lock_guard<std::mutex> lock(g_setMu);
  return g_maxWords;
}
void mock_ll_sets_reset(void) {
  std::lock_guard<std::mutex> lock(g_setMu);
  g_flaggedJobs = g_bySetJobs = g_maxWords = 0;
}

int mrp_ll_constraint_store_reserve(mrp_ll_ctx* c, int32_t nSlots, int32_t wordsPerSlot) {
  if (!c) return MRP_LL_E_INVALID;
  const bool bad = nSlots < 0 || wordsPerSlot < 0 || wordsPerSlot > 2048 || (nSlots > 0 && wordsPerSlot == 0);
  callLog(c, "constraint_store_reserve %d %d -> %d", nSlots, wordsPerSlot, bad ? MRP_LL_E_INVALID : MRP_LL_SUCCESS);
  if (bad) return MRP_LL_E_INVALID;
  {  // WORKAROUND for mock_ll.cpp, which this file may not change: its mrp_ll_destroy never forgets a context's co-worker
     // books (g_coDone), and a new context may live where a destroyed one did.  The `tagged` test in mrp_ll_submit_sets
     // below — and the same test in mock_ll_scan.cpp — would then take a lone worker for a co-worker and file its tickets
     // where it never looks.  A driver reserves its store before its first submission, so the stale (empty) books go here;
     // the fix proper is to erase them in mock_ll.cpp's mrp_ll_destroy.
    std::lock_guard<std::mutex> lock(g_coMu);
    for (int t = 0; t < 4; ++t) {
      auto it = g_coDone[t].find(c);
      if (it != g_coDone[t].end() && it->second.empty()) g_coDone[t].erase(it);
    }
  }
  std::lock_guard<std::mutex> lock(g_setMu);
  if (nSlots == 0) {
    g_setStores.erase(c);
    return MRP_LL_SUCCESS;
  }
  MockSetStore& s = g_setStores[c];
  s.wordsPerSlot = wordsPerSlot;
  s.slots.assign(static_cast<size_t>(nSlots), MockSet());
  return MRP_LL_SUCCESS;
}

int mrp_ll_submit_sets(mrp_ll_ctx* c, int32_t tag, int32_t n, const mrp_ll_job* jobs, mrp_ll_result* res,
                       mrp_ll_conflict* conflicts, const mrp_ll_constraint_ref* sets, int32_t* ticket) {
  if (tag < 0 || tag > 3) return MRP_LL_E_INVALID;
  std::vector<mrp_ll_job> flat(jobs, jobs + n);
  std::vector<std::vector<int32_t>> unionV(static_cast<size_t>(n)), unionE(static_cast<size_t>(n));
  std::vector<int32_t> resultSlot(static_cast<size_t>(n), -1);
  std::vector<uint8_t> bySet(static_cast<size_t>(n), 0), withBase(static_cast<size_t>(n), 0);
  {
    std::lock_guard<std::mutex> lock(g_setMu);
    auto it = g_setStores.find(c);
    for (int32_t i = 0; i < n; ++i) {
      mrp_ll_job& j = flat[i];
      if (!(j.flags & MRP_LL_JOB_CONSTRAINT_SET)) continue;
      j.flags &= ~MRP_LL_JOB_CONSTRAINT_SET;
      bool ok = sets != nullptr && it != g_setStores.end() && (j.algo == MRP_LL_ASTAR || j.algo == MRP_LL_ASTAR_EPS) &&
                !(j.flags & MRP_LL_JOB_ROOT_CHAIN);
      const MockSet* base = nullptr;
      if (ok) {
        const int32_t nSlots = static_cast<int32_t>(it->second.slots.size());
        const mrp_ll_constraint_ref& r = sets[i];
        ok = r.base_set_id >= -1 && r.base_set_id < nSlots && r.result_set_id >= -1 && r.result_set_id < nSlots &&
             !(r.base_set_id >= 0 && r.base_set_id == r.result_set_id);
        if (ok && r.base_set_id >= 0) {
          base = &it->second.slots[r.base_set_id];
          ok = base->written && base->mapId == j.map_id && base->gx == j.goal_x && base->gy == j.goal_y;
        }
      }
      if (ok) {
        if (base) {
          unionV[i] = base->vertex;
          unionE[i] = base->edge;
        }
        unionV[i].insert(unionV[i].end(), j.vertex_constraints, j.vertex_constraints + 3 * j.n_vertex_constraints);
        unionE[i].insert(unionE[i].end(), j.edge_constraints, j.edge_constraints + 5 * j.n_edge_constraints);
        ok = static_cast<int32_t>(unionV[i].size() / 3 + unionE[i].size() / 5) <= it->second.wordsPerSlot;
      }
      if (!ok) {
        j.map_id = -1;  // MRP_LL_BAD_JOB, not run
        continue;
      }
      j.n_vertex_constraints = static_cast<int32_t>(unionV[i].size() / 3);
      j.vertex_constraints = unionV[i].data();
      j.n_edge_constraints = static_cast<int32_t>(unionE[i].size() / 5);
      j.edge_constraints = unionE[i].data();
      resultSlot[i] = sets[i].result_set_id;
      bySet[i] = 1;
      withBase[i] = base ? 1 : 0;
    }
  }
  int rc;
  if (conflicts) {
    rc = mrp_ll_submit_scan(c, tag, n, flat.data(), res, conflicts, ticket);
  } else {  // (as mock_ll_scan.cpp: the ticket goes into the book its owner polls)
    bool tagged = false;
    {
      std::lock_guard<std::mutex> lock(g_coMu);
      for (int t = 0; t < 4; ++t) tagged = tagged || g_coDone[t].count(c) != 0;
    }
    rc = tagged ? mrp_ll_submit_tagged(c, tag, n, flat.data(), res, ticket) : mrp_ll_submit(c, n, flat.data(), res, ticket);
  }
  if (rc != MRP_LL_SUCCESS) return rc;
  std::lock_guard<std::mutex> lock(g_setMu);
  auto it = g_setStores.find(c);
  for (int32_t i = 0; i < n; ++i) {
    if (!bySet[i]) continue;
    g_flaggedJobs += 1;
    g_maxWords = std::max<int64_t>(g_maxWords, static_cast<int64_t>(unionV[i].size() / 3 + unionE[i].size() / 5));
    g_bySetJobs += withBase[i];
    if (resultSlot[i] < 0 || it == g_setStores.end()) continue;
    MockSet& s = it->second.slots[resultSlot[i]];
    s.written = true;
    s.mapId = jobs[i].map_id;
    s.gx = jobs[i].goal_x;
    s.gy = jobs[i].goal_y;
    s.vertex = unionV[i];
    s.edge = unionE[i];
  }
  return MRP_LL_SUCCESS;
}
}
