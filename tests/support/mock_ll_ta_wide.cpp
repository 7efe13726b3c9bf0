// TEST INFRASTRUCTURE ONLY — mock_ll_ta.cpp plus the engine's wide entry points the task-assignment drivers reach for
// instances beyond 64 agents or tasks:
//   mrp_ll_assign_series_create_w   the wide series of csrc/host/assign_series.h over the WIDE assignment wave program on the
//                                   CPU (mock_ll_ta_assign_wide.cpp); a gather-form problem is turned into its cost rows first
//   mrp_ll_assign_series_next       narrow and wide series together in one call (mock_ll_ta.cpp's own takes narrow ones only;
//                                   it is included under another name)
//   mrp_ll_ta_root_batch_w          mock_ll_ta.cpp's root call, which has no agent limit of its own
// MRP_MOCK_TA_CALLS: the _w calls append "assign_series_create_w" / "ta_root_batch_w" and nothing else (the narrow body they
// run is kept from appending its own name), so a test can count narrow and wide root calls apart.
// MOCK_TA_WIDE_BASE: the stand-in this one extends (mock_ll_ta_eps_wide.cpp sets mock_ll_ta_eps.cpp).  Its
// mrp_ll_assign_series_next is compiled under another name, the way mock_ll_ta.cpp takes over mock_ll.cpp's
// mrp_ll_search_batch.  -DMOCK_NO_WIDE_ROOT: an engine with the wide series but without wide root calls.
#ifndef MOCK_TA_WIDE_BASE
#define MOCK_TA_WIDE_BASE "mock_ll_ta.cpp"
#endif
#define mrp_ll_assign_series_next mock_narrow_assign_series_next
#include MOCK_TA_WIDE_BASE
#undef mrp_ll_assign_series_next

extern "C" int mock_ta_series_create_w(const void* owner, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_series** out);
extern "C" int mock_ta_series_next_mixed(int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results);

namespace {

// Runs `body` with MRP_MOCK_TA_CALLS unset: what it would append is the caller's to say.
template <class F>
int quietly(F body) {
  const char* file = std::getenv("MRP_MOCK_TA_CALLS");
  const std::string keep = file ? file : "";
  if (file) unsetenv("MRP_MOCK_TA_CALLS");
  const int rc = body();
  if (file) setenv("MRP_MOCK_TA_CALLS", keep.c_str(), 1);
  return rc;
}

// a wide problem in the matrix form (`cost` owns the rows of a gather-form one), as mock_ll_ta.cpp's asMatrix
mrp_ll_assign_problem_w asMatrixWide(const mrp_ll_ctx* c, const mrp_ll_assign_problem_w& p, std::vector<int32_t>& cost) {
  if (p.cost) return p;
  const std::vector<TaTable>& tabs = tablesOf(c);
  cost.assign(static_cast<size_t>(p.n_agents) * p.n_tasks + 1, 0);
  for (int t = 0; t < p.n_tasks; ++t) {
    const TaTable& tab = tabs[p.heuristic_ids[t]];
    const int dimx = c->maps[tab.mapId].dimx;
    for (int a = 0; a < p.n_agents; ++a) {
      const int d = tab.dist[p.starts_xy[2 * a] + dimx * p.starts_xy[2 * a + 1]];
      const bool ok = !p.allowed || ((p.allowed[static_cast<size_t>(a) * p.mask_words + t / 64] >> (t % 64)) & 1);
      cost[static_cast<size_t>(a) * p.n_tasks + t] = (!ok || d == INT_MAX || d > 0xFFFE) ? MRP_LL_ASSIGN_NO_EDGE : d;
    }
  }
  mrp_ll_assign_problem_w q = p;
  q.cost = cost.data();
  q.heuristic_ids = nullptr;
  q.starts_xy = nullptr;
  q.allowed = nullptr;
  return q;
}

}  // namespace

extern "C" {

int mrp_ll_assign_series_create_w(mrp_ll_ctx* c, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_series** out) {
  taCall("assign_series_create_w");
  std::vector<std::vector<int32_t>> rows(static_cast<size_t>(n));
  std::vector<mrp_ll_assign_problem_w> ps;
  for (int k = 0; k < n; ++k) ps.push_back(asMatrixWide(c, problems[k], rows[k]));
  return mock_ta_series_create_w(c, n, ps.data(), out);
}
int mrp_ll_assign_series_next(mrp_ll_ctx*, int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results) {
  taCall("assign_series_next");
  return mock_ta_series_next_mixed(n, series, results);
}
#ifndef MOCK_NO_WIDE_ROOT
int mrp_ll_ta_root_batch_w(mrp_ll_ctx* c, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts) {
  taCall("ta_root_batch_w");
  for (int r = 0; r < nRoots; ++r)
    if (roots[r].n_agents <= 64) taCall("narrow_root_in_wide_call");  // (the drivers send those through the narrow call)
  return quietly([&] { return mrp_ll_ta_root_batch(c, nRoots, roots, planned, conflicts); });
}
#endif

}  // extern "C"
