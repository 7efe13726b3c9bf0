// One conflict tree, stepped by the caller (include/mrp_hl.h "mrp_hl_ct_*"): the caller sees the pending low-level
// requests, runs them wherever it likes and delivers the results; mrp_hl_ct_round_mine / mrp_hl_ct_deliver_rows do that for
// ranks that share one tree's rounds and exchange fixed-size rows (ct_sharded.py).  Included by mrp_hl.cpp only.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "ct_session.hpp"

struct mrp_hl_ct {
  std::unique_ptr<mrp_hl::Instance> inst;
  std::vector<mrp_hl::LLRequest> req;
  mrp_hl::JobBatch batch;
  void rebuild() {  // job views of the pending requests; arrays stay valid until the next deliver
    batch.clear();
    for (const mrp_hl::LLRequest& r : req) batch.add(*inst, r);
    batch.patch();
  }
};

namespace mrp_hl {

// A search result as one row of kRowHdr + maxStates words, the unit the ranks exchange:
//   group, slot, status, cost, fmin, expanded (low 31 bits), expanded (the rest), n_states, then a word x | y << 16 per state
// (state k is at time k).  A rank whose round failed sends ONE row whose group word is kFailedRound, its return code in the
// status word.
constexpr int32_t kRowHdr = 8;
constexpr int32_t kFailedRound = INT32_MIN;  // (group ids are >= -1: -1 is the root step)
inline int32_t rowGroup(const int32_t* w) { return w[0]; }
inline int32_t rowSlot(const int32_t* w) { return w[1]; }
inline void encodeRow(int32_t* w, int32_t group, int32_t slot, const mrp_ll_result& r) {
  w[0] = group;
  w[1] = slot;
  w[2] = r.status;
  w[3] = r.cost;
  w[4] = r.fmin;
  w[5] = static_cast<int32_t>(r.expanded & 0x7FFFFFFF);
  w[6] = static_cast<int32_t>(r.expanded >> 31);
  w[7] = r.n_states;
  for (int32_t k = 0; k < r.n_states; ++k) w[kRowHdr + k] = r.states_txy[3 * k + 1] | (r.states_txy[3 * k + 2] << 16);
}
inline void encodeFailedRow(int32_t* w, size_t rowWords, int rc) {
  std::memset(w, 0, rowWords * sizeof(int32_t));
  w[0] = kFailedRound;
  w[2] = rc;
}
// into a result bound to maxStates states (bindResults); false: the row's state count does not fit
inline bool decodeRow(const int32_t* w, int32_t maxStates, mrp_ll_result& r) {
  r.status = w[2];
  r.cost = w[3];
  r.fmin = w[4];
  r.expanded = static_cast<int64_t>(w[5]) | (static_cast<int64_t>(w[6]) << 31);
  r.n_states = w[7];
  if (r.n_states < 0 || r.n_states > maxStates) return false;
  for (int32_t k = 0; k < r.n_states; ++k) {
    r.states_txy[3 * k] = k;
    r.states_txy[3 * k + 1] = w[kRowHdr + k] & 0xFFFF;
    r.states_txy[3 * k + 2] = w[kRowHdr + k] >> 16;
  }
  return true;
}

// the pending groups in order, and which rank searches which (group j -> rank j % world)
inline void roundOwners(const mrp_hl_ct& c, int32_t world, std::vector<int32_t>& groups, std::vector<int32_t>& ownerOfReq) {
  groups.clear();
  ownerOfReq.assign(c.req.size(), 0);
  for (size_t k = 0; k < c.req.size(); ++k) {
    if (groups.empty() || groups.back() != c.req[k].group) groups.push_back(c.req[k].group);
    ownerOfReq[k] = static_cast<int32_t>((groups.size() - 1) % static_cast<size_t>(world));
  }
}

}  // namespace mrp_hl

extern "C" {

int mrp_hl_ct_create(const mrp_hl_instance* in, const mrp_hl_options* opt, int32_t mapId, int32_t specWidth,
                     mrp_hl_ct** out) {
  if (!in || !opt || !out || in->n_agents < 0) return MRP_LL_E_INVALID;
  auto* c = new mrp_hl_ct();
  c->inst.reset(new mrp_hl::Instance(*in, mapId, *opt));
  c->inst->setSpecWidth(specWidth);
  c->inst->start(c->req);
  if (c->inst->done()) c->req.clear();
  c->rebuild();
  *out = c;
  return MRP_LL_SUCCESS;
}

void mrp_hl_ct_destroy(mrp_hl_ct* c) { delete c; }

int32_t mrp_hl_ct_n_requests(const mrp_hl_ct* c) { return c ? static_cast<int32_t>(c->req.size()) : 0; }

int mrp_hl_ct_request(const mrp_hl_ct* c, int32_t k, mrp_ll_job* job, int32_t* group, int32_t* slot) {
  if (!c || k < 0 || k >= static_cast<int32_t>(c->req.size()) || !job) return MRP_LL_E_INVALID;
  *job = c->batch.jobs[k];
  if (group) *group = c->req[k].group;
  if (slot) *slot = c->req[k].slot;
  return MRP_LL_SUCCESS;
}

int mrp_hl_ct_deliver(mrp_hl_ct* c, int32_t group, int32_t n, const mrp_ll_result* results) {
  if (!c || n < 0 || (n > 0 && !results)) return MRP_LL_E_INVALID;
  // the group's requests are consecutive in the pending list: take them out, keep the others
  size_t a = 0;
  while (a < c->req.size() && c->req[a].group != group) ++a;
  size_t b = a;
  while (b < c->req.size() && c->req[b].group == group) ++b;
  if (a == c->req.size() || static_cast<int32_t>(b - a) != n) return MRP_LL_E_INVALID;
  std::vector<mrp_hl::LLAnswer> ans;
  for (int32_t k = 0; k < n; ++k) ans.push_back(mrp_hl::answerOf(results[k]));
  c->req.erase(c->req.begin() + static_cast<std::ptrdiff_t>(a), c->req.begin() + static_cast<std::ptrdiff_t>(b));
  c->inst->deliver(group, ans, c->req);
  if (c->inst->done()) c->req.clear();  // requests of a finished instance point into freed CT nodes
  c->rebuild();
  return MRP_LL_SUCCESS;
}

int32_t mrp_hl_ct_done(const mrp_hl_ct* c) { return c && c->inst->done() ? 1 : 0; }

int32_t mrp_hl_ct_round_mine(mrp_hl_ct* c, mrp_ll_ctx* ll, int32_t rank, int32_t world, int32_t maxStates, int32_t* rows,
                             int32_t capRows, int32_t* rowsPerRank) {
  using namespace mrp_hl;
  if (!c || !ll || !rows || !rowsPerRank || world < 1 || rank < 0 || rank >= world || maxStates < 1 || capRows < 1)
    return MRP_LL_E_INVALID;
  const size_t rowWords = static_cast<size_t>(kRowHdr) + static_cast<size_t>(maxStates);
  std::vector<int32_t> groups, owner;
  roundOwners(*c, world, groups, owner);
  for (int32_t r = 0; r < world; ++r) rowsPerRank[r] = 0;
  std::vector<size_t> mine;
  for (size_t k = 0; k < c->req.size(); ++k) {
    rowsPerRank[owner[k]] += 1;
    if (owner[k] == rank) mine.push_back(k);
  }
  auto fail = [&](int rc) {
    encodeFailedRow(rows, rowWords, rc);
    return rc;
  };
  if (static_cast<int32_t>(mine.size()) > capRows) return fail(MRP_LL_E_INVALID);
  std::vector<mrp_ll_job> jobs(mine.size());
  std::vector<mrp_ll_result> res(mine.size());
  std::vector<int32_t> states;
  bindResults(res.data(), res.size(), states, maxStates);
  for (size_t q = 0; q < mine.size(); ++q) jobs[q] = c->batch.jobs[mine[q]];
  if (!mine.empty()) {
    const int rc = mrp_ll_search_batch(ll, static_cast<int32_t>(jobs.size()), jobs.data(), res.data());
    if (rc != MRP_LL_SUCCESS) return fail(rc);
  }
  for (size_t q = 0; q < mine.size(); ++q) {
    const mrp_ll_result& r = res[q];
    if (r.status == MRP_LL_PATH_TRUNCATED || r.n_states > maxStates) return fail(MRP_LL_E_INVALID);  // max_states too small
    encodeRow(rows + q * rowWords, c->req[mine[q]].group, c->req[mine[q]].slot, r);
  }
  return static_cast<int32_t>(mine.size());
}

int mrp_hl_ct_deliver_rows(mrp_hl_ct* c, const int32_t* gathered, int32_t world, int32_t rowsStride, int32_t maxStates) {
  using namespace mrp_hl;
  if (!c || !gathered || world < 1 || rowsStride < 1 || maxStates < 1) return MRP_LL_E_INVALID;
  const size_t rowWords = static_cast<size_t>(kRowHdr) + static_cast<size_t>(maxStates);
  std::vector<int32_t> groups, owner;
  roundOwners(*c, world, groups, owner);
  std::vector<int32_t> perRank(world, 0);
  for (size_t k = 0; k < c->req.size(); ++k) perRank[owner[k]] += 1;
  // a rank that failed sent one row marked kFailedRound: every rank stops here, together
  for (int32_t r = 0; r < world; ++r)
    if (rowGroup(gathered + static_cast<size_t>(r) * rowsStride * rowWords) == kFailedRound) return MRP_LL_E_DEVICE;
  std::map<int32_t, std::vector<const int32_t*>> byGroup;
  for (int32_t r = 0; r < world; ++r) {
    if (perRank[r] > rowsStride) return MRP_LL_E_INVALID;
    for (int32_t q = 0; q < perRank[r]; ++q) {
      const int32_t* w = gathered + (static_cast<size_t>(r) * rowsStride + q) * rowWords;
      byGroup[rowGroup(w)].push_back(w);
    }
  }
  std::vector<int32_t> states;
  std::vector<mrp_ll_result> res;
  for (int32_t g : groups) {  // the same order on every rank
    auto it = byGroup.find(g);
    if (it == byGroup.end()) return MRP_LL_E_INVALID;
    std::vector<const int32_t*>& rws = it->second;
    std::sort(rws.begin(), rws.end(), [](const int32_t* a, const int32_t* b) { return rowSlot(a) < rowSlot(b); });
    res.assign(rws.size(), mrp_ll_result());
    bindResults(res.data(), res.size(), states, maxStates);
    for (size_t q = 0; q < rws.size(); ++q)
      if (!decodeRow(rws[q], maxStates, res[q])) return MRP_LL_E_INVALID;
    const int rc = mrp_hl_ct_deliver(c, g, static_cast<int32_t>(res.size()), res.data());
    if (rc != MRP_LL_SUCCESS) return rc;
    if (c->inst->done()) break;
  }
  return MRP_LL_SUCCESS;
}

int mrp_hl_ct_solution(const mrp_hl_ct* c, mrp_hl_solution* out) {
  if (!c || !out || !c->inst->done()) return MRP_LL_E_INVALID;
  mrp_hl::writeSolution(*c->inst, *out);
  return MRP_LL_SUCCESS;
}

}  // extern "C"
