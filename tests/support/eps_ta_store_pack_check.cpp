// TEST INFRASTRUCTURE — a stand-alone check of the path-store form of MRP_LL_ASTAR_EPS_TA in the host packers
// (libmultirobotplanning_amd/csrc/host/ll_pack.h packJob, ta_eps_root_pack.h), built by tests/test_eps_ta_store_pack_cpu.py
// with the host sanitizers and run as a program of its own: the descriptor of a job that names its context by slots and
// stores its result, the jobs the packer refuses (nothing pushed), and the root packer with and without slot ids.
// Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/ta_eps_root_pack.h"

using namespace mrp::host;
using mrp::DevJob;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      std::fprintf(stderr, "eps_ta_store_pack_check: line %d: %s\n", __LINE__, #cond);     \
      std::exit(1);                                                                        \
    }                                                                                      \
  } while (0)

namespace {

PackEnv makeEnv() {  // map 0: 8 x 8 at word 0; tables 0 and 1 of map 0; a path store of 40 slots
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{8, 8, 2, 0});
  env.heurs.push_back(HeurRec{0, 128});
  env.heurs.push_back(HeurRec{0, 640});
  env.maxHorizon = 64;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 4096;
  env.pathStoreSlots = 40;
  return env;
}

struct Sink {
  std::vector<uint32_t> w;
  bool failed = false;
  size_t size() const { return 1000 + w.size(); }  // (the batch's words in front of this job's)
  bool fits(size_t) const { return true; }
  void push(uint32_t v) { w.push_back(v); }
  uint32_t* grow(size_t n) { w.resize(w.size() + n); return w.data() + w.size() - n; }
};
struct PSink {
  size_t asked = 0;
  std::vector<uint16_t> tab;
  bool failed = false;
  uint16_t* alloc(size_t n, uint32_t& off) { asked += 1; off = 48; tab.assign(n, 0x1234); return tab.data(); }
};

struct Job {
  std::vector<int32_t> len, ids;
  mrp_ll_job j;
  Job(int n, int agent) : len(n, 0), ids(n, -1) {
    std::memset(&j, 0, sizeof(j));
    j.map_id = 0; j.algo = MRP_LL_ASTAR_EPS_TA; j.w = 1.5f; j.agent_idx = agent;
    j.start_x = 1; j.start_y = 2; j.goal_x = 6; j.goal_y = 5;
    j.heuristic_id = 1;
    j.max_expansions = 777;
    j.n_agents = n; j.path_len = len.data(); j.path_ids = ids.data(); j.path_xy = nullptr;
    j.result_path_id = -1;
  }
  Job(const Job& o) : len(o.len), ids(o.ids), j(o.j) {
    j.path_len = len.data(); j.path_ids = ids.data();
  }
};

bool pack(const PackEnv& env, const mrp_ll_job& j, Sink& cs, PSink& ps, DevJob& d) {
  PendingSet pend;
  return packJob(env, j, PackArgs{}, cs, ps, d, pend);
}
// refused, and nothing left behind
void refused(const PackEnv& env, const mrp_ll_job& j, int line) {
  Sink cs;
  PSink ps;
  DevJob d;
  if (pack(env, j, cs, ps, d) || !cs.w.empty() || ps.asked != 0) {
    std::fprintf(stderr, "eps_ta_store_pack_check: line %d: job not refused cleanly\n", line);
    std::exit(1);
  }
}
#define REFUSED(env, j) refused(env, j, __LINE__)

void byIdDescriptor(const PackEnv& env) {
  // 19 agents, agent 7 searches; agent 3 has an empty path and a (deliberately wild) id, agent 18 the longest path
  Job b(19, 7);
  for (int a = 0; a < 19; ++a) {
    b.len[a] = 2 + a % 5;
    b.ids[a] = 39 - a;
  }
  b.len[3] = 0; b.ids[3] = 12345;
  b.len[7] = 60; b.ids[7] = 5;  // the searching agent's own entry is never looked at
  b.len[18] = 13;
  const int32_t vc[2][3] = {{3, 1, 1}, {4, 6, 5}};
  const int32_t ec[1][5] = {{2, 1, 1, 2, 1}};
  b.j.n_vertex_constraints = 2; b.j.vertex_constraints = &vc[0][0];
  b.j.n_edge_constraints = 1; b.j.edge_constraints = &ec[0][0];
  b.j.flags = MRP_LL_JOB_STORE_RESULT;
  b.j.result_path_id = 17;
  Sink cs;
  PSink ps;
  DevJob d;
  CHECK(pack(env, b.j, cs, ps, d));
  CHECK(ps.asked == 0);  // no table shipped
  CHECK(d.algo == MRP_LL_ASTAR_EPS_TA && d.w == 1.5f && d.max_expansions == 777);
  CHECK((d.ctx_flags & mrp::kCtxById) != 0 && (d.ctx_flags & (mrp::kCtxScan | mrp::kCtxHeavy | mrp::kCtxChain | mrp::kTaNoGoal)) == 0);
  CHECK(d.n_ctx == 19 && d.n_agents_pad == 32 && d.t_pad == 13);
  CHECK(d.heur_off == 640);  // both tables: the heuristic's offset beside the id list's
  CHECK(d.store_out_id == 17);
  CHECK(d.n_vc == 2 && d.n_ec == 1 && d.vc_off == 1000 && d.ec_off == 1002 && d.last_goal_constraint == 4);
  CHECK(d.path_off == 1003 && cs.w.size() == 3 + 19);
  for (int a = 0; a < 19; ++a)
    CHECK(cs.w[3 + a] == ((a == 7 || a == 3) ? mrp::kNoStoreSlot : static_cast<uint32_t>(39 - a)));
  CHECK(d.pad_[0] == 0 && d.pad_[1] == 0 && d.pad_[2] == 0 && d.reserved == 0);

  // the same job shipped: the same descriptor but for the context's form
  std::vector<std::vector<int32_t>> cells(19);
  std::vector<const int32_t*> xy(19);
  for (int a = 0; a < 19; ++a) {
    cells[a].assign(2 * static_cast<size_t>(b.len[a]) + 2, 1);
    xy[a] = cells[a].data();
  }
  mrp_ll_job s = b.j;
  s.path_ids = nullptr; s.path_xy = xy.data();
  Sink cs2;
  PSink ps2;
  DevJob o;
  CHECK(pack(env, s, cs2, ps2, o));
  CHECK(ps2.asked == 1 && ps2.tab.size() == 13u * 32u && o.path_off == 48 && o.n_ctx == 0 && !(o.ctx_flags & mrp::kCtxById));
  o.path_off = d.path_off; o.n_ctx = d.n_ctx; o.ctx_flags = d.ctx_flags;
  CHECK(std::memcmp(&o, &d, sizeof(DevJob)) == 0);

  // a context without any path: no table, no ids, no flag; an agent without a task keeps its flag beside kCtxById
  Job e(4, 1);
  Sink cs3;
  PSink ps3;
  CHECK(pack(env, e.j, cs3, ps3, d));
  CHECK(!(d.ctx_flags & mrp::kCtxById) && d.t_pad == 0 && d.n_agents_pad == 0 && cs3.w.empty() && d.store_out_id == mrp::kNoStoreSlot);
  Job g(2, 0);
  g.len[1] = 9; g.ids[1] = 0;
  g.j.flags = MRP_LL_JOB_NO_GOAL; g.j.heuristic_id = -1;
  Sink cs4;
  PSink ps4;
  CHECK(pack(env, g.j, cs4, ps4, d));
  CHECK(d.ctx_flags == (mrp::kCtxById | mrp::kTaNoGoal) && d.t_pad == 9 && d.n_agents_pad == 16 && d.heur_off == 0 && cs4.w.size() == 2);
}

void refusals(const PackEnv& env) {
  auto base = [] {
    Job b(3, 1);
    b.len[0] = 4; b.ids[0] = 2;
    b.len[2] = 6; b.ids[2] = 39;
    return b;
  };
  {  // the job itself is fine
    Job b = base();
    Sink cs;
    PSink ps;
    DevJob d;
    CHECK(pack(env, b.j, cs, ps, d) && d.t_pad == 6);
  }
  { Job b = base(); b.ids[2] = 40; REFUSED(env, b.j); }                           // id outside the store
  { Job b = base(); b.ids[0] = -1; REFUSED(env, b.j); }                           // a path without a slot
  { Job b = base(); b.len[2] = 65; REFUSED(env, b.j); }                           // t_pad beyond max_horizon
  { Job b = base(); b.j.path_len = nullptr; REFUSED(env, b.j); }
  { Job b = base(); b.j.flags = MRP_LL_JOB_STORE_RESULT; b.j.result_path_id = 40; REFUSED(env, b.j); }
  { Job b = base(); b.j.flags = MRP_LL_JOB_STORE_RESULT; b.j.result_path_id = -1; REFUSED(env, b.j); }
  { Job b = base(); b.j.initial_cost = 1; REFUSED(env, b.j); }
  { Job b = base(); b.j.flags = MRP_LL_JOB_ROOT_CHAIN; REFUSED(env, b.j); }
  { Job b = base(); b.j.flags = MRP_LL_JOB_HEAVY; REFUSED(env, b.j); }
  { Job b = base(); b.j.flags = MRP_LL_JOB_SCAN_CONFLICTS; REFUSED(env, b.j); }
  {  // ... also where the call would hand conflicts back
    Job b = base();
    b.j.flags = MRP_LL_JOB_SCAN_CONFLICTS;
    Sink cs;
    PSink ps;
    DevJob d;
    PendingSet pend;
    PackArgs args;
    args.scanAllowed = true;
    CHECK(!packJob(env, b.j, args, cs, ps, d, pend) && cs.w.empty());
  }
  {  // a constraint set
    Job b = base();
    b.j.flags = MRP_LL_JOB_CONSTRAINT_SET;
    PackEnv e2 = env;
    e2.consStoreSlots = 4; e2.consStoreStride = 64; e2.consSets.resize(4);
    mrp_ll_constraint_ref ref;
    ref.base_set_id = -1; ref.result_set_id = 1;
    Sink cs;
    PSink ps;
    DevJob d;
    PendingSet pend;
    PackArgs args;
    args.ref = &ref;
    CHECK(!packJob(e2, b.j, args, cs, ps, d, pend) && cs.w.empty());
  }
  {  // the table does not fit the arena slot's path area: 4096 bytes hold 64 rows of 32 agents, not of 48
    Job b(33, 0);
    for (int a = 1; a < 33; ++a) { b.len[a] = 3; b.ids[a] = a; }
    b.len[32] = 43;  // 43 x 48 x 2 = 4128
    REFUSED(env, b.j);
    b.len[32] = 42;  // 4032
    Sink cs;
    PSink ps;
    DevJob d;
    CHECK(pack(env, b.j, cs, ps, d) && d.t_pad == 42 && d.n_agents_pad == 48);
  }
  {  // no store reserved: neither form
    PackEnv e2 = env;
    e2.pathStoreSlots = 0;
    Job b = base();
    REFUSED(e2, b.j);
    Job c(1, 0);
    c.j.path_ids = nullptr; c.j.n_agents = 0;
    c.j.flags = MRP_LL_JOB_STORE_RESULT; c.j.result_path_id = 0;
    REFUSED(e2, c.j);
  }
}

struct Root {
  std::vector<int32_t> starts, goals, hids;
  std::vector<mrp_ll_result> results;
  mrp_ll_ta_root r;
  Root(int map, int n) : starts(2 * n), goals(2 * n), hids(n), results(n) {
    for (int a = 0; a < n; ++a) {
      starts[2 * a] = a % 8; starts[2 * a + 1] = a / 8;
      goals[2 * a] = 7 - a % 8; goals[2 * a + 1] = 7 - a / 8;
      hids[a] = a % 3 == 2 ? -1 : a % 2;
      std::memset(&results[a], 0, sizeof(mrp_ll_result));
    }
    r.map_id = map; r.n_agents = n;
    r.starts_xy = starts.data(); r.goals_xy = goals.data(); r.heuristic_ids = hids.data();
    r.max_expansions = 1000 + n;
    r.results = results.data();
  }
};

void rootsWithIds(const PackEnv& env) {
  Root r3(0, 3), r17(0, 17), r2(0, 2), r5(0, 5);
  const mrp_ll_ta_root roots[4] = {r3.r, r17.r, r2.r, r5.r};
  TaRootStaging plain;
  packTaEpsRoots(env, 1.5f, 4, roots, 100, plain);
  CHECK(plain.recs.size() == 4 && plain.slotWords.empty());
  for (const DevJob& d : plain.recs) CHECK(d.ec_off == d.vc_off && d.store_out_id == mrp::kNoStoreSlot);
  TaRootStaging plain2;  // NULL and "no root has ids" are one thing
  const int32_t* none[4] = {nullptr, nullptr, nullptr, nullptr};
  packTaEpsRoots(env, 1.5f, 4, roots, 100, plain2, none);
  CHECK(plain2.slotWords.empty() && plain2.words == plain.words && plain2.recs.size() == 4);
  for (size_t q = 0; q < 4; ++q) CHECK(std::memcmp(&plain2.recs[q], &plain.recs[q], sizeof(DevJob)) == 0);

  // roots 0 and 1 store (agent 1 of root 0 and the odd agents of root 1 do not), root 2 has no ids, root 3 a bad one
  std::vector<int32_t> i3 = {4, -1, 39}, i17(17), i5 = {0, 1, 2, 40, 3};
  for (int a = 0; a < 17; ++a) i17[a] = a % 2 ? -1 : a;
  const int32_t* ids[4] = {i3.data(), i17.data(), nullptr, i5.data()};
  TaRootStaging st;
  packTaEpsRoots(env, 1.5f, 4, roots, 100, st, ids);
  CHECK(st.recs.size() == 3 && st.devRootOf[0] == 0 && st.devRootOf[1] == 1 && st.devRootOf[2] == 2 && st.devRootOf[3] == -1);
  CHECK(st.nResults == 3 + 17 + 2);
  CHECK(st.words.size() == mrp::kTaRootAgentWords * (3 + 17 + 2) && st.slotWords.size() == 3 + 17);
  // the agent words and the records are today's, word for word, apart from where the slot run stands
  CHECK(std::equal(st.words.begin(), st.words.end(), plain.words.begin()));
  const uint32_t runBase = 100 + static_cast<uint32_t>(st.words.size());
  CHECK(st.recs[0].ec_off == runBase && st.recs[1].ec_off == runBase + 3 && st.recs[2].ec_off == st.recs[2].vc_off);
  for (size_t q = 0; q < 3; ++q) {
    DevJob d = st.recs[q];
    d.ec_off = plain.recs[q].ec_off;
    CHECK(std::memcmp(&d, &plain.recs[q], sizeof(DevJob)) == 0);
  }
  CHECK(st.slotWords[0] == 4 && st.slotWords[1] == mrp::kNoStoreSlot && st.slotWords[2] == 39);
  for (int a = 0; a < 17; ++a) CHECK(st.slotWords[3 + a] == (a % 2 ? mrp::kNoStoreSlot : static_cast<uint32_t>(a)));
  // the per-agent descriptor does not change with the slots
  for (int a = 0; a < 3; ++a) {
    DevJob x = st.recs[0], y = plain.recs[0];
    const uint32_t* w = st.words.data() + mrp::kTaRootAgentWords * a;
    mrp::taEpsRootAgentJob(x, w[0], w[1], w[2], 50, a ? 16u : 0u, a ? 7u : 0u);
    mrp::taEpsRootAgentJob(y, w[0], w[1], w[2], 50, a ? 16u : 0u, a ? 7u : 0u);
    x.ec_off = y.ec_off;
    CHECK(std::memcmp(&x, &y, sizeof(DevJob)) == 0);
  }
  // what the caller holds of a refused root: MRP_LL_BAD_JOB; ids below -1 and ids without a store refuse too
  int32_t planned[4];
  mrp_ll_conflict c[4];
  blankTaRootOutputs(env, 4, roots, planned, c, ids);
  CHECK(r5.results[0].status == MRP_LL_BAD_JOB && r5.results[4].status == MRP_LL_BAD_JOB && r3.results[0].status == MRP_LL_NOT_RUN &&
        r2.results[1].status == MRP_LL_NOT_RUN && planned[3] == 0 && c[3].found == -1);
  i5[3] = -2;
  CHECK(!taRootValid(env, r5.r, i5.data()));
  i5[3] = -1;
  CHECK(taRootValid(env, r5.r, i5.data()));
  PackEnv e2 = env;
  e2.pathStoreSlots = 0;
  CHECK(!taRootValid(e2, r5.r, i5.data()) && taRootValid(e2, r5.r, nullptr));
}

}  // namespace

int main() {
  const PackEnv env = makeEnv();
  byIdDescriptor(env);
  refusals(env);
  rootsWithIds(env);
  std::printf("eps_ta_store_pack_check: ok\n");
  return 0;
}
