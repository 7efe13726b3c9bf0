// TEST INFRASTRUCTURE — a stand-alone check of the packer and unpacker of mrp_ll_ta_eps_root_batch
// (libmultirobotplanning_amd/csrc/host/ta_eps_root_pack.h), built by tests/test_ta_eps_root_pack_cpu.py with the host
// sanitizers and run as a program of its own: the root's record (algo, weight, word offsets), the per-agent descriptor the
// workgroup makes (ll_device.h taEpsRootAgentJob) against packJob's for the ordinary MRP_LL_ASTAR_EPS_TA job with the paths
// before it as its shipped context, and the way back — a root the kernel left unfinished because its table did not fit, a
// root it finished without a scan, a root that ended behind an agent, a refused root.  Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/ta_eps_root_pack.h"

using namespace mrp::host;
using mrp::DevJob;
using mrp::DevResult;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      std::fprintf(stderr, "ta_eps_root_pack_check: line %d: %s\n", __LINE__, #cond);      \
      std::exit(1);                                                                        \
    }                                                                                      \
  } while (0)

namespace {

PackEnv makeEnv() {  // map 0: 8 x 8 at word 0; tables 0 and 1 of map 0
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{8, 8, 2, 0});
  env.heurs.push_back(HeurRec{0, 128});
  env.heurs.push_back(HeurRec{0, 640});
  env.maxHorizon = 64;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 128 * 1024;
  return env;
}

struct Root {
  std::vector<int32_t> starts, goals, hids;
  std::vector<mrp_ll_result> results;
  std::vector<std::vector<int32_t>> states, actions, costs;
  mrp_ll_ta_root r;
  Root(int map, int n, int cap = 8) : starts(2 * n), goals(2 * n), hids(n), results(n), states(n), actions(n), costs(n) {
    for (int a = 0; a < n; ++a) {
      starts[2 * a] = a % 8; starts[2 * a + 1] = a / 8;
      goals[2 * a] = 7 - a % 8; goals[2 * a + 1] = 7 - a / 8;
      hids[a] = a % 3 == 2 ? -1 : a % 2;
      states[a].assign(3 * cap, -1); actions[a].assign(cap, -1); costs[a].assign(cap, -1);
      std::memset(&results[a], 0x5A, sizeof(mrp_ll_result));
      results[a].states_txy = states[a].data(); results[a].actions = actions[a].data(); results[a].action_costs = costs[a].data();
      results[a].states_cap = cap;
      results[a].chain_results = nullptr;
    }
    r.map_id = map; r.n_agents = n;
    r.starts_xy = starts.data(); r.goals_xy = goals.data(); r.heuristic_ids = hids.data();
    r.max_expansions = 1000 + n;
    r.results = results.data();
  }
};

// The descriptor runTaEpsRoot makes for agent a, with agents 0 .. a - 1 planned with paths of lens[q] states, against packJob's
// for the ordinary job that ships those paths: all 112 bytes but path_off (the workgroup's table is not shipped).
void sameAsOrdinaryJob(const PackEnv& env, float w, const mrp_ll_ta_root& r, const DevJob& rec, const uint32_t* words, int a,
                       const std::vector<int32_t>& lens, int64_t budget) {
  const uint32_t npad = (static_cast<uint32_t>(r.n_agents) + 15u) & ~15u;
  uint32_t maxLen = 0;
  for (int q = 0; q < a; ++q) maxLen = std::max<uint32_t>(maxLen, static_cast<uint32_t>(lens[q]));
  DevJob d = rec;
  mrp::taEpsRootAgentJob(d, words[3 * a], words[3 * a + 1], words[3 * a + 2], budget, a ? npad : 0u, a ? maxLen : 0u);
  std::vector<std::vector<int32_t>> cells(r.n_agents);
  std::vector<int32_t> len(r.n_agents, 0);
  std::vector<const int32_t*> xy(r.n_agents, nullptr);
  for (int q = 0; q < r.n_agents; ++q) {
    if (q < a) {
      len[q] = lens[q];
      for (int t = 0; t < lens[q]; ++t) cells[q].insert(cells[q].end(), {(q + t) % 8, q % 8});
    }
    cells[q].push_back(0);
    xy[q] = cells[q].data();
  }
  mrp_ll_job j;
  std::memset(&j, 0, sizeof(j));
  j.map_id = r.map_id; j.algo = MRP_LL_ASTAR_EPS_TA; j.w = w; j.agent_idx = a;
  j.start_x = r.starts_xy[2 * a]; j.start_y = r.starts_xy[2 * a + 1];
  j.goal_x = r.goals_xy[2 * a]; j.goal_y = r.goals_xy[2 * a + 1];
  j.heuristic_id = r.heuristic_ids[a];
  j.flags = r.heuristic_ids[a] < 0 ? MRP_LL_JOB_NO_GOAL : 0;
  j.max_expansions = budget;
  j.n_agents = r.n_agents; j.path_len = len.data(); j.path_xy = xy.data();
  struct Sink {
    std::vector<uint32_t> w; bool failed = false;
    size_t size() const { return w.size(); }
    bool fits(size_t) const { return true; }
    void push(uint32_t v) { w.push_back(v); }
    uint32_t* grow(size_t n) { w.resize(w.size() + n); return w.data() + w.size() - n; }
  } cs;
  struct PSink {
    std::vector<uint16_t> tab; bool failed = false;
    uint16_t* alloc(size_t n, uint32_t& off) { off = 48; tab.assign(n, 0x1234); return tab.data(); }
  } ps;
  DevJob o;
  PendingSet pend;
  CHECK(packJob(env, j, PackArgs{}, cs, ps, o, pend));
  CHECK(a == 0 ? ps.tab.empty() : (o.path_off == 48 && ps.tab.size() == static_cast<size_t>(maxLen) * npad));
  o.vc_off = d.vc_off; o.ec_off = d.ec_off;  // (where the empty constraint lists stand is the batch's)
  o.path_off = d.path_off;                   // (the table is in the slot, not in the batch's path buffer)
  CHECK(d.path_off == 0 && d.n_ctx == 0 && d.reserved == 0);
  CHECK(std::memcmp(&o, &d, sizeof(DevJob)) == 0);
  // the ordinary job's table, for reference: the own column and the columns not yet planned are empty in every row
  for (uint32_t t = 0; a && t < maxLen; ++t)
    for (uint32_t q = static_cast<uint32_t>(a); q < npad; ++q) CHECK(ps.tab[t * npad + q] == mrp::kEmptyCell);
}

void packAndUnpack(const PackEnv& env) {
  Root r0(0, 3), bad(0, 3), r17(0, 17), r2(0, 2), r64(0, 64);
  bad.r.map_id = 7;
  const mrp_ll_ta_root roots[5] = {r0.r, bad.r, r17.r, r2.r, r64.r};
  const float w = 1.5f;
  TaRootStaging st;
  packTaEpsRoots(env, w, 5, roots, 100, st);
  CHECK(st.recs.size() == 4 && st.nResults == 3 + 17 + 2 + 64);
  CHECK(st.devRootOf[0] == 0 && st.devRootOf[1] == -1 && st.devRootOf[2] == 1 && st.devRootOf[3] == 2 && st.devRootOf[4] == 3);
  CHECK(st.firstResult[0] == 0 && st.firstResult[2] == 3 && st.firstResult[3] == 20 && st.firstResult[4] == 22);
  CHECK(st.words.size() == mrp::kTaRootAgentWords * (3 + 17 + 2 + 64));
  for (const DevJob& d : st.recs) CHECK(d.algo == MRP_LL_ASTAR_EPS_TA && d.w == w && d.last_goal_constraint == -1 && d.n_vc == 0 && d.n_ec == 0);
  CHECK(st.recs[0].vc_off == 100 && st.recs[1].vc_off == 109 && st.recs[1].n_ctx == 17 && st.recs[1].reserved == 3);
  CHECK(st.words[1] == 128 && st.words[4] == 640 && st.words[7] == 0 && st.words[8] == mrp::kTaNoGoal);
  std::vector<int32_t> lens;
  for (int a = 0; a < 64; ++a) lens.push_back(1 + (a * 7) % 11);
  for (int a = 0; a < 3; ++a) sameAsOrdinaryJob(env, w, roots[0], st.recs[0], st.words.data(), a, lens, 500 - a);
  for (int a = 0; a < 17; ++a) sameAsOrdinaryJob(env, w, roots[2], st.recs[1], st.words.data() + 9, a, lens, -1);
  for (int a = 0; a < 64; a += 9) sameAsOrdinaryJob(env, w, roots[4], st.recs[3], st.words.data() + 9 + 51 + 6, a, lens, 0);

  // ---- the way back: exactly the launch's buffers (the sanitizer watches their ends)
  const uint32_t outStride = 64 + mrp::kScanOutHalfs;
  std::vector<DevResult> dres(st.nResults);
  std::vector<uint16_t> out(static_cast<size_t>(st.nResults) * outStride, 0xEEEE);
  std::memset(dres.data(), 0, dres.size() * sizeof(DevResult));
  blankTaRootAnswers(st, out.data(), outStride);
  auto answer = [&](uint32_t first) { return const_cast<uint32_t*>(taRootAnswer(out.data(), outStride, first)); };
  auto path = [&](uint32_t ri, std::vector<uint16_t> cells) {
    dres[ri].status = mrp::ST_OK; dres[ri].n_states = static_cast<int32_t>(cells.size());
    dres[ri].cost = static_cast<int32_t>(cells.size()) - 1; dres[ri].fmin = dres[ri].cost; dres[ri].expanded = 10 + ri; dres[ri].tier = 1;
    std::memcpy(out.data() + static_cast<size_t>(ri) * outStride, cells.data(), cells.size() * 2);
  };
  // root 0 ends behind agent 1 (budget); agent 2 is not run
  path(0, {0, 1, 2});
  dres[1].status = mrp::ST_CAP_EXP; dres[1].expanded = 77; dres[1].tier = 1;
  answer(0)[mrp::kTaRootPlannedWord] = 2;
  // root 2 (17 agents): the table did not fit behind agent 4: five planned, the rest is the host's
  for (uint32_t a = 0; a < 5; ++a) path(3 + a, {static_cast<uint16_t>(a), static_cast<uint16_t>(a + 1)});
  answer(3)[0] = mrp::kTaRootScanSkipped;
  answer(3)[mrp::kTaRootPlannedWord] = 5;
  // root 3: both planned, the scan left to the host
  path(20, {0, 1});
  path(21, {5});
  answer(20)[0] = mrp::kTaRootScanSkipped;
  answer(20)[mrp::kTaRootPlannedWord] = 2;
  // root 4 (64 agents): all planned, scanned on the device: count 3
  for (uint32_t a = 0; a < 64; ++a) path(22 + a, {static_cast<uint16_t>(a)});
  const uint32_t conf[10] = {1, 0, 2, 9, 0, 4, 6, 0, 0, 3};
  std::memcpy(answer(22), conf, sizeof(conf));
  answer(22)[mrp::kTaRootPlannedWord] = 64;

  int32_t planned[5] = {-9, -9, -9, -9, -9};
  mrp_ll_conflict c[5];
  std::memset(c, 0x33, sizeof(c));
  mrp_ll_stats stats;
  std::memset(&stats, 0, sizeof(stats));
  std::vector<int32_t> needScan, needRest;
  unpackTaEpsRoots(stats, st, 5, roots, dres.data(), out.data(), outStride, planned, c, needScan, needRest);
  CHECK(planned[0] == 2 && planned[1] == 0 && planned[2] == 5 && planned[3] == 2 && planned[4] == 64);
  CHECK(needScan.size() == 1 && needScan[0] == 3);
  CHECK(needRest.size() == 1 && needRest[0] == 2);
  const mrp_ll_conflict none = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) CHECK(std::memcmp(&c[k], &none, sizeof(none)) == 0);
  CHECK(std::memcmp(&c[4], conf, sizeof(conf)) == 0 && c[4].count == 3);
  CHECK(r0.results[0].status == MRP_LL_OK && r0.results[0].fmin == 2 && r0.results[1].status == MRP_LL_CAP_EXPANSIONS &&
        r0.results[1].expanded == 77 && r0.results[2].status == MRP_LL_NOT_RUN);
  CHECK(r17.results[4].status == MRP_LL_OK && r17.results[4].n_states == 2 && r17.results[5].status == MRP_LL_NOT_RUN &&
        r17.results[16].status == MRP_LL_NOT_RUN && r17.results[16].expanded == 0);
  for (int a = 0; a < 3; ++a) CHECK(bad.results[a].status == MRP_LL_BAD_JOB && bad.results[a].n_states == 0);
  // a root that stopped early because an agent FAILED is nobody's to finish, whatever its answer word says
  dres[5].status = mrp::ST_NO_SOLUTION;
  unpackTaEpsRoots(stats, st, 5, roots, dres.data(), out.data(), outStride, planned, c, needScan, needRest);
  CHECK(needRest.empty() && planned[2] == 5);
  // every root refused: no launch, no device results
  const mrp_ll_ta_root refused[1] = {bad.r};
  TaRootStaging none1;
  packTaEpsRoots(env, w, 1, refused, 0, none1);
  CHECK(none1.recs.empty() && none1.nResults == 0);
  unpackTaEpsRoots(stats, none1, 1, refused, nullptr, nullptr, outStride, planned, c, needScan, needRest);
  CHECK(planned[0] == 0 && needScan.empty() && needRest.empty() && bad.results[0].status == MRP_LL_BAD_JOB);
}

}  // namespace

int main() {
  const PackEnv env = makeEnv();
  packAndUnpack(env);
  std::printf("ta_eps_root_pack_check: ok\n");
  return 0;
}
