// TEST INFRASTRUCTURE — a stand-alone check of the packer and unpacker of mrp_ll_ta_root_batch
// (libmultirobotplanning_amd/csrc/host/ta_root_pack.h), built by tests/test_ta_root_pack_cpu.py with the host sanitizers and run
// as a program of its own: every refusal include/mrp_ll.h lists, the record and the word offsets of accepted roots (a
// 64-agent one among them), the per-agent descriptor against packJob's for the ordinary job, and the way back — a root that
// ended behind an agent, a refused root, a scan the device left to the host.  Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/ta_root_pack.h"

using namespace mrp::host;
using mrp::DevJob;
using mrp::DevResult;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "ta_root_pack_check: line %d: %s\n", __LINE__, #cond);      \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

namespace {

PackEnv makeEnv() {  // map 0: 8 x 8 at word 0, map 1: 40 x 40 at word 32; tables 0 and 1 of map 0, table 2 of map 1
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{8, 8, 2, 0});
  env.maps.push_back(MapRec{40, 40, 50, 32});
  env.heurs.push_back(HeurRec{0, 128});
  env.heurs.push_back(HeurRec{0, 640});
  env.heurs.push_back(HeurRec{1, 1152});
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

void refusals(const PackEnv& env) {
  { Root a(0, 3); CHECK(taRootValid(env, a.r)); }
  { Root a(0, 64); CHECK(taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.map_id = 2; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.map_id = -1; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.starts[2] = 8; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.starts[5] = -1; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.hids[0] = 2; CHECK(!taRootValid(env, a.r)); }   // a table of another map
  { Root a(0, 3); a.hids[1] = 3; CHECK(!taRootValid(env, a.r)); }   // no such table
  { Root a(0, 3); a.goals[0] = 8; CHECK(!taRootValid(env, a.r)); }  // a task outside the grid (packJob refuses the ordinary job)
  { Root a(0, 3); a.goals[4] = 99; CHECK(taRootValid(env, a.r)); }  // ... ignored where the agent has no task
  { Root a(0, 3); a.r.n_agents = 0; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.n_agents = 65; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.n_agents = -4; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.starts_xy = nullptr; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.goals_xy = nullptr; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.heuristic_ids = nullptr; CHECK(!taRootValid(env, a.r)); }
  { Root a(0, 3); a.r.results = nullptr; CHECK(!taRootValid(env, a.r)); }
}

// The descriptor runTaRoot makes for agent a (ll_device.h taRootAgentJob, the function the kernel calls) against packJob's
// for the ordinary job: all 112 bytes.
void sameAsOrdinaryJob(const PackEnv& env, const mrp_ll_ta_root& r, const DevJob& rec, const uint32_t* words, int a, int64_t budget) {
  DevJob d = rec;
  mrp::taRootAgentJob(d, words[3 * a], words[3 * a + 1], words[3 * a + 2], budget);  // the workgroup's own function
  mrp_ll_job j;
  std::memset(&j, 0, sizeof(j));
  j.map_id = r.map_id; j.algo = MRP_LL_ASTAR_TA; j.w = 0.f;
  j.start_x = r.starts_xy[2 * a]; j.start_y = r.starts_xy[2 * a + 1];
  j.goal_x = r.goals_xy[2 * a]; j.goal_y = r.goals_xy[2 * a + 1];
  j.heuristic_id = r.heuristic_ids[a];
  j.flags = r.heuristic_ids[a] < 0 ? MRP_LL_JOB_NO_GOAL : 0;
  j.max_expansions = budget;
  struct Sink {
    std::vector<uint32_t> w; bool failed = false;
    size_t size() const { return w.size(); }
    bool fits(size_t) const { return true; }
    void push(uint32_t v) { w.push_back(v); }
    uint32_t* grow(size_t n) { w.resize(w.size() + n); return w.data() + w.size() - n; }
  } cs;
  struct PSink { bool failed = false; uint16_t* alloc(size_t, uint32_t&) { return nullptr; } } ps;
  DevJob o;
  PendingSet pend;
  CHECK(packJob(env, j, PackArgs{}, cs, ps, o, pend));
  o.vc_off = d.vc_off; o.ec_off = d.ec_off;  // (where the empty constraint lists stand is the batch's)
  CHECK(std::memcmp(&o, &d, sizeof(DevJob)) == 0);
}

void packAndUnpack(const PackEnv& env) {
  Root r0(0, 3), bad(0, 3), r64(0, 64), r40(1, 2);
  bad.r.map_id = 7;
  r40.hids[0] = 2; r40.hids[1] = -1;
  r40.starts = {39, 39, 0, 0}; r40.goals = {0, 39, 0, 0};
  const mrp_ll_ta_root roots[4] = {r0.r, bad.r, r64.r, r40.r};
  TaRootStaging st;
  packTaRoots(env, 4, roots, 100, st);
  CHECK(st.recs.size() == 3 && st.nResults == 3 + 64 + 2);
  CHECK(st.devRootOf[0] == 0 && st.devRootOf[1] == -1 && st.devRootOf[2] == 1 && st.devRootOf[3] == 2);
  CHECK(st.firstResult[0] == 0 && st.firstResult[2] == 3 && st.firstResult[3] == 67);
  CHECK(st.words.size() == mrp::kTaRootAgentWords * (3 + 64 + 2));
  CHECK(st.recs[0].vc_off == 100 && st.recs[1].vc_off == 100 + 9 && st.recs[2].vc_off == 100 + 9 + 192);  // the word offsets
  CHECK(st.recs[1].n_ctx == 64 && st.recs[1].reserved == 3 && st.recs[1].max_expansions == 1064);
  CHECK(st.recs[2].dimx == 40 && st.recs[2].map_word_off == 32 && st.recs[2].words_per_row == 50);
  CHECK(st.words[0] == (0u | 0u << 8 | 7u << 16 | 7u << 24) && st.words[1] == 128 && st.words[2] == 0);
  CHECK(st.words[3] == (1u | 0u << 8 | 6u << 16 | 7u << 24) && st.words[4] == 640 && st.words[5] == 0);
  CHECK(st.words[6] == 2u && st.words[7] == 0 && st.words[8] == mrp::kTaNoGoal);  // no task: goal 0, 0, offset 0
  CHECK(st.words[9 + 192] == (39u | 39u << 8 | 0u << 16 | 39u << 24) && st.words[9 + 192 + 1] == 1152);
  for (int a = 0; a < 3; ++a) sameAsOrdinaryJob(env, roots[0], st.recs[0], st.words.data(), a, 500 - a);
  for (int a = 0; a < 64; ++a) sameAsOrdinaryJob(env, roots[2], st.recs[1], st.words.data() + 9, a, -1);
  for (int a = 0; a < 2; ++a) sameAsOrdinaryJob(env, roots[3], st.recs[2], st.words.data() + 9 + 192, a, 0);

  // ---- the way back: exactly the launch's buffers (the sanitizer watches their ends)
  const uint32_t outStride = 64 + mrp::kScanOutHalfs;
  std::vector<DevResult> dres(st.nResults);
  std::vector<uint16_t> out(static_cast<size_t>(st.nResults) * outStride, 0xEEEE);
  std::memset(dres.data(), 0, dres.size() * sizeof(DevResult));
  blankTaRootAnswers(st, out.data(), outStride);
  auto answer = [&](uint32_t first) { return const_cast<uint32_t*>(taRootAnswer(out.data(), outStride, first)); };
  CHECK(answer(0)[0] == 0xFFFFFFFFu && answer(0)[mrp::kTaRootPlannedWord] == 0 && answer(3)[0] == 0xFFFFFFFFu);
  auto path = [&](uint32_t ri, std::vector<uint16_t> cells) {
    dres[ri].status = mrp::ST_OK; dres[ri].n_states = static_cast<int32_t>(cells.size());
    dres[ri].cost = static_cast<int32_t>(cells.size()) - 1; dres[ri].fmin = dres[ri].cost; dres[ri].expanded = 10 + ri;
    std::memcpy(out.data() + static_cast<size_t>(ri) * outStride, cells.data(), cells.size() * 2);
  };
  // root 0 ends behind agent 1 (no path); agent 2 is not run
  path(0, {0, 1, 2, 3 | 7 << 8});
  dres[1].status = mrp::ST_NO_SOLUTION; dres[1].expanded = 77; dres[1].tier = 1;
  answer(0)[mrp::kTaRootPlannedWord] = 2;
  // root 2 (64 agents): all planned, the device scanned: a vertex conflict
  for (uint32_t a = 0; a < 64; ++a) path(3 + a, {static_cast<uint16_t>(a), static_cast<uint16_t>(a + 1)});
  const uint32_t conf[10] = {1, 5, 2, 9, 0, 4, 6, 0, 0, 3};
  std::memcpy(answer(3), conf, sizeof(conf));
  answer(3)[mrp::kTaRootPlannedWord] = 64;
  // root 3: all planned, the scan left to the host; nine states into buffers of eight
  path(67, {0, 1, 2, 3, 4, 5, 6, 7, 8});
  path(68, {0});
  answer(67)[0] = mrp::kTaRootScanSkipped;
  answer(67)[mrp::kTaRootPlannedWord] = 2;

  int32_t planned[4] = {-9, -9, -9, -9};
  mrp_ll_conflict c[4];
  std::memset(c, 0x33, sizeof(c));
  mrp_ll_stats stats;
  std::memset(&stats, 0, sizeof(stats));
  std::vector<int32_t> needScan;
  unpackTaRoots(stats, st, 4, roots, dres.data(), out.data(), outStride, planned, c, needScan);
  CHECK(planned[0] == 2 && planned[1] == 0 && planned[2] == 64 && planned[3] == 2);
  CHECK(needScan.size() == 1 && needScan[0] == 3);
  const mrp_ll_conflict none = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  CHECK(std::memcmp(&c[0], &none, sizeof(none)) == 0 && std::memcmp(&c[1], &none, sizeof(none)) == 0 &&
        std::memcmp(&c[3], &none, sizeof(none)) == 0);
  CHECK(std::memcmp(&c[2], conf, sizeof(conf)) == 0);
  // the stop-behind result
  CHECK(r0.results[0].status == MRP_LL_OK && r0.results[0].n_states == 4 && r0.results[0].cost == 3 && r0.results[0].expanded == 10);
  CHECK(r0.states[0][9] == 3 && r0.states[0][10] == 3 && r0.states[0][11] == 7 && r0.actions[0][0] == MRP_LL_ACT_RIGHT);
  CHECK(r0.costs[0][2] == 1);
  CHECK(r0.results[1].status == MRP_LL_NO_SOLUTION && r0.results[1].n_states == 0 && r0.results[1].expanded == 77 && r0.results[1].tier == 1);
  CHECK(r0.results[2].status == MRP_LL_NOT_RUN && r0.results[2].cost == 0 && r0.results[2].fmin == 0 && r0.results[2].n_states == 0 &&
        r0.results[2].expanded == 0 && r0.results[2].tier == 0);
  CHECK(r0.results[2].states_txy == r0.states[2].data() && r0.results[2].states_cap == 8);  // the caller's buffers stay the caller's
  for (int a = 0; a < 3; ++a)
    CHECK(bad.results[a].status == MRP_LL_BAD_JOB && bad.results[a].cost == 0 && bad.results[a].n_states == 0 && bad.results[a].expanded == 0);
  CHECK(r64.results[63].status == MRP_LL_OK && r64.states[63][1] == 63 && r64.states[63][4] == 64);
  CHECK(r40.results[0].status == MRP_LL_PATH_TRUNCATED && r40.results[0].n_states == 9 && r40.results[1].n_states == 1);
  CHECK(stats.jobs == 2 + 64 + 2);
  // what the caller holds when a step of the call failed: nothing ran, refused roots say so
  blankTaRootOutputs(env, 4, roots, planned, c);
  for (int k = 0; k < 4; ++k) CHECK(planned[k] == 0 && std::memcmp(&c[k], &none, sizeof(none)) == 0);
  CHECK(r0.results[0].status == MRP_LL_NOT_RUN && r0.results[0].n_states == 0 && r0.results[0].cost == 0 && r0.results[0].expanded == 0);
  CHECK(r64.results[63].status == MRP_LL_NOT_RUN && r40.results[0].status == MRP_LL_NOT_RUN && bad.results[2].status == MRP_LL_BAD_JOB);
  CHECK(r0.results[0].states_txy == r0.states[0].data());
  // a device that reports more results than the root has agents is not believed
  answer(0)[mrp::kTaRootPlannedWord] = 1000;
  dres[1].status = mrp::ST_OK; dres[1].n_states = 1; dres[2].status = mrp::ST_OK; dres[2].n_states = 1;
  unpackTaRoots(stats, st, 4, roots, dres.data(), out.data(), outStride, planned, c, needScan);
  CHECK(planned[0] == 3);
}

}  // namespace

int main() {
  const PackEnv env = makeEnv();
  refusals(env);
  packAndUnpack(env);
  std::printf("ta_root_pack_check: ok\n");
  return 0;
}
