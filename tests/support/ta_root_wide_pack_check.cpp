// TEST INFRASTRUCTURE — a stand-alone check of the packers of mrp_ll_ta_root_batch_w and mrp_ll_ta_eps_root_batch_w
// (libmultirobotplanning_amd/csrc/host/ta_root_pack.h and ta_eps_root_pack.h with the agent limit as a parameter), built by
// tests/test_ta_root_wide_pack_cpu.py with the host sanitizers and run as a program of its own: the refusals at 0 and 257
// agents, the 256-agent record's word offsets, and the narrow validity, which still refuses 65.  Exits non-zero at the
// first failed check.  With -DEPS the same through packTaEpsRoots (algo and weight in the record).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/ta_eps_root_pack.h"

using namespace mrp::host;
using mrp::DevJob;

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "ta_root_wide_pack_check: line %d: %s\n", __LINE__, #cond);   \
      std::exit(1);                                                                      \
    }                                                                                    \
  } while (0)

namespace {

struct Root {  // n agents on a 32 x 32 map, agent a at (a % 32, a / 32), every third without a task
  std::vector<int32_t> starts, goals, hids;
  std::vector<mrp_ll_result> results;
  mrp_ll_ta_root r;
  explicit Root(int n) : starts(2 * (n > 0 ? n : 1)), goals(2 * (n > 0 ? n : 1)), hids(n > 0 ? n : 1), results(n > 0 ? n : 1) {
    for (int a = 0; a < n; ++a) {
      starts[2 * a] = a % 32; starts[2 * a + 1] = a / 32;
      goals[2 * a] = 31 - a % 32; goals[2 * a + 1] = 31 - a / 32;
      hids[a] = a % 3 == 2 ? -1 : a % 2;
      std::memset(&results[a], 0, sizeof(mrp_ll_result));
    }
    std::memset(&r, 0, sizeof(r));
    r.map_id = 0; r.n_agents = n;
    r.starts_xy = starts.data(); r.goals_xy = goals.data(); r.heuristic_ids = hids.data();
    r.max_expansions = 1000;
    r.results = results.data();
  }
};

void pack(const PackEnv& env, int32_t n, const mrp_ll_ta_root* roots, uint32_t wordBase, TaRootStaging& st, uint32_t maxAgents) {
#ifdef EPS
  packTaEpsRoots(env, 1.5f, n, roots, wordBase, st, nullptr, maxAgents);
#else
  packTaRoots(env, n, roots, wordBase, st, maxAgents);
#endif
}

}  // namespace

int main() {
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{32, 32, 1, 0});
  env.heurs.push_back(HeurRec{0, 128});
  env.heurs.push_back(HeurRec{0, 640});
  env.maxHorizon = 64;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 128 * 1024;
  const uint32_t wide = mrp::kTaRootWideMaxAgents;
  CHECK(wide == 256 && mrp::kTaRootMaxAgents == 64);

  Root r0(0), r1(1), r64(64), r65(65), r256(256), r257(257);
  // the narrow validity, as every caller of today uses it
  CHECK(!taRootValid(env, r0.r) && taRootValid(env, r1.r) && taRootValid(env, r64.r) && !taRootValid(env, r65.r));
  CHECK(!taRootValid(env, r256.r) && !taRootValid(env, r257.r));
  // the wide one
  CHECK(!taRootValid(env, r0.r, nullptr, wide) && taRootValid(env, r1.r, nullptr, wide) && taRootValid(env, r65.r, nullptr, wide));
  CHECK(taRootValid(env, r256.r, nullptr, wide) && !taRootValid(env, r257.r, nullptr, wide));

  // one batch: refused roots between accepted ones
  const mrp_ll_ta_root roots[6] = {r65.r, r0.r, r256.r, r257.r, r1.r, r64.r};
  TaRootStaging st;
  const uint32_t base = 100;
  pack(env, 6, roots, base, st, wide);
  CHECK(st.recs.size() == 4 && st.nResults == 65 + 256 + 1 + 64);
  CHECK(st.devRootOf[0] == 0 && st.devRootOf[1] == -1 && st.devRootOf[2] == 1 && st.devRootOf[3] == -1 && st.devRootOf[4] == 2 &&
        st.devRootOf[5] == 3);
  CHECK(st.firstResult[0] == 0 && st.firstResult[2] == 65 && st.firstResult[4] == 65 + 256 && st.firstResult[5] == 65 + 256 + 1);
  CHECK(st.words.size() == mrp::kTaRootAgentWords * (65 + 256 + 1 + 64) && st.slotWords.empty());
  // the 256-agent record: its words stand behind the 65-agent root's, three per agent
  const DevJob& d = st.recs[1];
  CHECK(d.n_ctx == 256 && d.reserved == 65 && d.vc_off == base + mrp::kTaRootAgentWords * 65 && d.ec_off == d.vc_off);
  CHECK(d.dimx == 32 && d.dimy == 32 && d.max_expansions == 1000 && d.store_out_id == mrp::kNoStoreSlot);
#ifdef EPS
  CHECK(d.algo == MRP_LL_ASTAR_EPS_TA && d.w == 1.5f);
#else
  CHECK(d.algo == MRP_LL_ASTAR_TA);
#endif
  const uint32_t* w = st.words.data() + (d.vc_off - base);
  for (uint32_t a = 0; a < 256; ++a) {
    const bool noGoal = a % 3 == 2;
    const uint32_t sg = (a % 32) | ((a / 32) << 8) | (noGoal ? 0u : ((31 - a % 32) << 16) | ((31 - a / 32) << 24));
    CHECK(w[3 * a] == sg);
    CHECK(w[3 * a + 1] == (noGoal ? 0u : (a % 2 ? 640u : 128u)));
    CHECK(w[3 * a + 2] == (noGoal ? mrp::kTaNoGoal : 0u));
  }
  CHECK(st.recs[2].vc_off == d.vc_off + mrp::kTaRootAgentWords * 256 && st.recs[2].n_ctx == 1 && st.recs[2].reserved == 65 + 256);
  // the same batch through the narrow limit: the 65- and 256-agent roots are refused too
  pack(env, 6, roots, base, st, mrp::kTaRootMaxAgents);
  CHECK(st.recs.size() == 2 && st.devRootOf[0] == -1 && st.devRootOf[2] == -1 && st.devRootOf[4] == 0 && st.devRootOf[5] == 1);
  // what the caller holds when nothing ran: a refused root's results say MRP_LL_BAD_JOB for as many agents as it named
  std::vector<int32_t> planned(6, 7);
  std::vector<mrp_ll_conflict> conf(6);
  blankTaRootOutputs(env, 6, roots, planned.data(), conf.data(), nullptr, wide);
  CHECK(r257.results[256].status == MRP_LL_BAD_JOB && r256.results[255].status == MRP_LL_NOT_RUN && r65.results[64].status == MRP_LL_NOT_RUN);
  blankTaRootOutputs(env, 6, roots, planned.data(), conf.data());
  CHECK(r65.results[64].status == MRP_LL_BAD_JOB && r64.results[63].status == MRP_LL_NOT_RUN && planned[2] == 0 && conf[2].found == -1);
  std::printf("ta_root_wide_pack_check%s: ok\n",
#ifdef EPS
              " (eps)"
#else
              ""
#endif
  );
  return 0;
}
