// TEST INFRASTRUCTURE — a stand-alone check of MRP_LL_JOB_TRY_LDS in the host packer (libmultirobotplanning_amd/csrc/host/
// ll_pack.h packJob), built by tests/test_eps_ta_try_lds_pack_cpu.py with the host sanitizers and run as a program of its
// own: the flag reaches ctx_flags (bit kCtxTryLds) of an MRP_LL_ASTAR_EPS_TA job and changes nothing else of its descriptor
// or of what is pushed, it combines with MRP_LL_JOB_NO_GOAL, MRP_LL_JOB_STORE_RESULT and path_ids, it is dropped for every
// other algorithm, a zero-initialised job never sets it, and what is rejected without it stays rejected with it.
// Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/ll_pack.h"

using namespace mrp::host;
using mrp::DevJob;

#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      std::fprintf(stderr, "eps_ta_try_lds_pack_check: line %d: %s\n", __LINE__, #cond); \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)

namespace {

struct Sink {
  std::vector<uint32_t> w;
  bool failed = false;
  size_t size() const { return 1000 + w.size(); }
  bool fits(size_t) const { return true; }
  void push(uint32_t v) { w.push_back(v); }
  uint32_t* grow(size_t n) { w.resize(w.size() + n); return w.data() + w.size() - n; }
};
struct PSink {
  std::vector<uint16_t> tab;
  bool failed = false;
  uint16_t* alloc(size_t n, uint32_t& off) { off = 48; tab.assign(n, 0x1234); return tab.data(); }
};

PackEnv makeEnv() {  // map 0: 8 x 8 at word 0; table 0 of map 0; a path store of 40 slots
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{8, 8, 2, 0});
  env.heurs.push_back(HeurRec{0, 128});
  env.maxHorizon = 64;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 4096;
  env.pathStoreSlots = 40;
  return env;
}

struct Packed {
  bool ok;
  DevJob d;
  std::vector<uint32_t> cons;
  std::vector<uint16_t> tab;
};
Packed pack(const PackEnv& env, const mrp_ll_job& j) {
  Packed p;
  Sink cs;
  PSink ps;
  PendingSet pend;
  std::memset(&p.d, 0, sizeof(p.d));
  p.ok = packJob(env, j, PackArgs{}, cs, ps, p.d, pend);
  p.cons = cs.w;
  p.tab = ps.tab;
  return p;
}

// with and without the flag: accepted alike, and equal but for the one bit (`expectBit`: set with the flag)
void pairOf(const PackEnv& env, mrp_ll_job j, bool expectBit, int line) {
  j.flags &= ~MRP_LL_JOB_TRY_LDS;
  const Packed a = pack(env, j);
  j.flags |= MRP_LL_JOB_TRY_LDS;
  Packed b = pack(env, j);
  bool good = a.ok == b.ok;
  if (good && a.ok) {
    good = !(a.d.ctx_flags & mrp::kCtxTryLds) && ((b.d.ctx_flags & mrp::kCtxTryLds) != 0) == expectBit;
    b.d.ctx_flags &= ~mrp::kCtxTryLds;
    good = good && std::memcmp(&a.d, &b.d, sizeof(DevJob)) == 0 && a.cons == b.cons && a.tab == b.tab;
  }
  if (!good) {
    std::fprintf(stderr, "eps_ta_try_lds_pack_check: line %d: the flag changed more than its bit\n", line);
    std::exit(1);
  }
}
#define PAIR(env, j, bit) pairOf(env, j, bit, __LINE__)

mrp_ll_job baseJob(int algo) {
  mrp_ll_job j;
  std::memset(&j, 0, sizeof(j));
  j.map_id = 0; j.algo = algo; j.w = 1.5f;
  j.start_x = 1; j.start_y = 2; j.goal_x = 6; j.goal_y = 5;
  j.heuristic_id = 0;
  j.max_expansions = -1;
  j.result_path_id = -1;
  return j;
}

}  // namespace

int main() {
  const PackEnv env = makeEnv();
  static_assert(MRP_LL_JOB_TRY_LDS == 128, "the flag's value is part of the C ABI");
  static_assert((mrp::kCtxTryLds & (mrp::kCtxById | mrp::kSippResident | mrp::kSippNoLds | mrp::kSippCommit | mrp::kTaNoGoal |
                                    mrp::kCtxChain | mrp::kCtxHeavy | mrp::kCtxScan | mrp::kCtxScanParent)) == 0,
                "a ctx_flags bit of its own");
  const int32_t vc[2][3] = {{3, 1, 1}, {4, 6, 5}};
  const int32_t ec[1][5] = {{2, 1, 1, 2, 1}};
  {  // the plain job, with constraints
    mrp_ll_job j = baseJob(MRP_LL_ASTAR_EPS_TA);
    j.n_vertex_constraints = 2; j.vertex_constraints = &vc[0][0];
    j.n_edge_constraints = 1; j.edge_constraints = &ec[0][0];
    PAIR(env, j, true);
    j.flags = MRP_LL_JOB_TRY_LDS;
    const Packed p = pack(env, j);
    CHECK(p.ok && (p.d.ctx_flags & mrp::kCtxTryLds) && p.d.n_vc == 2 && p.d.n_ec == 1 && p.d.algo == MRP_LL_ASTAR_EPS_TA);
  }
  {  // a zero-initialised job never sets it
    mrp_ll_job j = baseJob(MRP_LL_ASTAR_EPS_TA);
    const Packed p = pack(env, j);
    CHECK(p.ok && !(p.d.ctx_flags & mrp::kCtxTryLds));
  }
  {  // ... with MRP_LL_JOB_NO_GOAL
    mrp_ll_job j = baseJob(MRP_LL_ASTAR_EPS_TA);
    j.flags = MRP_LL_JOB_NO_GOAL; j.heuristic_id = -1;
    PAIR(env, j, true);
    j.flags |= MRP_LL_JOB_TRY_LDS;
    const Packed p = pack(env, j);
    CHECK(p.ok && (p.d.ctx_flags & mrp::kTaNoGoal) && (p.d.ctx_flags & mrp::kCtxTryLds));
  }
  {  // ... with a shipped context, with path_ids, with MRP_LL_JOB_STORE_RESULT
    std::vector<int32_t> len = {3, 0, 2}, ids = {7, -1, 9};
    const int32_t p0[6] = {1, 1, 2, 1, 3, 1}, p2[4] = {5, 5, 5, 6};
    const int32_t* xy[3] = {p0, nullptr, p2};
    mrp_ll_job j = baseJob(MRP_LL_ASTAR_EPS_TA);
    j.agent_idx = 1; j.n_agents = 3; j.path_len = len.data(); j.path_xy = xy;
    PAIR(env, j, true);
    j.path_ids = ids.data(); j.path_xy = nullptr;
    PAIR(env, j, true);
    j.flags = MRP_LL_JOB_STORE_RESULT | MRP_LL_JOB_TRY_LDS; j.result_path_id = 17;
    const Packed p = pack(env, j);
    CHECK(p.ok && (p.d.ctx_flags & mrp::kCtxById) && (p.d.ctx_flags & mrp::kCtxTryLds) && p.d.store_out_id == 17u);
    PAIR(env, j, true);
  }
  // dropped for every other algorithm
  for (int algo : {MRP_LL_ASTAR, MRP_LL_ASTAR_EPS, MRP_LL_ASTAR_TA}) {
    mrp_ll_job j = baseJob(algo);
    PAIR(env, j, false);
    j.flags = MRP_LL_JOB_TRY_LDS;
    const Packed p = pack(env, j);
    CHECK(p.ok && !(p.d.ctx_flags & mrp::kCtxTryLds));
  }
  {  // what is rejected without it stays rejected with it
    mrp_ll_job j = baseJob(MRP_LL_ASTAR_EPS_TA);
    j.flags = MRP_LL_JOB_HEAVY | MRP_LL_JOB_TRY_LDS;
    CHECK(!pack(env, j).ok);
    j.flags = MRP_LL_JOB_ROOT_CHAIN | MRP_LL_JOB_TRY_LDS;
    CHECK(!pack(env, j).ok);
    j.flags = MRP_LL_JOB_TRY_LDS; j.initial_cost = 3;
    CHECK(!pack(env, j).ok);
    j.initial_cost = 0; j.heuristic_id = 5;
    CHECK(!pack(env, j).ok);
    j.heuristic_id = 0; j.flags = MRP_LL_JOB_STORE_RESULT | MRP_LL_JOB_TRY_LDS; j.result_path_id = 40;
    CHECK(!pack(env, j).ok);
  }
  std::printf("eps_ta_try_lds_pack_check: ok\n");
  return 0;
}
