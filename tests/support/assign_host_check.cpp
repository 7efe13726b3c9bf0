// TEST INFRASTRUCTURE — a stand-alone check of the assignment packer's validation
// (libmultirobotplanning_amd/csrc/host/assign_pack.h: pure host logic, no HIP), built by tests/test_assign_host_cpu.py
// with the host sanitizers and run as a program of its own.  A problem out of range comes back MRP_LL_BAD_JOB and is not
// staged; its neighbours are staged exactly as they are without it.  Exits non-zero at the first failed check.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/assign_pack.h"

using namespace mrp::host;
namespace as = mrp::as;

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "assign_host_check: line %d: %s\n", __LINE__, #cond); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

namespace {

const int32_t kGood[4] = {90, 76, 35, MRP_LL_ASSIGN_NO_EDGE};

mrp_ll_assign_problem good() { return mrp_ll_assign_problem{2, 2, kGood, nullptr, nullptr, nullptr, nullptr, nullptr, 0}; }

struct Out {  // a caller's result with a task_of block of exactly n_agents words
  std::vector<int32_t> taskOf;
  mrp_ll_assign_result r;
  explicit Out(int n) : taskOf(n > 0 ? n : 0, 7), r{-9, -9, -9, n > 0 ? taskOf.data() : nullptr} {}
};

// packs good, bad, good: the bad one is rejected, the staging equals that of good, good alone
void expectBad(const PackEnv& env, const mrp_ll_assign_problem& bad, int line) {
  const mrp_ll_assign_problem three[3] = {good(), bad, good()};
  Out a(2), b(bad.n_agents), c(2);
  mrp_ll_assign_result res[3] = {a.r, b.r, c.r};
  AssignStaging st;
  packAssignBatch(env, 3, three, res, st);
  if (res[1].status != MRP_LL_BAD_JOB) {
    std::fprintf(stderr, "assign_host_check: the problem of line %d was not rejected\n", line);
    std::exit(1);
  }
  CHECK(res[0].status == MRP_LL_OK && res[2].status == MRP_LL_OK);
  CHECK(res[1].matched == 0 && res[1].cost == 0);
  for (int i = 0; i < bad.n_agents && i < 64; ++i) CHECK(b.taskOf[i] == -1);
  const mrp_ll_assign_problem two[2] = {good(), good()};
  mrp_ll_assign_result res2[2] = {a.r, c.r};
  AssignStaging want;
  packAssignBatch(env, 2, two, res2, want);
  CHECK(st.jobs.size() == 2 && st.problemOf[0] == 0 && st.problemOf[1] == 2);
  CHECK(st.data == want.data && st.outWords == want.outWords && st.ldsBytes == want.ldsBytes);
  for (int k = 0; k < 2; ++k) {
    CHECK(st.jobs[k].costOff == want.jobs[k].costOff && st.jobs[k].agentOff == want.jobs[k].agentOff);
    CHECK(st.jobs[k].outOff == want.jobs[k].outOff && st.jobs[k].nA == 2 && st.jobs[k].nT == 2);
  }
}
#define EXPECT_BAD(env, p) expectBad(env, p, __LINE__)

}  // namespace

int main() {
  PackEnv env;  // one 4 x 3 map with one table, one 40 x 40 map with one table
  env.maps.push_back(MapRec{4, 3, 1, 0});
  env.maps.push_back(MapRec{40, 40, 50, 32});
  env.heurs.push_back(HeurRec{0, 128});
  env.heurs.push_back(HeurRec{1, 1024});

  {  // what a sound problem is staged as
    const mrp_ll_assign_problem p = good();
    Out o(2);
    AssignStaging st;
    packAssignBatch(env, 1, &p, &o.r, st);
    CHECK(o.r.status == MRP_LL_OK && st.jobs.size() == 1);
    const as::AssignJob& j = st.jobs[0];
    CHECK(j.nA == 2 && j.nT == 2 && j.minMatching == 0 && j.costOff == 0 && j.agentOff == 4 && j.outOff == 0);
    CHECK(st.data.size() == 4 + 2 * as::kAgentWords && st.outWords == as::kOutHeadWords + 2 && st.ldsBytes == 2 * as::kRowBytes);
    CHECK(st.data[0] == 90 && st.data[3] == as::kNoEdge && st.data[4 + 2] == as::kModeFree);
  }
  std::vector<int32_t> big(65 * 65, 1);
  mrp_ll_assign_problem p = good();
  p.n_agents = 65;
  p.n_tasks = 1;
  p.cost = big.data();
  EXPECT_BAD(env, p);
  p.n_agents = 1;
  p.n_tasks = 65;
  EXPECT_BAD(env, p);
  p = good();
  p.n_agents = -1;
  EXPECT_BAD(env, p);
  const int32_t over[4] = {1, 2, 3, (int32_t)as::kMaxCost + 1}, neg[4] = {1, -1, 3, 4}, top[4] = {1, 2, 3, (int32_t)as::kMaxCost};
  p = good();
  p.cost = over;
  EXPECT_BAD(env, p);
  p.cost = neg;
  EXPECT_BAD(env, p);
  const int32_t forcedOut[2] = {2, MRP_LL_ASSIGN_FREE}, unknownMode[2] = {MRP_LL_ASSIGN_FREE, -4}, forcedIn[2] = {1, MRP_LL_ASSIGN_SOME_TASK};
  p = good();
  p.mode = forcedOut;
  EXPECT_BAD(env, p);
  p.mode = unknownMode;
  EXPECT_BAD(env, p);
  p = good();
  p.min_matching = 65;
  EXPECT_BAD(env, p);
  p.min_matching = -1;
  EXPECT_BAD(env, p);
  // the gather form
  const int32_t ids[2] = {0, 0}, idsUnknown[2] = {0, 2}, idsTwoMaps[2] = {0, 1};
  const int32_t starts[4] = {3, 2, 0, 0}, startsOut[4] = {4, 0, 0, 0};
  mrp_ll_assign_problem g{2, 2, nullptr, ids, starts, nullptr, nullptr, nullptr, 0};
  g.heuristic_ids = idsUnknown;
  EXPECT_BAD(env, g);
  g.heuristic_ids = idsTwoMaps;
  EXPECT_BAD(env, g);
  g.heuristic_ids = ids;
  g.starts_xy = startsOut;
  EXPECT_BAD(env, g);
  g.starts_xy = nullptr;
  EXPECT_BAD(env, g);
  {  // at the limits nothing is rejected
    mrp_ll_assign_problem q = good();
    q.cost = top;
    q.mode = forcedIn;
    q.min_matching = 64;
    const uint64_t allowed[2] = {1, ~0ull};
    g.starts_xy = starts;
    g.allowed = allowed;
    const mrp_ll_assign_problem two[2] = {q, g};
    Out a(2), b(2);
    mrp_ll_assign_result res[2] = {a.r, b.r};
    AssignStaging st;
    packAssignBatch(env, 2, two, res, st);
    CHECK(res[0].status == MRP_LL_OK && res[1].status == MRP_LL_OK && st.jobs.size() == 2);
    const as::AssignJob& j = st.jobs[1];
    CHECK(j.costOff == as::kNoCostOff && st.data[j.taskOff] == 128 && st.data[j.taskOff + 1] == 128);
    CHECK(st.data[j.agentOff] == 0xFFFFFFFEu && st.data[j.agentOff + 1] == 0xFFFFFFFFu);  // ~allowed is forbidden
    CHECK(st.data[j.agentOff + 3] == 2 * 32 + 3 && st.data[j.agentOff + as::kAgentWords + 3] == 0);  // stride 32 up to 32 x 32
    CHECK(st.data[st.jobs[0].agentOff + 2] == 1 && st.data[st.jobs[0].agentOff + as::kAgentWords + 2] == as::kModeSomeTask);
  }
  std::printf("assign_host_check: ok\n");
  return 0;
}
