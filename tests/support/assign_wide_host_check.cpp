// TEST INFRASTRUCTURE — a stand-alone check of the wide assignment packer (libmultirobotplanning_amd/csrc/host/
// assign_pack.h: packAssignBatchWide) and of the next-best series generalised to mask words (host/assign_series.h), built
// by tests/test_assign_wide_host_cpu.py with the host sanitizers and run as a program of its own: the limits, the staged
// words of a 65 x 130 problem, the row-source choice at the budget's edge, and a narrow series that stages the words it
// staged before the generalisation.  The series' problems are solved by the CPU emulation of the two wave programs.
// Exits non-zero at the first failed check.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wave_emu_assign.h"
#include "../../libmultirobotplanning_amd/csrc/assign_wave_wide.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_pack.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_series.h"

using namespace mrp::host;
namespace as = mrp::as;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      std::fprintf(stderr, "assign_wide_host_check: line %d: %s\n", __LINE__, #cond); \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

namespace {

const int32_t kGood[4] = {90, 76, 35, MRP_LL_ASSIGN_NO_EDGE};
const uint32_t kBudget = as::kLdsBudgetWide;

mrp_ll_assign_problem_w good() { return mrp_ll_assign_problem_w{2, 2, kGood, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1}; }

struct Out {  // a caller's result with a task_of block of exactly n_agents words
  std::vector<int32_t> taskOf;
  mrp_ll_assign_result r;
  explicit Out(int n) : taskOf(n > 0 ? n : 0, 7), r{-9, -9, -9, n > 0 ? taskOf.data() : nullptr} {}
};

// packs good, bad, good: the bad one is rejected, the staging equals that of good, good alone
void expectBad(const PackEnv& env, const mrp_ll_assign_problem_w& bad, int line) {
  const mrp_ll_assign_problem_w three[3] = {good(), bad, good()};
  Out a(2), b(bad.n_agents), c(2);
  mrp_ll_assign_result res[3] = {a.r, b.r, c.r};
  AssignStagingWide st;
  packAssignBatchWide(env, 3, three, res, kBudget, st);
  if (res[1].status != MRP_LL_BAD_JOB) {
    std::fprintf(stderr, "assign_wide_host_check: the problem of line %d was not rejected\n", line);
    std::exit(1);
  }
  CHECK(res[0].status == MRP_LL_OK && res[2].status == MRP_LL_OK);
  CHECK(res[1].matched == 0 && res[1].cost == 0);
  for (int i = 0; i < bad.n_agents && i < 256; ++i) CHECK(b.taskOf[i] == -1);
  const mrp_ll_assign_problem_w two[2] = {good(), good()};
  mrp_ll_assign_result res2[2] = {a.r, c.r};
  AssignStagingWide want;
  packAssignBatchWide(env, 2, two, res2, kBudget, want);
  CHECK(st.jobs.size() == 2 && st.problemOf[0] == 0 && st.problemOf[1] == 2);
  CHECK(st.data == want.data && st.outWords == want.outWords && st.ldsBytes == want.ldsBytes && st.scratchWords == 0);
  for (int k = 0; k < 2; ++k) {
    CHECK(st.jobs[k].costOff == want.jobs[k].costOff && st.jobs[k].agentOff == want.jobs[k].agentOff);
    CHECK(st.jobs[k].outOff == want.jobs[k].outOff && st.jobs[k].nA == 2 && st.jobs[k].nT == 2 && st.jobs[k].words == 1);
  }
}
#define EXPECT_BAD(env, p) expectBad(env, p, __LINE__)

// the two wave programs on the CPU emulator, recording what each call staged
struct Solvers {
  std::vector<std::vector<uint32_t>> narrowData, wideData;
  std::vector<int> narrowJobs, wideJobs;
  AssignSolveFn narrow() {
    return [this](int32_t n, const mrp_ll_assign_problem* ps, mrp_ll_assign_result* rs) {
      const PackEnv env;
      const std::vector<uint32_t> maps(1, 0);
      AssignStaging st;
      packAssignBatch(env, n, ps, rs, st);
      narrowData.push_back(st.data);
      narrowJobs.push_back((int)st.jobs.size());
      std::vector<uint32_t> out(st.outWords, 0xA5A5A5A5u);
      for (const as::AssignJob& job : st.jobs) {
        std::vector<uint8_t> mem(st.ldsBytes, 0xCD);
        wv::LdsWindow win{mem.data(), as::ldsBytes(job.nA), 0, 0};
        as::assignSolve(&win, maps.data(), st.data.data(), out.data(), job);
        CHECK(win.oobReads == 0 && win.oobWrites == 0);
      }
      unpackAssignBatch(st, out.data(), rs);
      return (int)MRP_LL_SUCCESS;
    };
  }
  AssignSolveWideFn wide() {
    return [this](int32_t n, const mrp_ll_assign_problem_w* ps, mrp_ll_assign_result* rs) {
      const PackEnv env;
      const std::vector<uint32_t> maps(1, 0);
      AssignStagingWide st;
      packAssignBatchWide(env, n, ps, rs, kBudget, st);
      wideData.push_back(st.data);
      wideJobs.push_back((int)st.jobs.size());
      std::vector<uint32_t> out(st.outWords + st.scratchWords, 0xA5A5A5A5u);
      for (const as::AssignJobWide& job : st.jobs) {
        std::vector<uint8_t> mem(as::ldsBytesWide(job.nA, job.nT, kBudget), 0xCD);
        wv::LdsWindow win{mem.data(), (uint32_t)mem.size(), 0, 0};
        as::assignSolveWideAny(&win, maps.data(), st.data.data(), out.data(), job);
        CHECK(win.oobReads == 0 && win.oobWrites == 0);
      }
      unpackAssignBatchWide(st, out.data(), rs);
      return (int)MRP_LL_SUCCESS;
    };
  }
};

}  // namespace

int main() {
  PackEnv env;  // one 4 x 3 map with one table
  env.maps.push_back(MapRec{4, 3, 1, 0});
  env.heurs.push_back(HeurRec{0, 128});

  {  // what a sound problem is staged as: the narrow layout with the record mode, start, forbidden (low, high)
    const mrp_ll_assign_problem_w p = good();
    Out o(2);
    AssignStagingWide st;
    packAssignBatchWide(env, 1, &p, &o.r, kBudget, st);
    CHECK(o.r.status == MRP_LL_OK && st.jobs.size() == 1 && st.outWords == as::kOutHeadWords + 2);
    const as::AssignJobWide& j = st.jobs[0];
    CHECK(j.words == 1 && j.rowSource == as::kRowsLds && j.costOff == 0 && j.agentOff == 4 && st.data.size() == 4 + 2 * 4);
    CHECK(st.data[3] == as::kNoEdge && st.data[4] == as::kModeFree && st.data[5] == 0 && st.data[6] == 0 && st.data[7] == 0);
    CHECK(st.ldsBytes == 2 * 256 && st.scratchWords == 0);
  }

  // the limits
  const std::vector<int32_t> zeros(257 * 2, 0);
  const std::vector<uint64_t> noMask(257 * 5, 0);
  {
    mrp_ll_assign_problem_w p = good();
    p.n_agents = 257, p.n_tasks = 1, p.cost = zeros.data();
    EXPECT_BAD(env, p);
    p.n_agents = 1, p.n_tasks = 257;
    EXPECT_BAD(env, p);
    p = good(), p.mask_words = 0;
    EXPECT_BAD(env, p);
    p.mask_words = 5;
    EXPECT_BAD(env, p);
    p = good(), p.n_agents = 1, p.n_tasks = 65, p.cost = zeros.data(), p.forbidden = noMask.data(), p.mask_words = 1;
    EXPECT_BAD(env, p);  // a mask of one word for 65 tasks
    p.forbidden = nullptr;
    {  // ... which is sound without a mask, and with two words
      Out o(1);
      AssignStagingWide st;
      packAssignBatchWide(env, 1, &p, &o.r, kBudget, st);
      CHECK(o.r.status == MRP_LL_OK);
      p.forbidden = noMask.data(), p.mask_words = 2;
      packAssignBatchWide(env, 1, &p, &o.r, kBudget, st);
      CHECK(o.r.status == MRP_LL_OK);
    }
    p = good(), p.min_matching = 257;
    EXPECT_BAD(env, p);
    p.min_matching = -1;
    EXPECT_BAD(env, p);
    const int32_t forcedBeyond[2] = {2, MRP_LL_ASSIGN_FREE}, unknownMode[2] = {-4, MRP_LL_ASSIGN_FREE};
    p = good(), p.mode = forcedBeyond;
    EXPECT_BAD(env, p);
    p.mode = unknownMode;
    EXPECT_BAD(env, p);
    const int32_t dear[4] = {1, 2, 3, 1 << 24};
    p = good(), p.cost = dear;
    EXPECT_BAD(env, p);
    {  // 256 x 256 with min_matching 256 is sound
      const std::vector<int32_t> big(256 * 256, 5);
      p = good(), p.n_agents = p.n_tasks = p.min_matching = 256, p.cost = big.data(), p.mask_words = 4;
      Out o(256);
      AssignStagingWide st;
      packAssignBatchWide(env, 1, &p, &o.r, kBudget, st);
      CHECK(o.r.status == MRP_LL_OK && st.jobs[0].words == 4 && st.jobs[0].rowSource == as::kRowsMem && st.ldsBytes == 0);
      CHECK(st.scratchWords == 0);  // the matrix form reads the staged costs themselves
    }
  }

  {  // the staged words of a 65 x 130 problem: C = 3, records of 2 + 6 words
    const int nA = 65, nT = 130;
    std::vector<int32_t> cost((size_t)nA * nT);
    for (size_t k = 0; k < cost.size(); ++k) cost[k] = k % 7 == 0 ? MRP_LL_ASSIGN_NO_EDGE : (int32_t)(k % 1000);
    std::vector<uint64_t> forb((size_t)nA * 3, 0);
    forb[64 * 3 + 2] = 1ull << 1 | 1ull << 63;  // agent 64: task 129, and bit 191 (beyond n_tasks: staged as given, ignored)
    forb[1 * 3 + 0] = 1ull << 63;               // agent 1: task 63
    forb[1 * 3 + 1] = 1ull << 32;               // agent 1: task 96
    std::vector<int32_t> mode(nA, MRP_LL_ASSIGN_FREE);
    mode[64] = 128, mode[2] = MRP_LL_ASSIGN_NO_TASK, mode[3] = MRP_LL_ASSIGN_SOME_TASK;
    const mrp_ll_assign_problem_w p{nA, nT, cost.data(), nullptr, nullptr, nullptr, forb.data(), mode.data(), 7, 3};
    Out o(nA);
    AssignStagingWide st;
    packAssignBatchWide(env, 1, &p, &o.r, kBudget, st);
    CHECK(o.r.status == MRP_LL_OK && st.jobs.size() == 1);
    const as::AssignJobWide& j = st.jobs[0];
    CHECK(j.nA == 65 && j.nT == 130 && j.minMatching == 7 && j.words == 3 && j.costOff == 0 && j.agentOff == 65 * 130);
    CHECK(as::agentWordsWide(3) == 8 && st.data.size() == 65 * 130 + 65 * 8);
    CHECK(j.rowSource == as::kRowsLds && st.ldsBytes == 65 * 768 && st.outWords == as::kOutHeadWords + 65);
    CHECK(st.data[0] == as::kNoEdge && st.data[1] == 1 && st.data[65 * 130 - 2] == (65 * 130 - 2) % 1000);
    const uint32_t* r = st.data.data() + j.agentOff;
    CHECK(r[0] == as::kModeFree && r[1] == 0);
    for (int w = 2; w < 8; ++w) CHECK(r[w] == 0);
    CHECK(r[8 + 2] == 0 && r[8 + 3] == 0x80000000u && r[8 + 4] == 0 && r[8 + 5] == 1 && r[8 + 6] == 0 && r[8 + 7] == 0);
    CHECK(r[2 * 8] == as::kModeNoTask && r[3 * 8] == as::kModeSomeTask && r[64 * 8] == 128);
    CHECK(r[64 * 8 + 6] == 2 && r[64 * 8 + 7] == 0x80000000u && r[64 * 8 + 2] == 0);
    // the gather form: two mask words given for 65 tasks, C = 2; ~allowed is forbidden
    const int gA = 70, gT = 65;
    const std::vector<int32_t> ids(gT, 0);
    std::vector<int32_t> starts(2 * gA, 0);
    starts[2 * 69] = 3, starts[2 * 69 + 1] = 2;
    std::vector<uint64_t> allowed((size_t)gA * 2, ~0ull);
    allowed[69 * 2 + 1] = 0;  // agent 69 may not take task 64
    allowed[0] = ~1ull;
    const mrp_ll_assign_problem_w g{gA, gT, nullptr, ids.data(), starts.data(), allowed.data(), nullptr, nullptr, 0, 2};
    Out og(gA);
    packAssignBatchWide(env, 1, &g, &og.r, 0, st);  // budget 0: memory rows, the wave writes the matrix into scratch
    CHECK(og.r.status == MRP_LL_OK);
    const as::AssignJobWide& gj = st.jobs[0];
    CHECK(gj.costOff == as::kNoCostOff && gj.taskOff == 0 && gj.agentOff == 65 && gj.words == 2 && gj.rowSource == as::kRowsMem);
    CHECK(st.data[0] == 128 && st.data.size() == 65 + 70 * 6);
    CHECK(st.scratchWords == 70 * 65 && gj.scratchOff == st.outWords && st.outWords == as::kOutHeadWords + 70 && st.ldsBytes == 0);
    const uint32_t* q = st.data.data() + gj.agentOff;
    CHECK(q[0] == as::kModeFree && q[1] == 0 && q[2] == 1 && q[3] == 0 && q[4] == 0 && q[5] == 0);
    CHECK(q[69 * 6 + 1] == (uint32_t)(2 * heurStride(env.maps[0]) + 3) && q[69 * 6 + 4] == 0xFFFFFFFFu && q[69 * 6 + 5] == 0xFFFFFFFFu);
  }

  {  // the row source at the budget's edge: a pure function of (nA, nT, budget)
    CHECK(as::rowSourceWide(128, 128, 65536) == as::kRowsLds && as::ldsBytesWide(128, 128, 65536) == 65536);
    CHECK(as::rowSourceWide(128, 128, 65535) == as::kRowsMem && as::ldsBytesWide(128, 128, 65535) == 0);
    CHECK(as::rowSourceWide(128, 129, 65536) == as::kRowsMem);  // a third word: 768-byte rows
    CHECK(as::rowSourceWide(85, 129, 65536) == as::kRowsLds && as::rowSourceWide(86, 129, 65536) == as::kRowsMem);
    CHECK(as::rowSourceWide(256, 64, 65536) == as::kRowsMem && as::rowSourceWide(64, 256, 65536) == as::kRowsLds);
    CHECK(as::rowSourceWide(256, 256, 65536) == as::kRowsMem && as::rowSourceWide(65, 65, 0) == as::kRowsMem);
    CHECK(as::rowSourceWide(65, 65, 65 * 512) == as::kRowsLds && as::rowSourceWide(65, 65, 65 * 512 - 1) == as::kRowsMem);
    CHECK(as::scratchWordsWide(65, 65, true, 0) == 65 * 65 && as::scratchWordsWide(65, 65, false, 0) == 0);
    CHECK(as::scratchWordsWide(65, 65, true, 65536) == 0 && as::wordsWide(0, 0) == 1 && as::wordsWide(64, 65) == 2);
    // two gather problems with memory rows: the scratch regions lie behind all result records, one after the other
    const std::vector<int32_t> ids(3, 0), starts(2 * 5, 0);
    const mrp_ll_assign_problem_w g{5, 3, nullptr, ids.data(), starts.data(), nullptr, nullptr, nullptr, 0, 1};
    const mrp_ll_assign_problem_w two[2] = {g, g};
    Out a(5), b(5);
    mrp_ll_assign_result res[2] = {a.r, b.r};
    AssignStagingWide st;
    packAssignBatchWide(env, 2, two, res, 0, st);
    CHECK(st.outWords == 2 * (as::kOutHeadWords + 5) && st.scratchWords == 30);
    CHECK(st.jobs[0].scratchOff == st.outWords && st.jobs[1].scratchOff == st.outWords + 15);
  }

  {  // a narrow series through the generalised code stages what it staged before: per child the 16 cost words, then per
     // agent (forbidden low, forbidden high, mode, 0); the children of the 4 x 4's optimum [3, 2, 1, 0] in index order
    const int32_t four[16] = {90, 76, 75, 80, 35, 85, 55, 65, 125, 95, 90, 105, 45, 110, 95, 115};
    const mrp_ll_assign_problem p{4, 4, four, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    Solvers sv;
    mrp_ll_assign_series* s = nullptr;
    CHECK(assignSeriesCreate(nullptr, 1, &p, &s, sv.narrow()) == MRP_LL_SUCCESS && s && !s->wide && s->maskWords == 1);
    Out o(4);
    CHECK(assignSeriesNext(1, &s, &o.r, sv.narrow()) == MRP_LL_SUCCESS);
    CHECK(o.r.status == MRP_LL_OK && o.r.cost == 275 && o.taskOf[0] == 3 && o.taskOf[1] == 2 && o.taskOf[2] == 1 && o.taskOf[3] == 0);
    CHECK(sv.narrowData.size() == 2 && sv.narrowJobs[1] == 4);
    std::vector<uint32_t> want;
    const int best[4] = {3, 2, 1, 0};
    for (int kid = 0; kid < 4; ++kid) {
      for (int k = 0; k < 16; ++k) want.push_back((uint32_t)four[k]);
      for (int a = 0; a < 4; ++a) {
        want.push_back(a == kid ? 1u << best[a] : 0u);
        want.push_back(0);
        want.push_back(a < kid ? (uint32_t)best[a] : as::kModeFree);
        want.push_back(0);
      }
    }
    CHECK(sv.narrowData[1] == want);
    delete s;  // (plain delete destroys a series)
  }

  {  // a narrow and a wide series in one step: one call of each solver; a wide child's forbidden bit beyond 63
    std::vector<int32_t> cost(2 * 130, MRP_LL_ASSIGN_NO_EDGE);
    cost[0 * 130 + 129] = 1, cost[0 * 130 + 64] = 2, cost[1 * 130 + 129] = 3, cost[1 * 130 + 5] = 9;
    const mrp_ll_assign_problem_w pw{2, 130, cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3};
    const int32_t small[2] = {2, 1};
    const mrp_ll_assign_problem pn{2, 1, small, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    Solvers sv;
    mrp_ll_assign_series* s[2] = {nullptr, nullptr};
    CHECK(assignSeriesCreateWide(nullptr, 1, &pw, &s[0], sv.wide()) == MRP_LL_SUCCESS && s[0]->wide && s[0]->maskWords == 3);
    CHECK(assignSeriesCreate(nullptr, 1, &pn, &s[1], sv.narrow()) == MRP_LL_SUCCESS);
    mrp_ll_assign_problem_w few = pw;
    few.mask_words = 2;  // a node's masks need a word for every task
    mrp_ll_assign_series* none = nullptr;
    CHECK(assignSeriesCreateWide(nullptr, 1, &few, &none, sv.wide()) == MRP_LL_E_INVALID && !none);
    Out a(2), b(2);
    mrp_ll_assign_result res[2] = {a.r, b.r};
    CHECK(assignSeriesNext(2, s, res, sv.narrow()) == MRP_LL_E_INVALID);  // a wide series needs the wide solver
    const size_t nw = sv.wideData.size(), nn = sv.narrowData.size();
    CHECK(assignSeriesNext(2, s, res, sv.narrow(), sv.wide()) == MRP_LL_SUCCESS);
    CHECK(sv.wideData.size() == nw + 1 && sv.narrowData.size() == nn + 1 && sv.wideJobs.back() == 2 && sv.narrowJobs.back() == 2);
    CHECK(res[0].status == MRP_LL_OK && res[0].matched == 2 && res[0].cost == 5 && a.taskOf[0] == 64 && a.taskOf[1] == 129);
    CHECK(res[1].status == MRP_LL_OK && res[1].cost == 1 && b.taskOf[0] == -1 && b.taskOf[1] == 0);
    // the first wide child forbids agent 0 its task 64: bit 0 of word 1
    const uint32_t* r = sv.wideData.back().data() + 2 * 130;
    CHECK(r[0] == as::kModeFree && r[2] == 0 && r[3] == 0 && r[4] == 1 && r[5] == 0 && r[6] == 0 && r[7] == 0);
    // the series go on: the wide one's other matchings of two pairs are {a0: 129, a1: 5} = 10 and {a0: 64, a1: 5} = 11
    CHECK(assignSeriesNext(2, s, res, sv.narrow(), sv.wide()) == MRP_LL_SUCCESS);
    CHECK(res[0].status == MRP_LL_OK && res[0].cost == 10 && a.taskOf[0] == 129 && a.taskOf[1] == 5);
    CHECK(res[1].status == MRP_LL_OK && res[1].cost == 2 && b.taskOf[0] == 0 && b.taskOf[1] == -1);
    CHECK(assignSeriesNext(2, s, res, sv.narrow(), sv.wide()) == MRP_LL_SUCCESS);
    CHECK(res[0].status == MRP_LL_OK && res[0].cost == 11 && a.taskOf[0] == 64 && a.taskOf[1] == 5);
    CHECK(res[1].status == MRP_LL_NO_SOLUTION && res[1].matched == 0);
    CHECK(assignSeriesNext(2, s, res, sv.narrow(), sv.wide()) == MRP_LL_SUCCESS);
    CHECK(res[0].status == MRP_LL_NO_SOLUTION && res[1].status == MRP_LL_NO_SOLUTION);
    delete s[0];
    delete s[1];
  }

  std::printf("assign_wide_host_check: ok\n");
  return 0;
}
