// TEST INFRASTRUCTURE — stand-alone program: the two task-assignment drivers (csrc/hl/mrp_hl_ta.cpp, csrc/hl/mrp_hl_ecbs_ta.cpp
// over the rounds of csrc/hl/ta_rounds.hpp) on the stand-in engines, for a run under the host sanitizers.  They watch the
// lifetimes the round loop depends on: the mrp_ll_result records' pointers into the ResultPool, the mrp_ll_ta_root records'
// into the round's goal and heuristic vectors, the focal contexts that the mrp_ll_job records point into, and the Path deleters
// that hand their slots back to the shared free list.  Built and run by tests/test_ta_driver_sanitize_cpu.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DMOCK_TA_WIDE_BASE='"mock_ll_ta_eps_store.cpp"'
//       ta_driver_sanitize_main.cpp csrc/hl/mrp_hl.cpp csrc/hl/mrp_hl_ta.cpp csrc/hl/mrp_hl_ecbs_ta.cpp mock_ll_ta_eps_wide.cpp
//       mock_ll_ta_assign.cpp mock_ll_ta_assign_wide.cpp ecbs_ta_check.cpp -Wl,--wrap=mrp_ll_search_batch -loracle
// One batch: twelve seeded 8 x 8 instances of 3 .. 6 agents that share their potential goals (trees expand and take second
// roots), the two instances without a reachable goal of tests/test_cbs_ta_driver_cpu.py, one instance of 65 agents.  Solved by
// mrp_hl_solve_cbs_ta_batch and by mrp_hl_solve_ecbs_ta_batch (w = 1.0 and 1.3) with use_root_kernel 0 and 1, ECBS-TA once more under
// MRP_HL_TA_DEVICE_PATHS=1 with MRP_HL_TA_PATH_SLOTS=8 (the free list runs empty: contexts fall back to shipping).
// Exit status 0: the two root forms agree field by field, the knob changes no answer, the batch reached what it is for.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "mrp_hl.h"

namespace {

uint64_t g_seed = 20241021;
uint32_t rnd(uint32_t n) {  // [0, n)
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_seed >> 33) % n);
}

struct Instance {
  int32_t dimx = 0, dimy = 0;
  std::vector<int32_t> obst, starts, goalFirst, goals;
  int nAgents() const { return (int)starts.size() / 2; }
  mrp_hl_ta_instance record() const {
    mrp_hl_ta_instance r;
    r.dimx = dimx;
    r.dimy = dimy;
    r.n_obstacles = (int32_t)obst.size() / 2;
    r.obstacles_xy = obst.data();
    r.n_agents = nAgents();
    r.starts_xy = starts.data();
    r.goal_first = goalFirst.data();
    r.goals_xy = goals.data();
    return r;
  }
};

// `goalsOf[a]`: agent a's potential goals
Instance instanceOf(int dimx, int dimy, const std::vector<std::pair<int, int>>& obst, const std::vector<std::pair<int, int>>& starts,
                    const std::vector<std::vector<std::pair<int, int>>>& goalsOf) {
  Instance I;
  I.dimx = dimx;
  I.dimy = dimy;
  for (const auto& o : obst) I.obst.insert(I.obst.end(), {o.first, o.second});
  for (const auto& s : starts) I.starts.insert(I.starts.end(), {s.first, s.second});
  I.goalFirst.push_back(0);
  for (const auto& g : goalsOf) {
    for (const auto& c : g) I.goals.insert(I.goals.end(), {c.first, c.second});
    I.goalFirst.push_back((int32_t)I.goals.size() / 2);
  }
  I.obst.insert(I.obst.end(), {0, 0});  // (never read past n_obstacles; keeps data() non-null)
  I.goals.insert(I.goals.end(), {0, 0});
  return I;
}

// 8 x 8, 3 .. 6 agents; every agent may take one to three cells of ONE pool of n - 1 .. n + 1 goals (which may be start cells)
Instance seeded() {
  const int n = 3 + (int)rnd(4);
  std::set<std::pair<int, int>> blocked, taken;
  auto fresh = [&](std::set<std::pair<int, int>>& among) {
    for (;;) {
      const std::pair<int, int> c((int)rnd(8), (int)rnd(8));
      if (!blocked.count(c) && among.insert(c).second) return c;
    }
  };
  std::vector<std::pair<int, int>> obst, starts, pool;
  for (int i = 0; i < 12; ++i) obst.push_back(fresh(blocked));
  for (int a = 0; a < n; ++a) starts.push_back(fresh(taken));
  taken.clear();
  for (int g = 0; g < n - 1 + (int)rnd(3); ++g) pool.push_back(fresh(taken));
  std::vector<std::vector<std::pair<int, int>>> goalsOf((size_t)n);
  for (int a = 0; a < n; ++a)
    for (int g = 0; g < 1 + (int)rnd(3); ++g) goalsOf[(size_t)a].push_back(pool[rnd((uint32_t)pool.size())]);
  return instanceOf(8, 8, obst, starts, goalsOf);
}

struct Answer {
  mrp_hl_ta_solution s;
  std::vector<int32_t> taskXY, pathLen, paths;
};
const int kPathCap = 64;

bool same(const Answer& a, const Answer& b) {
  return a.s.status == b.s.status && a.s.n_ll_searches == b.s.n_ll_searches && a.s.cost == b.s.cost && a.s.makespan == b.s.makespan &&
         a.s.high_level_expanded == b.s.high_level_expanded && a.s.low_level_expanded == b.s.low_level_expanded &&
         a.s.num_task_assignments == b.s.num_task_assignments && a.s.n_roots == b.s.n_roots && a.s.root_conflicts == b.s.root_conflicts &&
         a.s.n_root_searches == b.s.n_root_searches && a.s.schedule_digest == b.s.schedule_digest && a.taskXY == b.taskXY &&
         a.pathLen == b.pathLen && a.paths == b.paths;
}

// w == 0: CBS-TA, else ECBS-TA at w
bool solve(float w, int useRootKernel, const std::vector<Instance>& insts, std::vector<Answer>& out, mrp_hl_batch_stats& stats) {
  std::vector<mrp_hl_ta_instance> recs;
  for (const Instance& I : insts) recs.push_back(I.record());
  out.assign(insts.size(), Answer());
  std::vector<mrp_hl_ta_solution> sols(insts.size());
  for (size_t k = 0; k < insts.size(); ++k) {
    const size_t n = (size_t)insts[k].nAgents();
    out[k].taskXY.assign(2 * n, -7);
    out[k].pathLen.assign(n, -7);
    out[k].paths.assign(n * kPathCap * 3, -7);
    mrp_hl_ta_solution& s = sols[k];
    s = mrp_hl_ta_solution();
    s.task_xy = out[k].taskXY.data();
    s.path_len = out[k].pathLen.data();
    s.paths_xyt = out[k].paths.data();
    s.path_cap = kPathCap;
  }
  mrp_hl_ta_options opt;
  opt.max_task_assignments = 1 << 30;
  opt.use_root_kernel = useRootKernel;
  opt.max_hl_expansions = 300;  // (a bound on the run; the counters of both root forms agree under it)
  opt.max_ll_expansions = -1;
  const int32_t n = (int32_t)insts.size();
  const int rc = w == 0.0f ? mrp_hl_solve_cbs_ta_batch(0, &opt, n, recs.data(), sols.data(), &stats)
                           : mrp_hl_solve_ecbs_ta_batch(0, w, &opt, n, recs.data(), sols.data(), &stats);
  for (size_t k = 0; k < insts.size(); ++k) out[k].s = sols[k];
  return rc == MRP_LL_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) g_seed = std::strtoull(argv[1], nullptr, 10);  // (to look for another seed; the test runs the default)
  std::vector<Instance> insts;
  for (int k = 0; k < 12; ++k) insts.push_back(seeded());
  // no goal that anybody can reach: a walled-in goal, a goal on an obstacle, a goal outside the grid; and no goal at all
  insts.push_back(instanceOf(5, 5, {{3, 4}, {4, 3}}, {{0, 0}, {1, 1}}, {{{4, 4}}, {{4, 4}, {3, 4}, {9, 9}}}));
  insts.push_back(instanceOf(4, 4, {}, {{0, 0}, {1, 1}}, {{}, {}}));
  {  // 65 agents on an open 32 x 32 map, each with the one goal sixteen rows below it
    std::vector<std::pair<int, int>> starts;
    std::vector<std::vector<std::pair<int, int>>> goalsOf;
    for (int a = 0; a < 65; ++a) {
      starts.push_back({a % 32, a / 32});
      goalsOf.push_back({{a % 32, 16 + a / 32}});
    }
    insts.push_back(instanceOf(32, 32, {}, starts, goalsOf));
  }
  int bad = 0;
  // ECBS-TA at w = 1.0 takes second roots (any child dearer than the root's bound asks for one), at 1.3 its focal list matters
  const char* names[3] = {"cbs_ta", "ecbs_ta w 1.0", "ecbs_ta w 1.3"};
  const float ws[3] = {0.0f, 1.0f, 1.3f};
  for (int algo = 0; algo < 3; ++algo) {
    std::vector<Answer> first;
    for (int knob = 0; knob <= (algo > 0 ? 1 : 0); ++knob) {  // (the knob is ECBS-TA's)
      if (knob) {
        setenv("MRP_HL_TA_DEVICE_PATHS", "1", 1);
        setenv("MRP_HL_TA_PATH_SLOTS", "8", 1);
      }
      for (int useRootKernel = 0; useRootKernel < 2; ++useRootKernel) {
        std::vector<Answer> got;
        mrp_hl_batch_stats stats;
        if (!solve(ws[algo], useRootKernel, insts, got, stats)) {
          std::printf("%s use_root_kernel %d knob %d: the call failed\n", names[algo], useRootKernel, knob);
          return 1;
        }
        if (first.empty()) first = got;
        int secondRoots = 0, expanded = 0, solved = 0;
        for (size_t k = 0; k < insts.size(); ++k) {
          if (!same(got[k], first[k])) {
            bad += 1;
            std::printf("%s use_root_kernel %d knob %d: instance %d differs (status %d against %d, cost %ld against %ld)\n", names[algo],
                        useRootKernel, knob, (int)k, got[k].s.status, first[k].s.status, (long)got[k].s.cost, (long)first[k].s.cost);
          }
          secondRoots += got[k].s.n_roots >= 2 ? 1 : 0;
          expanded += got[k].s.high_level_expanded >= 2 ? 1 : 0;
          solved += got[k].s.status == MRP_HL_SOLVED ? 1 : 0;
        }
        std::printf("%s use_root_kernel %d knob %d: %d instances, %d solved, %d with children, %d with a second root, %ld rounds\n",
                    names[algo], useRootKernel, knob, (int)insts.size(), solved, expanded, secondRoots, (long)stats.rounds);
        // what the seed was chosen to reach; the wide instance and the two without a goal end as they must
        const int wantNoGoal = algo == 0 ? MRP_HL_NO_SOLUTION : MRP_HL_SOLVED;  // (ECBS-TA plans a first root without tasks)
        if (expanded < 2 || secondRoots < (algo < 2 ? 2 : 0) || got[14].s.status != MRP_HL_SOLVED || got[12].s.status != wantNoGoal ||
            got[13].s.status != wantNoGoal) {
          std::printf("ta_driver_sanitize: the batch no longer reaches what it is for\n");
          bad += 1;
        }
      }
      unsetenv("MRP_HL_TA_DEVICE_PATHS");
      unsetenv("MRP_HL_TA_PATH_SLOTS");
    }
  }
  std::printf("ta_driver_sanitize: %d wrong\n", bad);
  return bad != 0 ? 1 : 0;
}
