// What the rounds of the two task-assignment solvers (hl/ta_rounds.hpp; csrc/hl/mrp_hl_ta.cpp: CBS-TA, csrc/hl/mrp_hl_ecbs_ta.cpp:
// ECBS-TA) need around their trees: the engine context with its assignment series, the caller-side result buffers of a round,
// a result turned into a tree's path, and the set-up of a batch — maps, tasks, one launch for all shortest-path tables, one
// for all optima.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../include/mrp_hl.h"
#include "ta_tree_base.hpp"

// The engine's wide entry points (up to 256 agents and tasks).  Weak references, as mrp_hl_ecbs_ta.cpp's to the stored root
// call: an engine library without them still loads; an instance beyond 64 agents or tasks then ends MRP_HL_LL_ERROR, and a
// wide root without a wide root call is planned as ordinary jobs.
extern "C" int mrp_ll_assign_series_create_w(mrp_ll_ctx*, int32_t, const mrp_ll_assign_problem_w*, mrp_ll_assign_series**)
    __attribute__((weak));
extern "C" int mrp_ll_ta_root_batch_w(mrp_ll_ctx*, int32_t, const mrp_ll_ta_root*, int32_t*, mrp_ll_conflict*) __attribute__((weak));
extern "C" int mrp_ll_ta_eps_root_batch_w(mrp_ll_ctx*, float, int32_t, const mrp_ll_ta_root*, mrp_ll_conflict*, int32_t*)
    __attribute__((weak));

namespace mrp_hl {
namespace ta {

constexpr int32_t kPathCap = 512;  // the engine's default max_horizon: no path is longer

// The caller-side buffers of one round's results: states and action costs, kPathCap per search.
struct ResultPool {
  std::vector<int32_t> states, costs;
  void reserve(size_t n) {
    if (states.size() < n * kPathCap * 3) states.resize(n * kPathCap * 3);
    if (costs.size() < n * kPathCap) costs.resize(n * kPathCap);
  }
  void attach(mrp_ll_result& r, size_t k) {
    std::memset(&r, 0, sizeof(r));
    r.states_txy = states.data() + k * kPathCap * 3;
    r.action_costs = costs.data() + k * kPathCap;
    r.states_cap = kPathCap;
  }
};

// The MRP_HL_TA_* environment knobs of mrp_hl_solve_ecbs_ta_batch, read once per call (as solve_knobs.hpp's for the CBS / ECBS
// solver).
struct TaKnobs {
  // MRP_HL_TA_DEVICE_PATHS=1: every path stays in the engine's device-resident path store, in the slot its search was told
  // to leave it in, and a search whose conflict-tree node has every other agent's path there names them by slot instead of
  // shipping the focal table.  Same results; off by default.
  bool devicePaths = false;
  // MRP_HL_TA_PATH_SLOTS=N: slots of that store.  Unset (-1): four per agent over the batch's instances, between 256 and
  // 65536 (about 1 KB of device memory a slot) — room for every root and a few levels of children; not tuned.  (The trees
  // keep every node they made, so a tree's slots come back when a search leaves no path or the tree is destroyed.)  A tree
  // that finds the free list empty ships its contexts as without the knob.
  int32_t pathSlots = -1;
  static TaKnobs read() {
    TaKnobs k;
    if (const char* e = std::getenv("MRP_HL_TA_DEVICE_PATHS")) k.devicePaths = std::atoi(e) != 0;
    if (const char* e = std::getenv("MRP_HL_TA_PATH_SLOTS")) k.pathSlots = std::max(1, std::atoi(e));
    return k;
  }
  int32_t slotsFor(int64_t agentsOfTheBatch) const {
    if (pathSlots > 0) return pathSlots;
    return static_cast<int32_t>(std::min<int64_t>(65536, std::max<int64_t>(256, 4 * agentsOfTheBatch)));
  }
};

// The free list of the path store's slots.  A slot lives and dies with its path: it is taken when the search that will
// produce the path is issued, belongs to the Path made of that search's result (pathOf below: the deleter gives it back
// when the last PathP drops), and comes straight back when the search leaves no path.
// Why a freed slot can be handed out at once: the driver's engine calls are synchronous — a call returns when every search
// of the round has ended — and paths are dropped only between calls, while the trees consume a round's results.  So no
// job in flight names a slot on this list; a slot freed in round r is at the earliest written by a search of round r + 1.
// Inside one batch a slot is written by the one search it was handed to and read only by jobs whose node holds its Path:
// never both, since a slot on the list belongs to no Path.
struct PathSlots {
  std::vector<int32_t> free;
  void reset(int32_t n) {
    free.resize(static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) free[i] = n - 1 - i;
  }
  int32_t take() {
    if (free.empty()) return -1;
    const int32_t s = free.back();
    free.pop_back();
    return s;
  }
  void give(int32_t s) {
    if (s >= 0) free.push_back(s);
  }
};
typedef std::shared_ptr<PathSlots> PathSlotsP;

// slot >= 0: the search also left the path in that slot of `slots`' store.
inline PathP pathOf(const mrp_ll_result& r, int32_t slot = -1, const PathSlotsP& slots = PathSlotsP()) {
  std::shared_ptr<Path> p;
  if (slot >= 0 && slots) {
    p = std::shared_ptr<Path>(new Path(), [slots](Path* q) {
      slots->give(q->slot);
      delete q;
    });
    p->slot = slot;
  } else {
    p = std::make_shared<Path>();
  }
  p->cost = r.cost;
  int32_t g = 0;
  for (int k = 0; k < r.n_states; ++k) {
    p->xy.push_back(r.states_txy[3 * k + 1]);
    p->xy.push_back(r.states_txy[3 * k + 2]);
    p->g.push_back(g);
    if (k + 1 < r.n_states) g += r.action_costs[k];
  }
  return p;
}

struct Engine {
  mrp_ll_ctx* ctx = nullptr;
  std::vector<mrp_ll_assign_series*> series;
  ~Engine() {
    for (mrp_ll_assign_series* s : series)
      if (s) mrp_ll_assign_series_destroy(s);
    if (ctx) mrp_ll_destroy(ctx);
  }
};

constexpr int32_t kNarrowLimit = 64;   // agents and tasks of mrp_ll_assign_series_create and of the narrow root calls
constexpr int32_t kWideLimit = 256;    // ... of mrp_ll_assign_series_create_w and of the _w root calls

// Makes trees[k] (TreeT: ta::Tree or ecbs_ta::Tree) and fills its base from inst[k]; an instance beyond the limits — 256
// agents or 256 distinct potential goals, 64 of each with an engine that has no mrp_ll_assign_series_create_w — ends
// MRP_HL_LL_ERROR.
// The instances within 64 x 64 share ONE mrp_ll_assign_series_create, the others ONE mrp_ll_assign_series_create_w, which is
// called only when there are such instances.  Returns MRP_LL_SUCCESS or the engine's error.
template <typename TreeT>
int setUpBatch(Engine& eng, int32_t n, const mrp_hl_ta_instance* inst, std::vector<std::unique_ptr<TreeT>>& trees) {
  typedef TreeBase Tree;
  int rc = MRP_LL_SUCCESS;
  const int32_t limit = &mrp_ll_assign_series_create_w != nullptr ? kWideLimit : kNarrowLimit;
  // ---- the instances: maps, tasks, one launch for all tables, one for all optima
  trees.clear();
  trees.resize(static_cast<size_t>(n));
  std::vector<int32_t> tabMap, tabGoal;
  for (int32_t k = 0; k < n; ++k) {
    const mrp_hl_ta_instance& I = inst[k];
    trees[k].reset(new TreeT());
    Tree& t = *trees[k];
    t.nAgents = I.n_agents;
    if (I.n_agents < 1 || I.n_agents > limit || !I.starts_xy || !I.goal_first || (I.goal_first[I.n_agents] > 0 && !I.goals_xy) ||
        mrp_ll_upload_map(eng.ctx, I.dimx, I.dimy, I.n_obstacles, I.obstacles_xy, &t.mapId) != MRP_LL_SUCCESS) {
      t.nAgents = I.n_agents > 0 && I.n_agents <= limit ? I.n_agents : 0;
      t.end(MRP_HL_LL_ERROR);
      continue;
    }
    t.starts.assign(I.starts_xy, I.starts_xy + 2 * I.n_agents);
    std::vector<std::vector<int32_t>> tasksOf(static_cast<size_t>(I.n_agents));  // per agent: the tasks it may take
    bool tooMany = false;
    for (int a = 0; a < I.n_agents && !tooMany; ++a) {
      if (t.starts[2 * a] < 0 || t.starts[2 * a] >= I.dimx || t.starts[2 * a + 1] < 0 || t.starts[2 * a + 1] >= I.dimy) tooMany = true;
      for (int q = I.goal_first[a]; q < I.goal_first[a + 1]; ++q) {
        const int32_t gx = I.goals_xy[2 * q], gy = I.goals_xy[2 * q + 1];
        if (gx < 0 || gx >= I.dimx || gy < 0 || gy >= I.dimy) continue;  // can never be assigned
        size_t task = 0;
        while (task < t.taskXY.size() / 2 && !(t.taskXY[2 * task] == gx && t.taskXY[2 * task + 1] == gy)) ++task;
        if (task == t.taskXY.size() / 2) t.taskXY.insert(t.taskXY.end(), {gx, gy});
        if (task >= static_cast<size_t>(limit)) {
          tooMany = true;
          break;
        }
        tasksOf[a].push_back(static_cast<int32_t>(task));
      }
    }
    if (tooMany) {
      t.end(MRP_HL_LL_ERROR);
      continue;
    }
    // the masks as mrp_ll_assign_problem_w lays them out: bit task % 64 of the agent's word task / 64
    t.maskWords = std::max<int32_t>(1, static_cast<int32_t>((t.taskXY.size() / 2 + 63) / 64));
    t.allowed.assign(static_cast<size_t>(I.n_agents) * t.maskWords, 0);
    for (int a = 0; a < I.n_agents; ++a)
      for (int32_t task : tasksOf[a]) t.allowed[static_cast<size_t>(a) * t.maskWords + task / 64] |= 1ull << (task % 64);
    for (size_t task = 0; task < t.taskXY.size() / 2; ++task) {
      tabMap.push_back(t.mapId);
      tabGoal.insert(tabGoal.end(), {t.taskXY[2 * task], t.taskXY[2 * task + 1]});
    }
  }
  std::vector<int32_t> tabIds(tabMap.size() + 1, -1);
  rc = mrp_ll_compute_heuristics(eng.ctx, static_cast<int32_t>(tabMap.size()), tabMap.data(), tabGoal.data(), tabIds.data());
  if (rc != MRP_LL_SUCCESS) return rc;
  {
    std::vector<mrp_ll_assign_problem> probs;
    std::vector<mrp_ll_assign_problem_w> probsWide;
    std::vector<int32_t> treeOf, treeOfWide;
    size_t next = 0;
    for (int32_t k = 0; k < n; ++k) {
      Tree& t = *trees[k];
      if (!t.running()) continue;
      t.taskHeur.assign(tabIds.begin() + next, tabIds.begin() + next + t.taskXY.size() / 2);
      next += t.taskXY.size() / 2;
      if (t.nAgents <= kNarrowLimit && t.taskHeur.size() <= static_cast<size_t>(kNarrowLimit)) {  // (one mask word)
        mrp_ll_assign_problem p;
        std::memset(&p, 0, sizeof(p));
        p.n_agents = t.nAgents;
        p.n_tasks = static_cast<int32_t>(t.taskHeur.size());
        p.heuristic_ids = t.taskHeur.data();
        p.starts_xy = t.starts.data();
        p.allowed = t.allowed.data();
        probs.push_back(p);
        treeOf.push_back(k);
      } else {
        mrp_ll_assign_problem_w p;
        std::memset(&p, 0, sizeof(p));
        p.n_agents = t.nAgents;
        p.n_tasks = static_cast<int32_t>(t.taskHeur.size());
        p.heuristic_ids = t.taskHeur.data();
        p.starts_xy = t.starts.data();
        p.allowed = t.allowed.data();
        p.mask_words = t.maskWords;
        probsWide.push_back(p);
        treeOfWide.push_back(k);
      }
    }
    eng.series.assign(static_cast<size_t>(n), nullptr);
    std::vector<mrp_ll_assign_series*> made(probs.size() + 1, nullptr);
    rc = mrp_ll_assign_series_create(eng.ctx, static_cast<int32_t>(probs.size()), probs.data(), made.data());
    if (rc != MRP_LL_SUCCESS) return rc;
    for (size_t q = 0; q < treeOf.size(); ++q) eng.series[treeOf[q]] = made[q];
    if (!probsWide.empty()) {  // (only with an engine that has the call: `limit` above)
      std::vector<mrp_ll_assign_series*> madeWide(probsWide.size() + 1, nullptr);
      rc = mrp_ll_assign_series_create_w(eng.ctx, static_cast<int32_t>(probsWide.size()), probsWide.data(), madeWide.data());
      for (size_t q = 0; q < treeOfWide.size(); ++q) eng.series[treeOfWide[q]] = madeWide[q];  // (the Engine destroys what was made)
      if (rc != MRP_LL_SUCCESS) return rc;
    }
  }
  return MRP_LL_SUCCESS;
}

// The caller-side task_of buffers of one mrp_ll_assign_series_next over `count` series: a stride that holds any instance.
inline std::vector<int32_t> taskOfBuffers(size_t count, std::vector<mrp_ll_assign_result>& res) {
  std::vector<int32_t> taskOf(count * static_cast<size_t>(kWideLimit), -1);
  res.resize(count);
  for (size_t q = 0; q < count; ++q) {
    std::memset(&res[q], 0, sizeof(res[q]));
    res[q].task_of = taskOf.data() + q * static_cast<size_t>(kWideLimit);
  }
  return taskOf;
}

}  // namespace ta
}  // namespace mrp_hl
