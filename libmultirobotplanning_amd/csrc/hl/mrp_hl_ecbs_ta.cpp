// mrp_hl_solve_ecbs_ta_batch (include/mrp_hl.h): ECBS with task assignment for a batch of instances, in the rounds of
// hl/ta_rounds.hpp over hl/ecbs_ta_tree.hpp's state machines.  What is ECBS-TA's own in a round:
//   the root call      mrp_ll_ta_eps_root_batch for the new roots of at most 64 agents, one workgroup each, and
//                      mrp_ll_ta_eps_root_batch_w for the others; the tree takes the call's scan and count
//   a root as jobs     n DEPENDENT searches, one agent per round, each with the paths of the agents before it as its shipped
//                      focal context; the tree scans and counts itself
//   the children       two MRP_LL_ASTAR_EPS_TA searches with the node's paths as the context; the trees scan and count their
//                      children's conflicts themselves
//   fmin               of every search that left a path, for the tree's lower bounds
// MRP_HL_TA_DEVICE_PATHS=1 (ta_batch_setup.hpp TaKnobs; off by default, same results): the engine's path store is reserved,
// every search is told to leave its path in a slot of it (a root through mrp_ll_ta_eps_root_batch_stored), and a job whose
// node has every other agent's path there goes out with path_ids instead of a shipped table.  Instances of more than 64
// agents ignore the knob: their contexts ship, their searches store nothing and their roots go through the unstored call.
// MRP_HL_TA_EPS_LDS=1 (solve_knobs.hpp TaEpsKnobs; off by default, same results): the jobs of call 3 carry MRP_LL_JOB_TRY_LDS.
// A translation unit of its own, like csrc/hl/mrp_hl_ta.cpp.
#include <deque>

#include "../../../include/mrp_hl.h"
#include "ecbs_ta_tree.hpp"
#include "solve_knobs.hpp"
#include "ta_rounds.hpp"

// The engine's entry point for roots that leave their paths in the store.  A weak reference: an engine library without it
// still loads, and MRP_HL_TA_DEVICE_PATHS then sends its roots through the plain call, their paths unstored.
extern "C" int mrp_ll_ta_eps_root_batch_stored(mrp_ll_ctx*, float, int32_t, const mrp_ll_ta_root*, mrp_ll_conflict*, int32_t*,
                                               const int32_t* const*) __attribute__((weak));

namespace {

using mrp_hl::ta::Cons;
using mrp_hl::ta::Engine;
using mrp_hl::ta::kPathCap;
using mrp_hl::ta::PathP;
using mrp_hl::ta::pathOf;
using mrp_hl::ta::PathSlots;
using mrp_hl::ta::PathSlotsP;

// The focal context of one job: the solution vector the search sees (its own entry is ignored, an empty path is skipped).
struct Context {
  std::vector<int32_t> len, ids;  // ids: the paths' slots in the path store, -1: not there (or no path)
  std::vector<const int32_t*> xy;
  void of(const std::vector<PathP>& sol) {
    static const int32_t none[2] = {0, 0};
    len.assign(sol.size(), 0);
    ids.assign(sol.size(), -1);
    xy.assign(sol.size(), none);
    for (size_t a = 0; a < sol.size(); ++a)
      if (sol[a]) {
        len[a] = sol[a]->len();
        ids[a] = sol[a]->slot;
        xy[a] = sol[a]->xy.data();
      }
  }
  // The context of `agent`'s search can go by slot: some other agent has a path, and each of those paths is in the store.
  // (Asked for trees of at most 64 agents only — the table the workgroup then builds fits: 64 agents x kPathCap 512 states
  // x 2 bytes = 64 KiB of the default engine's 128 KiB path area.  256 agents x 512 states do not, so wider trees ship.)
  bool byId(int agent) const {
    bool any = false;
    for (size_t a = 0; a < len.size(); ++a) {
      if (static_cast<int>(a) == agent || len[a] <= 0) continue;
      if (ids[a] < 0) return false;
      any = true;
    }
    return any;
  }
};

struct EcbsTa {
  typedef mrp_hl::ecbs_ta::Tree Tree;
  float w = 1.0f;
  bool tryLds = false;  // MRP_HL_TA_EPS_LDS: the jobs start in the LDS tier
  PathSlotsP slots;     // MRP_HL_TA_DEVICE_PATHS: the store's free list (null: the knob is off)
  // of the round
  const mrp_ll_result* res = nullptr;
  std::vector<int32_t> outSlot;  // the slot result q's search was told to leave its path in (-1: none); path() takes it
  std::deque<Context> ctx;       // what the round's jobs point into

  static bool wideRootCall() { return &mrp_ll_ta_eps_root_batch_w != nullptr; }
  int setUp(Engine& eng, const std::vector<std::unique_ptr<Tree>>& trees) {
    for (const auto& t : trees) t->w = w;
    tryLds = mrp_hl::TaEpsKnobs::read().tryLds;
    const mrp_hl::ta::TaKnobs knobs = mrp_hl::ta::TaKnobs::read();
    if (!knobs.devicePaths) return MRP_LL_SUCCESS;
    int64_t agents = 0;
    for (const auto& t : trees) agents += t->running() && t->nAgents <= mrp_hl::ta::kNarrowLimit ? t->nAgents : 0;
    const int32_t nSlots = knobs.slotsFor(agents);
    const int rc = mrp_ll_path_store_reserve(eng.ctx, nSlots);
    if (rc != MRP_LL_SUCCESS) return rc;
    slots = std::make_shared<PathSlots>();
    slots->reset(nSlots);
    return MRP_LL_SUCCESS;
  }
  // Only trees of at most 64 agents keep paths in the store (Context::byId).
  bool stores(const Tree& t) const { return slots && t.nAgents <= mrp_hl::ta::kNarrowLimit; }
  void beginRound(const mrp_ll_result* results, size_t nResults) {
    res = results;
    outSlot.assign(nResults + 1, -1);
    ctx.clear();
  }
  void endRound() {
    for (int32_t s : outSlot)  // a search that left no path, or whose tree had ended: its slot is free again
      if (s >= 0) slots->give(s);
  }
  int rootCall(mrp_ll_ctx* c, bool wide, int32_t m, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* scan) {
    if (wide) return mrp_ll_ta_eps_root_batch_w(c, w, m, roots, scan, planned);
    if (!slots || &mrp_ll_ta_eps_root_batch_stored == nullptr) return mrp_ll_ta_eps_root_batch(c, w, m, roots, scan, planned);
    std::vector<std::vector<int32_t>> ids(static_cast<size_t>(m));
    std::vector<const int32_t*> idsOf(static_cast<size_t>(m));
    for (int32_t i = 0; i < m; ++i) {  // (narrow roots: stores() holds for every one of them)
      for (int32_t a = 0; a < roots[i].n_agents; ++a) {
        const size_t q = static_cast<size_t>(roots[i].results - res) + static_cast<size_t>(a);
        ids[i].push_back(outSlot[q] = slots->take());
      }
      idsOf[i] = ids[i].data();
    }
    return mrp_ll_ta_eps_root_batch_stored(c, w, m, roots, scan, planned, idsOf.data());
  }
  // `agent`'s search for `task` against the paths of `c`; its result is number q
  void job(std::vector<mrp_ll_job>& jobs, const Tree& t, int agent, int32_t task, const Cons* cons, const Context& c, int64_t budget,
           size_t q) {
    jobs.emplace_back();
    mrp_ll_job& j = jobs.back();
    mrp_hl::ta::fillJob(j, t, MRP_LL_ASTAR_EPS_TA, t.w, agent, task, cons, budget);
    j.agent_idx = agent;
    j.n_agents = static_cast<int32_t>(c.len.size());
    j.path_len = c.len.data();
    if (stores(t) && c.byId(agent))  // the context goes by slot, nothing is shipped
      j.path_ids = c.ids.data();
    else
      j.path_xy = c.xy.data();
    if (stores(t)) outSlot[q] = slots->take();
    if (outSlot[q] >= 0) {  // the search also leaves its path there
      j.result_path_id = outSlot[q];
      j.flags |= MRP_LL_JOB_STORE_RESULT;
    }
    if (tryLds) j.flags |= MRP_LL_JOB_TRY_LDS;
  }
  size_t rootJobsOf(const Tree&) { return 1; }
  void rootJobs(const Tree& t, int64_t budget, size_t first, std::vector<mrp_ll_job>& jobs) {
    ctx.emplace_back();
    ctx.back().of(t.rootPaths);
    job(jobs, t, t.rootAgent, t.rootTasks[t.rootAgent], nullptr, ctx.back(), budget, first);
  }
  void childJobs(const Tree& t, int64_t budget, size_t first, std::vector<mrp_ll_job>& jobs) {
    ctx.emplace_back();
    ctx.back().of(t.nodes[t.popped].sol);
    const std::vector<int32_t>& taskOf = t.nodes[t.popped].taskOf;
    for (int s = 0; s < 2; ++s)
      job(jobs, t, t.childAgent[s], taskOf[t.childAgent[s]], t.childCons[s].get(), ctx.back(), budget, first + static_cast<size_t>(s));
  }
  PathP path(const mrp_ll_result& r, size_t q) {
    int32_t s = outSlot[q];
    outSlot[q] = -1;
    if (s >= 0 && r.n_states >= kPathCap) {  // as long as a slot: the device did not store it (mrp_ll.h)
      slots->give(s);
      s = -1;
    }
    return pathOf(r, s, slots);
  }
  void gotRoot(Tree& t, bool viaCall, const std::vector<PathP>& paths, const mrp_ll_result* r, int done, bool all, const mrp_ll_conflict& scan) {
    if (!viaCall) {
      t.gotRootSearch(paths[0], r[0].fmin);  // (the one search of this round is t.rootAgent's)
      return;
    }
    if (all && done != t.nAgents) {
      t.end(MRP_HL_LL_ERROR);  // (the call completes every root it accepts: a refused one)
      return;
    }
    std::vector<int32_t> fmin(static_cast<size_t>(t.nAgents), 0);
    for (int a = 0; a < done; ++a)
      if (paths[a]) fmin[a] = r[a].fmin;
    t.gotRoot(paths, fmin, done, scan);
  }
  void gotChildren(Tree& t, const PathP path[2], const mrp_ll_result* r) {
    const int32_t fmin[2] = {path[0] ? r[0].fmin : 0, path[1] ? r[1].fmin : 0};
    t.gotChildren(path, fmin);
  }
};

}  // namespace

extern "C" int mrp_hl_solve_ecbs_ta_batch(int32_t device, float w, const mrp_hl_ta_options* opt, int32_t n,
                                          const mrp_hl_ta_instance* inst, mrp_hl_ta_solution* sols, mrp_hl_batch_stats* stats) {
  if (!(w >= 1.0f)) return MRP_LL_E_INVALID;
  EcbsTa algo;
  algo.w = w;
  return mrp_hl::ta::solveTaBatch(algo, device, opt, n, inst, sols, stats);
}
