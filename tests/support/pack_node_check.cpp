// TEST INFRASTRUCTURE — a stand-alone check of how the engine's packer (libmultirobotplanning_amd/csrc/host/ll_pack.h) takes
// MRP_LL_JOB_SCAN_FROM_PARENT jobs (mrp_ll_submit_node), built by tests/test_node_scan_parent_cpu.py with the host sanitizers
// and run as a program of its own, beside pack_check.cpp: every rejection include/mrp_ll.h lists, with no constraint set
// created, and the words of an accepted job — the focal context has no column for agent_idx, the replaced path's slot and
// the two integers stand BEHIND the context's ids.  Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../libmultirobotplanning_amd/csrc/host/ll_pack.h"

using namespace mrp::host;
using mrp::DevJob;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "pack_node_check: line %d: %s\n", __LINE__, #cond);         \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

namespace {

PackEnv makeEnv() {  // one 8 x 8 map, a path store of 8 slots, no session
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{8, 8, 2, 0});
  env.maxHorizon = 64;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 128 * 1024;
  env.pathStoreSlots = 8;
  return env;
}

struct Node {  // three agents, agent 1 searches; its replaced path is in slot 5
  int32_t ids[3] = {2, 5, 3};
  int32_t len[3] = {4, 3, 2};
  mrp_ll_scan_base base{7, 2};
  mrp_ll_job job;
  Node() {
    std::memset(&job, 0, sizeof(job));
    job.algo = MRP_LL_ASTAR_EPS;
    job.w = 1.5f;
    job.goal_x = 3;
    job.goal_y = 2;
    job.max_expansions = -1;
    job.result_path_id = -1;
    job.n_agents = 3;
    job.agent_idx = 1;
    job.path_ids = ids;
    job.path_len = len;
    job.flags = MRP_LL_JOB_SCAN_CONFLICTS | MRP_LL_JOB_SCAN_FROM_PARENT;
  }
  PackArgs args() const { return PackArgs{true, nullptr, &base}; }
};

struct Packed {
  bool ok;
  DevJob d;
  PendingSet pending;
  uint32_t used;
  std::unique_ptr<uint32_t[]> cons;
};
Packed pack(const PackEnv& env, const mrp_ll_job& j, const PackArgs& args) {
  Packed p;
  p.cons.reset(new uint32_t[kSlotConsWords]);  // exactly a job slot's capacity: the sanitizer sees a word past it
  std::unique_ptr<uint16_t[]> paths(new uint16_t[kSlotPathHalfs]);
  ConsSinkSlot cs{p.cons.get(), 0, kSlotConsWords};
  PathSinkSlot ps{paths.get(), 0, kSlotPathHalfs};
  p.ok = packJob(env, j, args, cs, ps, p.d, p.pending);
  p.used = cs.used;
  return p;
}
bool rejected(const PackEnv& env, const mrp_ll_job& j, const PackArgs& args) {
  const Packed p = pack(env, j, args);
  return !p.ok && p.pending.slot == -1;
}

}  // namespace

int main() {
  const PackEnv env = makeEnv();
  {  // accepted: the ids without the searching agent's, then slot, parent_count, clean_before
    Node n;
    const Packed p = pack(env, n.job, n.args());
    CHECK(p.ok);
    CHECK((p.d.ctx_flags & (mrp::kCtxById | mrp::kCtxScan | mrp::kCtxScanParent)) == (mrp::kCtxById | mrp::kCtxScan | mrp::kCtxScanParent));
    CHECK(p.d.n_ctx == 3 && p.d.t_pad == 4 && p.d.n_agents_pad == 16 && p.d.reserved == 1);
    CHECK(p.used == 6 && p.d.path_off == 0);
    const uint32_t want[6] = {2, mrp::kNoStoreSlot, 3, 5, 7, 2};
    CHECK(std::memcmp(p.cons.get(), want, sizeof(want)) == 0);
    // the replaced path the longest of the node: still no row, no column for it
    n.len[1] = 40;
    const Packed q = pack(env, n.job, n.args());
    CHECK(q.ok && q.d.t_pad == 4 && q.cons[1] == mrp::kNoStoreSlot && q.cons[3] == 5);
  }
  {  // the same job without the new flag: nothing behind the ids, whatever bases[i] holds
    Node n;
    n.job.flags = MRP_LL_JOB_SCAN_CONFLICTS;
    n.base = mrp_ll_scan_base{-5, -5};
    n.ids[1] = -1;
    const Packed p = pack(env, n.job, n.args());
    CHECK(p.ok && p.used == 3 && !(p.d.ctx_flags & mrp::kCtxScanParent) && (p.d.ctx_flags & mrp::kCtxScan));
  }
  {  // one agent: accepted, nothing to compare (found 0, count 0 on the device)
    Node n;
    n.job.n_agents = 1;
    n.job.agent_idx = 0;
    n.ids[0] = 5;
    const Packed p = pack(env, n.job, n.args());
    CHECK(p.ok && (p.d.ctx_flags & mrp::kCtxScan) && !(p.d.ctx_flags & mrp::kCtxScanParent) && p.used == 0);
  }
  // ---- every rejection of mrp_ll.h ----
  { Node n; n.job.flags = MRP_LL_JOB_SCAN_FROM_PARENT; CHECK(rejected(env, n.job, n.args())); }                       // without MRP_LL_JOB_SCAN_CONFLICTS
  { Node n; CHECK(rejected(env, n.job, PackArgs{true, nullptr, nullptr})); }                                          // through mrp_ll_submit_scan / _sets
  { Node n; CHECK(rejected(env, n.job, PackArgs{false, nullptr, nullptr})); }                                         // through mrp_ll_submit
  { Node n; CHECK(rejected(env, n.job, PackArgs{false, nullptr, &n.base})); }                                         // no conflicts array
  { Node n; n.ids[1] = -1; CHECK(rejected(env, n.job, n.args())); }                                                   // no slot for the replaced path
  { Node n; n.ids[1] = 8; CHECK(rejected(env, n.job, n.args())); }                                                    // ... a slot that does not exist
  { Node n; n.len[1] = 0; CHECK(rejected(env, n.job, n.args())); }                                                    // an empty replaced path
  { Node n; n.base.parent_count = -1; CHECK(rejected(env, n.job, n.args())); }
  { Node n; n.base.clean_before = -1; CHECK(rejected(env, n.job, n.args())); }
  // ... and what MRP_LL_JOB_SCAN_CONFLICTS requires
  { Node n; n.ids[2] = -1; CHECK(rejected(env, n.job, n.args())); }
  { Node n; n.len[0] = 0; CHECK(rejected(env, n.job, n.args())); }
  { Node n; n.job.algo = MRP_LL_ASTAR; CHECK(rejected(env, n.job, n.args())); }
  { Node n; n.job.flags |= MRP_LL_JOB_ROOT_CHAIN; CHECK(rejected(env, n.job, n.args())); }
  { Node n; n.job.path_ids = nullptr; CHECK(rejected(env, n.job, n.args())); }
  { Node n; n.job.agent_idx = 3; CHECK(rejected(env, n.job, n.args())); }
  { Node n; PackEnv noStore = makeEnv(); noStore.pathStoreSlots = 0; CHECK(rejected(noStore, n.job, n.args())); }
  std::printf("pack_node_check: ok\n");
  return 0;
}
