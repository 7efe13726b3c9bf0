// TEST INFRASTRUCTURE — a stand-alone check of what the packer (libmultirobotplanning_amd/csrc/host/ll_pack.h) makes of
// MRP_LL_JOB_TABLE_H, built by tests/test_table_h_cpu.py with the host sanitizers and run as a program of its own:
//   the flag sets the device flag, the table's word offset and the table-h algo word, and nothing else of the descriptor;
//   every refusal mrp_ll.h lists is a refusal (never a silent Manhattan search);
//   a job WITHOUT the flag packs to the bytes it always packed to, whatever its heuristic_id.
// Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../libmultirobotplanning_amd/csrc/host/ll_pack.h"

using namespace mrp::host;
using mrp::DevJob;

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      std::fprintf(stderr, "table_h_pack_check: line %d: %s\n", __LINE__, #cond);       \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

namespace {

PackEnv makeEnv() {  // two maps (4 x 3 and 40 x 2), three tables: two of map 0, one of map 1
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{4, 3, 1, 0});
  env.maps.push_back(MapRec{40, 2, 3, 32});
  env.heurs.push_back(HeurRec{0, 64});
  env.heurs.push_back(HeurRec{0, 64 + 512});
  env.heurs.push_back(HeurRec{1, 64 + 1024});
  env.maxHorizon = 16;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 128 * 1024;
  env.pathStoreSlots = 8;
  env.consStoreSlots = 4;
  env.consStoreStride = 64;
  env.consSets.resize(4);
  return env;
}
mrp_ll_job makeJob(int algo) {  // (0, 0) -> (3, 1) on map 0 with one vertex and one edge constraint
  static const int32_t vc[] = {2, 1, 1};
  static const int32_t ec[] = {1, 0, 0, 1, 0};
  mrp_ll_job j;
  std::memset(&j, 0, sizeof(j));
  j.algo = algo;
  j.w = 1.5f;
  j.goal_x = 3;
  j.goal_y = 1;
  j.max_expansions = 77;
  j.result_path_id = -1;
  j.n_vertex_constraints = 1;
  j.vertex_constraints = vc;
  j.n_edge_constraints = 1;
  j.edge_constraints = ec;
  return j;
}
struct Slot {
  std::unique_ptr<uint32_t[]> cons;
  std::unique_ptr<uint16_t[]> paths;
  ConsSinkSlot cs;
  PathSinkSlot ps;
  Slot() : cons(new uint32_t[kSlotConsWords]), paths(new uint16_t[kSlotPathHalfs]), cs{cons.get(), 0, kSlotConsWords},
           ps{paths.get(), 0, kSlotPathHalfs} {}
};
bool pack(const PackEnv& env, const mrp_ll_job& j, DevJob& d, PackArgs args = PackArgs()) {
  Slot s;
  PendingSet p;
  std::memset(&d, 0xEE, sizeof(d));
  const bool ok = packJob(env, j, args, s.cs, s.ps, d, p);
  CHECK(ok || p.slot == -1);
  return ok;
}
bool refused(const PackEnv& env, const mrp_ll_job& j, PackArgs args = PackArgs()) {
  DevJob d;
  return !pack(env, j, d, args);
}

void flagSetsFlagOffsetAndAlgo() {
  const PackEnv env = makeEnv();
  for (int algo : {MRP_LL_ASTAR, MRP_LL_ASTAR_EPS}) {
    mrp_ll_job j = makeJob(algo);
    DevJob plain, flagged;
    CHECK(pack(env, j, plain));
    j.flags = MRP_LL_JOB_TABLE_H;
    j.heuristic_id = 1;
    if (algo == MRP_LL_ASTAR) j.initial_cost = 7;  // (the host unpacker applies it: nothing of it in the descriptor)
    CHECK(pack(env, j, flagged));
    CHECK(flagged.ctx_flags == (plain.ctx_flags | mrp::kCtxTableH));
    CHECK(flagged.heur_off == 64u + 512u && plain.heur_off == 0u);
    CHECK(flagged.algo == (mrp::kAlgoTableH | static_cast<uint32_t>(algo)) && plain.algo == static_cast<uint32_t>(algo));
    DevJob same = flagged;  // ... and nothing else differs
    same.ctx_flags = plain.ctx_flags;
    same.heur_off = plain.heur_off;
    same.algo = plain.algo;
    CHECK(std::memcmp(&same, &plain, sizeof(DevJob)) == 0);
    j.heuristic_id = 0;
    CHECK(pack(env, j, flagged) && flagged.heur_off == 64u);
    // a focal context shipped with the job stays what it is
    if (algo == MRP_LL_ASTAR_EPS) {
      static const int32_t p1[] = {0, 0, 1, 0, 2, 0};
      const int32_t len[2] = {0, 3};
      const int32_t* xy[2] = {nullptr, p1};
      j.n_agents = 2;
      j.path_len = len;
      j.path_xy = xy;
      CHECK(pack(env, j, flagged) && flagged.n_agents_pad == 16u && flagged.t_pad == 3u && (flagged.ctx_flags & mrp::kCtxTableH));
    }
  }
  {  // the other algorithms ignore the flag, as they ignore MRP_LL_JOB_TRY_LDS
    mrp_ll_job j = makeJob(MRP_LL_ASTAR_TA);
    j.heuristic_id = 1;
    DevJob a, b;
    CHECK(pack(env, j, a));
    j.flags = MRP_LL_JOB_TABLE_H;
    CHECK(pack(env, j, b) && std::memcmp(&a, &b, sizeof(DevJob)) == 0);
  }
}

void refusals() {
  PackEnv env = makeEnv();
  for (int algo : {MRP_LL_ASTAR, MRP_LL_ASTAR_EPS}) {
    mrp_ll_job j = makeJob(algo);
    j.flags = MRP_LL_JOB_TABLE_H;
    j.heuristic_id = 1;
    CHECK(!refused(env, j));
    for (int bad : {-1, 3, 1000}) {  // unknown ids
      mrp_ll_job k = j;
      k.heuristic_id = bad;
      CHECK(refused(env, k));
    }
    {  // a table of another map
      mrp_ll_job k = j;
      k.heuristic_id = 2;
      CHECK(refused(env, k));
      k.map_id = 1;
      k.goal_y = 1;
      CHECK(!refused(env, k));
      k.heuristic_id = 0;
      CHECK(refused(env, k));
    }
    const int32_t ids[2] = {-1, 3};
    const int32_t len[2] = {0, 3};
    mrp_ll_constraint_ref ref{-1, 1};
    mrp_ll_scan_base base{0, 0};
    PackArgs args;
    args.scanAllowed = true;
    args.ref = &ref;
    args.base = &base;
    for (int with : {MRP_LL_JOB_STORE_RESULT, MRP_LL_JOB_ROOT_CHAIN, MRP_LL_JOB_HEAVY, MRP_LL_JOB_SCAN_CONFLICTS,
                     MRP_LL_JOB_SCAN_CONFLICTS | MRP_LL_JOB_SCAN_FROM_PARENT, MRP_LL_JOB_SCAN_FROM_PARENT, MRP_LL_JOB_CONSTRAINT_SET}) {
      mrp_ll_job k = j;
      k.flags |= with;
      k.result_path_id = 2;
      k.n_agents = 2;
      k.agent_idx = 0;
      k.path_len = len;
      k.path_ids = (with & MRP_LL_JOB_SCAN_CONFLICTS) ? ids : nullptr;
      CHECK(refused(env, k, args));
    }
    {  // path_ids
      mrp_ll_job k = j;
      k.n_agents = 2;
      k.path_len = len;
      k.path_ids = ids;
      CHECK(refused(env, k));
    }
    // one-algorithm sessions (mrp_ll_session_begin_algo / _tiers / _tiers_gated: kind 1 and 2) and SIPP sessions; a mixed
    // session takes the job
    env.session.active = true;
    env.session.outStride = 1024;
    env.session.ldsPathBytes = 4096;
    for (int kind : {1, 2}) {
      env.session.kind = kind;
      CHECK(refused(env, j));
      mrp_ll_job plain = j;
      plain.flags = 0;
      CHECK(!refused(env, plain));  // (the session's own check of the job's algorithm is not the packer's)
    }
    env.session.kind = 0;
    CHECK(!refused(env, j));
    env.session.sipp = true;
    CHECK(refused(env, j));
    env.session = PackEnv::Session();
  }
}

// Without the flag nothing of a job's descriptor depends on heuristic_id.  What a plain job packs to is fixed by
// tests/support/pack_check.cpp against the word formats; here: the words that the flag touches keep their plain values.
void unflaggedJobsAreWhatTheyWere() {
  const PackEnv env = makeEnv();
  for (int algo : {MRP_LL_ASTAR, MRP_LL_ASTAR_EPS}) {
    mrp_ll_job j = makeJob(algo);
    DevJob ref;
    CHECK(pack(env, j, ref));
    CHECK(ref.algo == static_cast<uint32_t>(algo) && ref.heur_off == 0u && (ref.ctx_flags & mrp::kCtxTableH) == 0u);
    CHECK(ref.n_vc == 1u && ref.n_ec == 1u && ref.vc_off == 0u && ref.ec_off == 1u && ref.max_expansions == 77 && ref.store_out_id == mrp::kNoStoreSlot);
    for (int hid : {-5, 0, 1, 2, 3, 1 << 30}) {  // valid, of another map, unknown: all the same
      j.heuristic_id = hid;
      DevJob d;
      CHECK(pack(env, j, d));
      CHECK(std::memcmp(&d, &ref, sizeof(DevJob)) == 0);
    }
  }
}

}  // namespace

int main() {
  static_assert(sizeof(mrp_ll_job) == 176, "mrp_ll_job keeps its size");
  static_assert(sizeof(DevJob) == 112, "DevJob keeps its size");
  static_assert(MRP_LL_JOB_TABLE_H == 256, "the flag's value");
  flagSetsFlagOffsetAndAlgo();
  refusals();
  unflaggedJobsAreWhatTheyWere();
  std::printf("table_h_pack_check: ok\n");
  return 0;
}
