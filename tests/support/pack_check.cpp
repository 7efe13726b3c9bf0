// TEST INFRASTRUCTURE — a stand-alone check of the engine's packer and unpacker
// (libmultirobotplanning_amd/csrc/host/ll_pack.h), built by tests/test_pack_cpu.py with the host sanitizers and run as a
// program of its own.  Every slot area handed to the code under test is a heap block of exactly the stated capacity, so
// AddressSanitizer sees a word written or read past it.  Expected values are worked out by hand from the word formats of
// ll_device.h.  Exits non-zero at the first failed check.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../libmultirobotplanning_amd/csrc/host/ll_pack.h"

using namespace mrp::host;
using mrp::DevJob;
using mrp::DevResult;

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "pack_check: line %d: %s\n", __LINE__, #cond);              \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

namespace {

constexpr int kHorizon = 16;

PackEnv makeEnv() {  // one 4 x 3 map, no session, no stores
  PackEnv env;
  static int owner;
  env.owner = &owner;
  env.maps.push_back(MapRec{4, 3, 1, 0});
  env.maxHorizon = kHorizon;
  env.ldsNodes = 2048;
  env.arenaNodes = 131072;
  env.arenaPathsBytes = 128 * 1024;
  return env;
}
mrp_ll_job makeJob(int algo) {  // (0, 0) -> (3, 2) on map 0
  mrp_ll_job j;
  std::memset(&j, 0, sizeof(j));
  j.algo = algo;
  j.w = 1.5f;
  j.goal_x = 3;
  j.goal_y = 2;
  j.max_expansions = -1;
  j.result_path_id = -1;
  return j;
}
// a job slot's areas as the session hands them out: heap blocks of exactly the slot's capacity
struct Slot {
  uint32_t index;
  std::unique_ptr<uint32_t[]> cons;
  std::unique_ptr<uint16_t[]> paths;
  ConsSinkSlot cs;
  PathSinkSlot ps;
  explicit Slot(uint32_t slot, uint32_t consWords = kSlotConsWords, uint32_t pathHalfs = kSlotPathHalfs)
      : index(slot), cons(new uint32_t[consWords]), paths(new uint16_t[pathHalfs]),
        cs{cons.get(), slot * consWords, consWords}, ps{paths.get(), slot * pathHalfs, pathHalfs} {}
};
bool pack(const PackEnv& env, const mrp_ll_job& j, Slot& s, DevJob& d, PackArgs args = PackArgs(), PendingSet* pending = nullptr) {
  PendingSet local;
  return packJob(env, j, args, s.cs, s.ps, d, pending ? *pending : local);
}
bool rejected(const PackEnv& env, const mrp_ll_job& j, PackArgs args = PackArgs()) {
  Slot s(0);
  DevJob d;
  PendingSet p;
  const bool ok = pack(env, j, s, d, args, &p);
  return !ok && p.slot == -1;
}

void vertexAndEdgeWords() {
  PackEnv env = makeEnv();
  mrp_ll_job j = makeJob(MRP_LL_ASTAR);
  const int32_t vc[] = {2, 1, 2,           // t, x, y -> 0x00020201
                        9, 4, 2,           // outside the grid (on the goal's row): dropped, and not a goal constraint
                        kHorizon, 3, 2,    // on the goal at t >= max_horizon: dropped from the words, but it is the last goal constraint
                        3, 3, 2};          // on the goal -> 0x00030203
  const int32_t ec[] = {1, 1, 0, 2, 0,          // (1,0) -> (2,0): Right = 2 -> 1 << 19 | (0 * 4 + 1) << 3 | 2
                        1, 0, 0, 2, 0,          // no neighbours: dropped
                        kHorizon, 1, 0, 2, 0,   // t >= max_horizon: dropped
                        1, -1, 0, 0, 0};        // from outside the grid: dropped
  j.n_vertex_constraints = 4;
  j.vertex_constraints = vc;
  j.n_edge_constraints = 4;
  j.edge_constraints = ec;
  Slot s(5);
  DevJob d;
  CHECK(pack(env, j, s, d));
  CHECK(d.vc_off == 5u * kSlotConsWords && d.n_vc == 2 && d.n_ec == 1);
  CHECK(d.ec_off == d.vc_off + d.n_vc);
  CHECK(s.cons[0] == 0x00020201u && s.cons[1] == 0x00030203u);
  CHECK(s.cons[2] == ((1u << 19) | ((0u * 4u + 1u) << 3) | 2u) && s.cons[2] == 0x0008000Au);
  CHECK(s.cs.used == 3);
  CHECK(d.last_goal_constraint == kHorizon);
  CHECK(d.dimx == 4 && d.dimy == 3 && d.sx == 0 && d.sy == 0 && d.gx == 3 && d.gy == 2 && d.algo == MRP_LL_ASTAR);
  // the first two alone: none of them is on the goal, the one outside the grid least of all
  j.n_vertex_constraints = 2;
  Slot s2(0);
  CHECK(pack(env, j, s2, d) && d.last_goal_constraint == -1 && d.n_vc == 1);
  // the same words from the functions the CPU emulation of the compact tier calls
  std::vector<uint32_t> words;
  struct Sink {
    std::vector<uint32_t>& v;
    void push(uint32_t w) { v.push_back(w); }
  } sink{words};
  CHECK(packVertexWords(vc, 4, 4, 3, kHorizon, 3, 2, false, sink) == kHorizon);
  packEdgeWords(ec, 4, 4, 3, kHorizon, sink);
  CHECK(words.size() == 3 && words[0] == 0x00020201u && words[1] == 0x00030203u && words[2] == 0x0008000Au);
  words.clear();
  CHECK(packVertexWords(vc, 2, 4, 3, kHorizon, 3, 2, true, sink) == 9);  // an agent without a task: any cell counts
}

void focalTable() {
  PackEnv env = makeEnv();
  mrp_ll_job j = makeJob(MRP_LL_ASTAR_EPS);
  const int32_t len[] = {2, 0, 3};
  const int32_t p0[] = {0, 0, 1, 0}, p2[] = {3, 2, 4, 2, 3, 1};  // agent 2 leaves the grid at t = 1
  const int32_t* const xy[] = {p0, nullptr, p2};
  j.n_agents = 3;
  j.agent_idx = 0;
  j.path_len = len;
  j.path_xy = xy;
  Slot s(3);
  DevJob d;
  CHECK(pack(env, j, s, d));
  CHECK(d.t_pad == 3 && d.n_agents_pad == 16 && d.path_off == 3u * kSlotPathHalfs && d.ctx_flags == 0);
  const uint16_t col2[] = {0x0203, 0xFFFF, 0x0103};
  for (int t = 0; t < 3; ++t)
    for (int a = 0; a < 16; ++a) CHECK(s.paths[t * 16 + a] == (a == 2 ? col2[t] : 0xFFFF));  // own and empty columns: 0xFFFF
  // searched for the agent with the empty path: the short path of agent 0 is extended by its last cell
  j.agent_idx = 1;
  Slot s1(0);
  CHECK(pack(env, j, s1, d) && d.t_pad == 3);
  const uint16_t col0[] = {0x0000, 0x0001, 0x0001};
  for (int t = 0; t < 3; ++t)
    for (int a = 0; a < 16; ++a) CHECK(s1.paths[t * 16 + a] == (a == 0 ? col0[t] : a == 2 ? col2[t] : 0xFFFF));
}

void slotOverflow() {
  PackEnv env = makeEnv();
  {
    mrp_ll_job j = makeJob(MRP_LL_ASTAR);
    std::vector<int32_t> vc(3 * (kSlotConsWords + 1), 0);  // (t = 0, 0, 0), one more than the area holds
    j.n_vertex_constraints = static_cast<int32_t>(kSlotConsWords + 1);
    j.vertex_constraints = vc.data();
    CHECK(rejected(env, j));
    j.n_vertex_constraints = static_cast<int32_t>(kSlotConsWords);  // exactly full: accepted
    Slot s(0);
    DevJob d;
    CHECK(pack(env, j, s, d) && d.n_vc == kSlotConsWords);
  }
  {
    mrp_ll_job j = makeJob(MRP_LL_ASTAR_EPS);
    const int rows = static_cast<int>(kSlotPathHalfs / 16 + 1);  // [rows][16] = kSlotPathHalfs + 16 halfwords
    std::vector<int32_t> path(2 * rows, 0);
    const int32_t len[] = {0, rows};
    const int32_t* const xy[] = {nullptr, path.data()};
    j.n_agents = 2;
    j.path_len = len;
    j.path_xy = xy;
    CHECK(rejected(env, j));
  }
}

void rejections() {
  PackEnv env = makeEnv();
  mrp_ll_job j = makeJob(MRP_LL_ASTAR);
  CHECK(!rejected(env, j));
  j.map_id = 1;
  CHECK(rejected(env, j));
  j.map_id = -1;
  CHECK(rejected(env, j));
  j = makeJob(7);
  CHECK(rejected(env, j));
  j = makeJob(MRP_LL_ASTAR_EPS);
  j.initial_cost = 1;
  CHECK(rejected(env, j));
  j = makeJob(MRP_LL_ASTAR);
  j.initial_cost = 0x40000000;
  CHECK(rejected(env, j));
  j.initial_cost = 0x3FFFFFFF;
  CHECK(!rejected(env, j));
  j = makeJob(MRP_LL_ASTAR);
  j.start_x = 4;
  CHECK(rejected(env, j));
  j = makeJob(MRP_LL_ASTAR);
  j.goal_y = 3;
  CHECK(rejected(env, j));
  j = makeJob(MRP_LL_ASTAR_TA);  // ... but an agent without a task has no goal to check
  j.goal_y = 3;
  j.flags = MRP_LL_JOB_NO_GOAL;
  CHECK(!rejected(env, j));
  j = makeJob(MRP_LL_ASTAR_EPS);
  j.flags = MRP_LL_JOB_STORE_RESULT;
  j.result_path_id = 0;
  CHECK(rejected(env, j));  // no path store
  env.pathStoreSlots = 8;
  CHECK(!rejected(env, j));
  {  // node scan: admitted only by a call that hands conflicts back, and every other agent's path is named by its slot
    const int32_t ids[] = {-1, 1}, len[] = {0, 1}, idsBad[] = {-1, -1};
    j = makeJob(MRP_LL_ASTAR_EPS);
    j.flags = MRP_LL_JOB_SCAN_CONFLICTS;
    j.n_agents = 2;
    j.path_ids = ids;
    j.path_len = len;
    PackArgs scanOk;
    scanOk.scanAllowed = true;
    CHECK(rejected(env, j));
    Slot s(0);
    DevJob d;
    CHECK(pack(env, j, s, d, scanOk) && (d.ctx_flags & mrp::kCtxScan) && (d.ctx_flags & mrp::kCtxById) && d.reserved == 0);
    CHECK(s.cons[0] == mrp::kNoStoreSlot && s.cons[1] == 1u);
    j.path_ids = idsBad;
    CHECK(rejected(env, j, scanOk));
  }
  {  // root chains: only in a session of A*-epsilon jobs, at most kChainMaxAgents agents, every start and goal in the grid
    std::vector<int32_t> ids(mrp::kChainMaxAgents + 1, 0), sg(4 * (mrp::kChainMaxAgents + 1), 0);
    ids[1] = 1;
    sg[2] = 3; sg[3] = 2; sg[4] = 1; sg[6] = 3; sg[7] = 2;  // (0,0) -> (3,2), (1,0) -> (3,2)
    j = makeJob(MRP_LL_ASTAR_EPS);
    j.flags = MRP_LL_JOB_ROOT_CHAIN;
    j.n_agents = 2;
    j.path_ids = ids.data();
    j.chain_starts_goals_xy = sg.data();
    CHECK(rejected(env, j));  // no session
    env.session.active = true;
    env.session.kind = 0;
    env.session.outStride = 10240;
    env.session.ldsPathBytes = 4096;
    CHECK(rejected(env, j));  // a mixed session
    env.session.kind = 1;
    Slot s(2);
    DevJob d;
    CHECK(pack(env, j, s, d) && d.ctx_flags == mrp::kCtxChain && d.n_ctx == 2 && d.t_pad == 0 && d.reserved == 2);
    CHECK(s.cons[0] == 0x02030000u && s.cons[1] == 0x02030001u && s.cons[2] == 0u && s.cons[3] == 1u && s.cs.used == 4);
    j.n_agents = static_cast<int32_t>(mrp::kChainMaxAgents + 1);
    CHECK(rejected(env, j));
    j.n_agents = 2;
    sg[4] = 4;  // the second agent starts outside the grid
    CHECK(rejected(env, j));
  }
}

void constraintSets() {
  PackEnv env = makeEnv();
  env.consStoreSlots = 4;
  env.consStoreStride = 8;
  env.consSets.assign(4, ConsSetRec());
  const int32_t vc[] = {2, 1, 2, 9, 3, 2, 1, 0, 0};
  const int32_t ec[] = {1, 1, 0, 2, 0};
  mrp_ll_job j = makeJob(MRP_LL_ASTAR_EPS);
  j.flags = MRP_LL_JOB_CONSTRAINT_SET;
  j.n_vertex_constraints = 1;
  j.vertex_constraints = vc;
  j.n_edge_constraints = 1;
  j.edge_constraints = ec;
  mrp_ll_constraint_ref ref = {0, 2};
  PackArgs args;
  CHECK(rejected(env, j, args));  // no ref
  args.ref = &ref;
  ref = {1, 1};
  CHECK(rejected(env, j, args));  // base == result
  ref = {0, 2};
  CHECK(rejected(env, j, args));  // the base has not been written
  ConsSetRec& base = env.consSets[0];
  base.written = true;
  base.inFlight = true;
  base.nVc = 4; base.nEc = 2; base.lastGoal = 7; base.mapId = 0; base.gx = 3; base.gy = 2;
  CHECK(rejected(env, j, args));  // the base's writer has not been collected
  base.inFlight = false;
  base.gx = 0;
  CHECK(rejected(env, j, args));  // built for another goal
  base.gx = 3;
  j.n_vertex_constraints = 2;     // 4 + 2 + 2 + 1 = 9 words into slots of 8
  {
    Slot s(0);
    DevJob d;
    PendingSet p;
    CHECK(!pack(env, j, s, d, args, &p) && p.slot == -1);
  }
  j.n_vertex_constraints = 1;     // 4 + 2 + 1 + 1 = 8 words
  Slot s(1);
  DevJob d;
  PendingSet p;
  CHECK(pack(env, j, s, d, args, &p));
  CHECK(d.pad_[0] == 1u && d.pad_[1] == (4u | 2u << 16) && d.pad_[2] == 3u);
  CHECK(d.n_vc == 5 && d.n_ec == 3 && d.last_goal_constraint == 7);
  CHECK(s.cs.used == 2 && s.cons[0] == 0x00020201u && s.cons[1] == 0x0008000Au && d.ec_off == d.vc_off + 1);
  CHECK(p.slot == 2 && p.rec.nVc == 5 && p.rec.nEc == 3 && p.rec.lastGoal == 7 && p.rec.mapId == 0 && p.rec.gx == 3 && p.rec.gy == 2);
  {  // the additions' goal constraint is later than the base's
    mrp_ll_job j9 = j;
    j9.vertex_constraints = vc + 3;
    Slot s9(0);
    DevJob d9;
    CHECK(pack(env, j9, s9, d9, args) && d9.last_goal_constraint == 9);
  }
  int32_t slot = 99;
  uint32_t seq = 99;
  commitSet(env, false, p, slot, seq);
  CHECK(slot == -1 && seq == 0 && !env.consSets[2].written && env.consSets[2].seq == 0 && env.consSetSeq == 0);
  commitSet(env, true, p, slot, seq);
  CHECK(slot == 2 && seq == 1 && env.consSets[2].written && env.consSets[2].inFlight && env.consSets[2].nVc == 5);
  setCollected(env, 2, seq + 1);  // an earlier writer of a recycled slot
  CHECK(env.consSets[2].inFlight);
  setCollected(env, 4, seq);      // no such slot
  setCollected(env, 2, seq);
  CHECK(!env.consSets[2].inFlight && env.consSets[2].written);
}

void sipp() {
  PackEnv env = makeEnv();
  mrp_ll_job j = makeJob(MRP_LL_SIPP);
  const int32_t xy[] = {1, 1, 1, 1}, cnt[] = {2, 0};
  const int32_t iv[] = {7, INT_MAX, 2, 3};  // out of order
  j.n_collision_locations = 1;
  j.collision_xy = xy;
  j.collision_count = cnt;
  j.collision_intervals = iv;
  // cellIdx: 12 halfwords (cell 5 = special 1), specFirst[2], two safe intervals [0,1], [4,6]
  const uint32_t want[12] = {0, 0, 0x00010000u, 0, 0, 0, 0, 2, 0, 1, 4, 6};
  DevJob d;
  {
    Slot s(0, 12);
    CHECK(pack(env, j, s, d) && s.cs.used == 12 && std::memcmp(s.cons.get(), want, sizeof(want)) == 0);
    CHECK(d.n_vc == 1 && d.n_ec == 2 && d.t_pad == 0 && d.last_goal_constraint == 0 && d.algo == MRP_LL_SIPP);
    Slot small(0, 11);
    CHECK(!pack(env, j, small, d));
  }
  {  // the start cell is the special one
    j.start_x = 1;
    j.start_y = 1;
    j.initial_cost = 2;  // inside [2,3]
    Slot s(0, 12);
    CHECK(pack(env, j, s, d) && d.t_pad == 0xFFFFFFFFu && d.last_goal_constraint == 2);
    j.initial_cost = 5;  // inside the second safe interval
    CHECK((s.cs.used = 0, pack(env, j, s, d)) && d.t_pad == 1);
    j.initial_cost = static_cast<int32_t>(mrp::kGMask) + 1;
    CHECK((s.cs.used = 0, !pack(env, j, s, d)));
    j.initial_cost = 0;
    j.start_x = j.start_y = 0;
  }
  {  // an empty list after a non-empty one on the same cell: the default interval again
    j.n_collision_locations = 2;
    const uint32_t want2[10] = {0, 0, 0x00010000u, 0, 0, 0, 0, 1, 0, 0x7FFFFFFFu};
    Slot s(0, 10);
    CHECK(pack(env, j, s, d) && s.cs.used == 10 && std::memcmp(s.cons.get(), want2, sizeof(want2)) == 0);
    j.n_collision_locations = 1;
  }
  {  // the incrementally maintained table holds the same intervals and packs the same words
    mrp_ll_sipp_table T;
    T.dimx = 4;
    T.dimy = 3;
    T.cellIdx.assign(12, 0);
    T.cellIdx16.assign(12, 0);
    T.isDirty.assign(12, 0);
    sippTableAddCell(&T, 5, 7, INT_MAX, true);
    sippTableAddCell(&T, 5, 2, 3, true);
    CHECK(T.totalSafe == 2 && T.spec.size() == 1 && T.spec[0].safe[0].s == 0 && T.spec[0].safe[0].e == 1 &&
          T.spec[0].safe[1].s == 4 && T.spec[0].safe[1].e == 6);
    mrp_ll_job jt = makeJob(MRP_LL_SIPP);
    jt.sipp_table = &T;
    Slot s(0, 12);
    DevJob dt;
    CHECK(pack(env, jt, s, dt) && s.cs.used == 12 && std::memcmp(s.cons.get(), want, sizeof(want)) == 0);
    CHECK(dt.n_vc == 1 && dt.n_ec == 2 && dt.t_pad == 0 && dt.ctx_flags == 0);
    // a committed path's stays reach the table when its job comes back (batch form: the host adds them)
    const uint32_t raw[] = {0u | 0u << 16, 1u | 3u << 16};  // cell 0 at t = 0, cell 1 from t = 3 on
    DevResult r;
    std::memset(&r, 0, sizeof(r));
    r.status = mrp::ST_OK;
    r.n_states = 2;
    finishSippTableJob(&T, 2u, r, reinterpret_cast<const uint16_t*>(raw));
    CHECK(T.spec.size() == 3 && T.spec[1].safe.size() == 1 && T.spec[1].safe[0].s == 3 && T.spec[2].safe.size() == 1 &&
          T.spec[2].safe[0].s == 0 && T.spec[2].safe[0].e == 2);
  }
}

void unpacking() {
  mrp_ll_stats stats;
  std::memset(&stats, 0, sizeof(stats));
  DevResult d;
  std::memset(&d, 0, sizeof(d));
  d.status = mrp::ST_OK;
  d.cost = 3;
  d.fmin = 3;
  d.n_states = 2;
  d.expanded = 4;
  mrp_ll_result r;
  std::memset(&r, 0, sizeof(r));
  {  // A* with initial_cost 5
    const uint16_t p[] = {0x0000, 0x0001};
    unpackResult(stats, d, p, false, r, false, 0, 5);
    CHECK(r.status == MRP_LL_OK && r.cost == 8 && r.fmin == 8 && r.n_states == 2 && r.expanded == 4 && stats.jobs == 1);
    d.n_states = 1;  // the start is the goal: the start node's f carries no initial cost
    unpackResult(stats, d, p, false, r, false, 0, 5);
    CHECK(r.cost == 8 && r.fmin == 3 && stats.jobs == 2 && stats.expansions == 8);
    unpackResult(stats, d, p, true, r, false, 0, 5);  // a rejected job is no search
    CHECK(r.status == MRP_LL_BAD_JOB && r.cost == 0 && stats.jobs == 2);
  }
  {  // SIPP with start time 5; (c0, g = 0), (c1, g = 3) is a Wait of cost 2 and a move
    const uint32_t raw[] = {0u | 0u << 16, 1u | 3u << 16};
    d.n_states = 2;
    d.cost = 10;
    std::unique_ptr<int32_t[]> txy(new int32_t[9]), act(new int32_t[3]), cost(new int32_t[3]);
    r.states_txy = txy.get();
    r.actions = act.get();
    r.action_costs = cost.get();
    r.states_cap = 3;
    unpackResult(stats, d, reinterpret_cast<const uint16_t*>(raw), false, r, true, 4, 5);
    CHECK(r.status == MRP_LL_OK && r.cost == 5 && r.fmin == 3 && r.n_states == 3);
    const int32_t wantTxy[9] = {0, 0, 0, 2, 0, 0, 3, 1, 0};
    CHECK(std::memcmp(txy.get(), wantTxy, sizeof(wantTxy)) == 0);
    CHECK(act[0] == MRP_LL_ACT_WAIT && cost[0] == 2 && act[1] == MRP_LL_ACT_RIGHT && cost[1] == 1);
    // one state short: truncated, and nothing is written past states_cap
    std::unique_ptr<int32_t[]> txy2(new int32_t[6]), act2(new int32_t[2]), cost2(new int32_t[2]);
    r.states_txy = txy2.get();
    r.actions = act2.get();
    r.action_costs = cost2.get();
    r.states_cap = 2;
    unpackResult(stats, d, reinterpret_cast<const uint16_t*>(raw), false, r, true, 4, 5);
    CHECK(r.status == MRP_LL_PATH_TRUNCATED && r.n_states == 3 && r.cost == 5 && txy2[3] == 2 && act2[1] == MRP_LL_ACT_RIGHT);
  }
  {  // task assignment: a Wait at the goal (2, 0) is free
    const uint16_t p[] = {0x0001, 0x0001, 0x0002, 0x0002};
    d.n_states = 4;
    d.cost = 2;
    mrp_ll_job j = makeJob(MRP_LL_ASTAR_TA);
    j.goal_x = 2;
    j.goal_y = 0;
    const int32_t init = jobInitOf(j, true);
    CHECK(init == (0x40000000 | 0x0002) && jobInitOf(j, false) == 0);
    std::unique_ptr<int32_t[]> txy(new int32_t[9]), act(new int32_t[3]), cost(new int32_t[3]);
    r.states_txy = txy.get();
    r.actions = act.get();
    r.action_costs = cost.get();
    r.states_cap = 3;  // one state short
    unpackResult(stats, d, p, false, r, false, 0, init);
    CHECK(r.status == MRP_LL_PATH_TRUNCATED && r.cost == 2 && r.n_states == 4);
    CHECK(cost[0] == 1 && cost[1] == 1 && cost[2] == 0 && act[0] == MRP_LL_ACT_WAIT && act[1] == MRP_LL_ACT_RIGHT && act[2] == MRP_LL_ACT_WAIT);
    CHECK(txy[6] == 2 && txy[7] == 2 && txy[8] == 0);
    j.flags = MRP_LL_JOB_NO_GOAL;
    CHECK(jobInitOf(j, true) == (0x40000000 | 0x10000));
  }
  {  // a root chain's output area of exactly outWords words; the offsets in it are words the device wrote
    const uint32_t outWords = 64;
    std::unique_ptr<uint32_t[]> area(new uint32_t[outWords]);
    std::memset(area.get(), 0, outWords * 4);
    auto entry = [&](int i, uint32_t status, uint32_t cost, uint32_t nStates, uint32_t off) {
      uint32_t* e = area.get() + i * mrp::kChainEntryWords;
      e[0] = status; e[1] = cost; e[2] = cost; e[3] = nStates; e[4] = 3; e[5] = off;
    };
    entry(0, mrp::ST_OK, 1, 2, 32);            // a path of two states at word 32
    area[32] = 0x0000u | 0x0001u << 16;
    entry(1, mrp::ST_OK, 1, 2, outWords + 1);  // the offset is past the area
    entry(2, mrp::ST_OK, 2, 3, outWords - 1);  // the offset is inside, the path runs one word past the end
    std::memset(&d, 0, sizeof(d));
    d.status = mrp::ST_OK;
    d.n_states = 3;
    d.expanded = 9;
    d.cost = -1;
    d.fmin = -1;
    mrp_ll_result sub[4];
    std::memset(sub, 0, sizeof(sub));
    std::unique_ptr<int32_t[]> txy(new int32_t[4 * 6]);
    for (int i = 0; i < 4; ++i) {
      sub[i].states_txy = txy.get() + 6 * i;
      sub[i].states_cap = 2;
      sub[i].status = -7;
    }
    std::memset(&r, 0, sizeof(r));
    r.chain_results = sub;
    const int64_t jobs0 = stats.jobs;
    unpackChain(stats, d, reinterpret_cast<const uint16_t*>(area.get()), false, r, 4, outWords);
    CHECK(r.status == MRP_LL_OK && r.n_states == 3 && r.expanded == 9 && r.cost == -1);
    CHECK(sub[0].status == MRP_LL_OK && sub[0].cost == 1 && sub[0].n_states == 2 && txy[4] == 1 && txy[5] == 0);
    CHECK(sub[1].status == mrp::ST_BAD && sub[1].n_states == 0);
    CHECK(sub[2].status == mrp::ST_BAD && sub[2].n_states == 0);
    CHECK(sub[3].status == MRP_LL_NOT_RUN && sub[3].n_states == 0);
    CHECK(stats.jobs == jobs0 + 3);
    unpackChain(stats, d, reinterpret_cast<const uint16_t*>(area.get()), true, r, 4, outWords);
    CHECK(r.status == MRP_LL_BAD_JOB && r.n_states == 0 && sub[0].status == MRP_LL_NOT_RUN);
  }
  {  // conflicts: the last kScanOutHalfs halfwords of an output area of exactly outStride halfwords
    const uint32_t outStride = 96;
    std::unique_ptr<uint16_t[]> area(new uint16_t[outStride]);
    const int32_t ten[10] = {1, 4, 0, 2, 1, 3, 2, 3, 1, 6};
    std::memcpy(area.get() + (outStride - mrp::kScanOutHalfs), ten, sizeof(ten));
    mrp_ll_conflict c;
    std::memset(&d, 0, sizeof(d));
    d.status = mrp::ST_OK;
    unpackConflicts(d, area.get(), outStride, false, c);
    CHECK(c.found == 1 && c.time == 4 && c.agent2 == 2 && c.type == 1 && c.y2 == 1 && c.count == 6);
    d.status = mrp::ST_NO_SOLUTION;
    unpackConflicts(d, area.get(), outStride, false, c);
    CHECK(c.found == -1 && c.time == 0 && c.agent1 == 0 && c.agent2 == 0 && c.type == 0 && c.x1 == 0 && c.y1 == 0 && c.x2 == 0 &&
          c.y2 == 0 && c.count == 0);
    d.status = mrp::ST_OK;
    unpackConflicts(d, nullptr, outStride, true, c);  // a rejected job never ran
    CHECK(c.found == -1 && c.count == 0);
  }
  {
    PackEnv env = makeEnv();
    DevJob t;
    trivialRejectedJob(env, t);
    CHECK(t.dimx == 1 && t.dimy == 1 && t.max_expansions == 0 && t.last_goal_constraint == -1);
  }
}

}  // namespace

int main() {
  vertexAndEdgeWords();
  focalTable();
  slotOverflow();
  rejections();
  constraintSets();
  sipp();
  unpacking();
  std::printf("pack_check: ok\n");
  return 0;
}
