// The packer of the low-level engine: mrp_ll_job -> DevJob + constraint words + path table; with it come the safe-interval
// tables (ll_sipp_table.h) and the way back, DevResult -> mrp_ll_result (ll_unpack.h).
// Pure host logic: no HIP, no mrp_ll_ctx.  What it needs of the engine it reads from a PackEnv (a member of the context),
// what a call adds comes in as PackArgs and leaves as a PendingSet.  Compiles with plain g++ -std=c++17: the stand-alone
// check tests/support/pack_check.cpp runs it under the host sanitizers, tests/support/emu_ll.cpp feeds the CPU emulation
// of the compact tier with the words it writes.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/mrp_ll.h"
#include "../heur_layout.h"
#include "../ll_device.h"
#include "ll_sipp_table.h"
#include "ll_unpack.h"

namespace mrp {
namespace host {

struct MapRec {
  int32_t dimx, dimy;
  uint32_t wpr, wordOff;
};
struct HeurRec {  // MRP_LL_ASTAR_TA: shortest-path table of one goal cell, heurTableWords words inside the maps buffer
  int32_t mapId;
  uint32_t wordOff;
};
// halfwords, 0xFFFF = unreachable: [y * 32 + x] for maps up to 32 x 32 (what the compact tier copies into its window),
// [y * dimx + x] beyond (arena tier only)
static inline bool heurSmall(const MapRec& m) { return hb::isSmall(static_cast<uint32_t>(m.dimx), static_cast<uint32_t>(m.dimy)); }
static inline size_t heurTableWords(const MapRec& m) {
  return heurSmall(m) ? kHeurWords : (static_cast<size_t>(m.dimx) * m.dimy + 1) / 2;
}
static inline int heurStride(const MapRec& m) { return heurSmall(m) ? 32 : m.dimx; }

// Host mirror of one slot of the device-resident constraint store (mrp_ll_constraint_store_reserve): what the packer needs
// of a set without reading device memory.  Updated when a job that writes the slot is accepted, under the submit lock.
struct ConsSetRec {
  uint32_t nVc = 0, nEc = 0;   // packed vertex / edge words in the slot
  int32_t lastGoal = -1;       // m_lastGoalConstraint of the set (ecbs.cpp:268-273)
  int32_t mapId = -1, gx = 0, gy = 0;  // the map and the goal cell it was built for
  bool written = false;        // some accepted job has this slot as its result
  bool inFlight = false;       // ... and that job's result has not been collected yet
  uint32_t seq = 0;            // which write (a recycled slot's earlier writer must not clear inFlight)
};

// What the packer reads of the engine.  mrp_ll_ctx holds ONE of these as a member and keeps it current; nothing here is
// per call.
struct PackEnv {
  const void* owner = nullptr;     // identity of the engine (a mrp_ll_sipp_table of another engine ships whole)
  std::vector<MapRec> maps;
  std::vector<HeurRec> heurs;
  int32_t maxHorizon = 0, ldsNodes = 0, arenaNodes = 0;  // mrp_ll_options max_horizon / lds_nodes / arena_nodes as in force
  struct Session {
    bool active = false;
    bool sipp = false;             // mrp_ll_session_begin_sipp
    int kind = 0;                  // A* sessions: 0 = mixed kernel, 1 = A*-epsilon jobs only, 2 = A* jobs only
    uint32_t outStride = 0;        // halfwords per job slot of the host output area
    uint32_t ldsPathBytes = 0;     // bytes of the resident kernel's window that hold the focal path table (0: no compact tier)
  } session;
  uint32_t arenaPathsBytes = 0;
  uint32_t pathStoreSlots = 0;     // device-resident path store (mrp_ll_path_store_reserve); 0: none
  uint32_t consStoreSlots = 0, consStoreStride = 0;  // device-resident constraint store; 0 slots: none
  std::vector<ConsSetRec> consSets;                  // ... and its host mirror
  uint32_t consSetSeq = 0;
  // device-resident SIPP tables: chunks of sippTabsPerChunk tables of sippTabStride bytes each (about 64 MB a chunk)
  std::vector<uint8_t*> sippTabChunks;
  size_t sippTabStride = 0;
  int32_t sippTabsPerChunk = 64;
  mutable SippScratch sippScratch;  // work space of packSipp, not state
};

struct PackArgs {
  bool scanAllowed = false;                    // the call hands conflicts back (what admits MRP_LL_JOB_SCAN_CONFLICTS jobs)
  const mrp_ll_constraint_ref* ref = nullptr;  // the job's entry of mrp_ll_submit_sets (what admits MRP_LL_JOB_CONSTRAINT_SET jobs)
  const mrp_ll_scan_base* base = nullptr;      // the job's entry of mrp_ll_submit_node (what admits MRP_LL_JOB_SCAN_FROM_PARENT jobs)
};
// The constraint-store slot the job just packed writes (-1: none) and what the mirror holds for it once the job has been
// accepted (commitSet).
struct PendingSet {
  int32_t slot = -1;
  ConsSetRec rec;
};

// Where a packed job's constraint words / path table go in a session: a fixed ring-slot area.
constexpr uint32_t kSlotConsWords = 1024;        // 4 KB of constraint words per job
constexpr uint32_t kSlotPathHalfs = 16 * 1024;   // 32 KB path table per job
struct ConsSinkSlot {
  uint32_t* area;
  uint32_t baseOff, cap, used = 0;
  bool failed = false;
  size_t size() const { return baseOff + used; }
  bool fits(size_t n) const { return used + n <= cap; }
  void push(uint32_t w) {
    if (used >= cap) {
      failed = true;
      return;
    }
    area[used++] = w;
  }
  uint32_t* grow(size_t n) {
    if (used + n > cap) {
      failed = true;
      return nullptr;
    }
    uint32_t* p = area + used;
    used += static_cast<uint32_t>(n);
    return p;
  }
};
struct PathSinkSlot {
  uint16_t* area;
  uint32_t baseOff, cap;
  bool failed = false;
  uint16_t* alloc(size_t n, uint32_t& off) {
    if (n > cap) {
      failed = true;
      return nullptr;
    }
    off = baseOff;
    return area;
  }
};

// index in the reference's successor order Wait, Left, Right, Up, Down (ecbs.cpp:365-398)
static inline int neighborIndexFromDelta(int dx, int dy) {
  if (dx == 0 && dy == 0) return 0;
  if (dx == -1 && dy == 0) return 1;
  if (dx == 1 && dy == 0) return 2;
  if (dx == 0 && dy == 1) return 3;
  if (dx == 0 && dy == -1) return 4;
  return -1;
}

// The start interval (findSafeInterval(start, startTime), sipp.hpp:98-100,286-296) as the job's t_pad; no interval ->
// search() returns false: the device reports NO_SOLUTION for 0xFFFFFFFF (an empty open list cannot be encoded).
static inline uint32_t sippStartWord(const SippScratch::Iv* v, size_t n, bool special, int32_t startTime) {
  if (!special) return 0u;
  for (size_t k = 0; k < n; ++k)
    if (v[k].s <= startTime && v[k].e >= startTime) return static_cast<uint32_t>(k);
  return 0xFFFFFFFFu;
}

// The table of a job from an mrp_ll_sipp_table: cellIdx[cells], specFirst[K + 1], ivals[total][2] (see runSipp).
template <class ConsSink>
static inline bool packSippFromTable(const mrp_ll_job& j, const MapRec& mp, ConsSink& cs, DevJob& d) {
  if (!j.sipp_table->log.empty()) sippTableSync(const_cast<mrp_ll_sipp_table*>(j.sipp_table));
  const mrp_ll_sipp_table& T = *j.sipp_table;
  if (T.dimx != mp.dimx || T.dimy != mp.dimy) return false;
  const int cells = mp.dimx * mp.dimy;
  const uint32_t K = static_cast<uint32_t>(T.spec.size());
  d.algo = MRP_LL_SIPP;
  d.max_expansions = j.max_expansions;
  d.vc_off = static_cast<uint32_t>(cs.size());
  const size_t cw = (static_cast<size_t>(cells) + 1) / 2;  // cellIdx travels as halfwords
  uint32_t* w = cs.grow(cw + K + 1 + 2 * static_cast<size_t>(T.totalSafe));
  if (!w) return false;
  w[cw - 1] = 0;
  std::memcpy(w, T.cellIdx16.data(), sizeof(uint16_t) * cells);
  w += cw;
  uint32_t run = 0;
  for (uint32_t k = 0; k < K; ++k) {
    w[k] = run;
    run += static_cast<uint32_t>(T.spec[k].safe.size());
  }
  w[K] = run;
  w += K + 1;
  for (uint32_t k = 0; k < K; ++k) {
    if (!T.spec[k].safe.empty()) std::memcpy(w, T.spec[k].safe.data(), sizeof(SippScratch::Iv) * T.spec[k].safe.size());
    w += 2 * T.spec[k].safe.size();
  }
  d.n_vc = K;
  d.n_ec = T.totalSafe;
  d.ec_off = 0;
  d.n_agents_pad = 0;
  d.path_off = 0;
  const int32_t startTime = j.initial_cost;
  if (startTime > static_cast<int32_t>(kGMask)) return false;
  d.last_goal_constraint = startTime;
  const int sc = j.start_y * mp.dimx + j.start_x;
  const bool special = T.cellIdx[sc] != 0;
  const std::vector<SippScratch::Iv>* v = special ? &T.spec[T.cellIdx[sc] - 1].safe : nullptr;
  d.t_pad = sippStartWord(special ? v->data() : nullptr, special ? v->size() : 0, special, startTime);
  return !cs.failed;
}

// Session mode: the job carries the delta of a device-resident table (ll_device.h kSippResident).  `T` is updated (its
// dirty list is consumed, it is marked in flight), so the job MUST run — the session publishes it right away.
template <class ConsSink>
static inline bool packSippResident(const PackEnv& env, const mrp_ll_job& j, const MapRec& mp, ConsSink& cs, DevJob& d) {
  mrp_ll_sipp_table& T = *const_cast<mrp_ll_sipp_table*>(j.sipp_table);
  if (T.dimx != mp.dimx || T.dimy != mp.dimy) return false;
  const int cells = mp.dimx * mp.dimy;
  const int32_t startTime = j.initial_cost;
  if (startTime > static_cast<int32_t>(kGMask)) return false;
  const bool fresh = T.devFresh || T.epoch >= kSippEpochMax;  // epochs used up: start over from a zeroed table
  if (fresh && !T.log.empty()) sippTableSync(&T);
  if (T.overflow) return false;
  const size_t nRec = fresh ? T.spec.size() : T.dirty.size();
  // every record of one job has room for the same number of intervals: the longest list among them, as a power of two >= 2
  size_t longest = 0;
  if (fresh) {
    for (const mrp_ll_sipp_table::Spec& sp : T.spec) longest = std::max(longest, sp.safe.size());
  } else {
    for (int32_t cell : T.dirty) longest = std::max(longest, T.spec[T.cellIdx[cell] - 1].safe.size());
  }
  size_t recIv = 4;  // bounds words per record: whole 16-byte units
  while (recIv < longest) recIv *= 2;
  const size_t hdrWords = (nRec + 3) & ~size_t(3);
  if ((cs.size() & 3u) != 0 || !cs.fits(hdrWords + nRec * recIv)) return false;  // nothing consumed yet
  d.vc_off = static_cast<uint32_t>(cs.size());
  uint32_t* hdr = cs.grow(hdrWords + nRec * recIv);
  if (!hdr) return false;
  uint32_t* body = hdr + hdrWords;
  size_t r = 0;
  auto emit = [&](int32_t cell) {
    const mrp_ll_sipp_table::Spec& sp = T.spec[T.cellIdx[cell] - 1];
    hdr[r] = static_cast<uint32_t>(cell) | (static_cast<uint32_t>(sp.safe.size()) << 16);
    uint32_t* b = body + r * recIv;
    for (size_t q = 0; q < recIv; ++q)  // start | end << 16 (ll_device.h; T.overflow has vouched for the ranges)
      b[q] = q < sp.safe.size() ? static_cast<uint32_t>(sp.safe[q].s) |
                                      (sp.safe[q].e == INT32_MAX ? kSippEndInf : static_cast<uint32_t>(sp.safe[q].e)) << 16
                                : 0u;
    if (recIv == kSippRowWords) b[15] = static_cast<uint32_t>(sp.safe.size()) + 1u;  // a whole row: its last word is the count
    r += 1;
  };
  if (fresh) {
    for (int32_t cell = 0; cell < cells; ++cell)
      if (T.cellIdx[cell]) emit(cell);
    T.epoch = 0;
  } else {
    for (int32_t cell : T.dirty) emit(cell);
  }
  for (int32_t cell : T.dirty) T.isDirty[cell] = 0;
  T.dirty.clear();
  T.devFresh = false;
  T.epoch += 1;
  T.inFlight = true;
  const uint64_t addr = reinterpret_cast<uint64_t>(env.sippTabChunks[T.devIndex / env.sippTabsPerChunk]) +
                        static_cast<uint64_t>(T.devIndex % env.sippTabsPerChunk) * env.sippTabStride;
  d.algo = MRP_LL_SIPP;
  d.max_expansions = j.max_expansions;
  d.n_agents_pad = static_cast<uint32_t>(addr);
  d.path_off = static_cast<uint32_t>(addr >> 32);
  static const bool noLds = [] {
    const char* e = std::getenv("MRP_LL_SIPP_NO_LDS");  // tier comparison (tests, probes)
    return e && *e == '1';
  }();
  d.ctx_flags = kSippResident | (noLds ? kSippNoLds : 0u);
  d.n_ctx = T.epoch;
  d.n_vc = static_cast<uint32_t>(recIv);  // intervals per delta record
  d.n_ec = T.totalSafe;
  d.ec_off = static_cast<uint32_t>(nRec) | (fresh ? 0x80000000u : 0u);
  d.last_goal_constraint = startTime;
  // the start interval (findSafeInterval, sipp.hpp:286-296) is looked up by the workgroup: with sipp_commit the
  // device copy is ahead of this one
  d.t_pad = 0;
  if (j.sipp_commit) d.ctx_flags |= kSippCommit;
  return true;
}

template <class ConsSink>
static inline bool packSipp(const PackEnv& env, const mrp_ll_job& j, const MapRec& mp, ConsSink& cs, DevJob& d) {
  if (j.sipp_table) {
    const mrp_ll_sipp_table& T = *j.sipp_table;
    // resident form: in a session, for a table of this engine that fits the fixed layout (one job per table in flight)
    if (env.session.active && T.owner == env.owner && T.devIndex >= 0 && !T.overflow && !T.inFlight &&
        packSippResident(env, j, mp, cs, d))
      return true;
    return packSippFromTable(j, mp, cs, d);
  }
  const int cells = mp.dimx * mp.dimy;
  if (j.n_collision_locations < 0) return false;
  if (j.n_collision_locations > 0 && (!j.collision_xy || !j.collision_count || !j.collision_intervals)) return false;
  typedef SippScratch::Iv Iv;
  SippScratch& sc0 = env.sippScratch;
  std::vector<int32_t>& cellIdx = sc0.cellIdx;
  cellIdx.assign(cells, 0);
  sc0.first.clear();
  sc0.count.clear();
  sc0.pool.clear();
  size_t off = 0;
  for (int n = 0; n < j.n_collision_locations; ++n) {
    const int x = j.collision_xy[2 * n], y = j.collision_xy[2 * n + 1];
    const int cnt = j.collision_count[n];
    const int32_t* civ = j.collision_intervals + 2 * off;
    off += cnt;
    if (x < 0 || x >= mp.dimx || y < 0 || y >= mp.dimy) continue;  // never visited
    const int cell = y * mp.dimx + x;
    const uint32_t p0 = static_cast<uint32_t>(sc0.pool.size());
    if (cnt > 0) safeFromCollisions(civ, cnt, sc0.ci, sc0.pool);
    const uint32_t nSafe = static_cast<uint32_t>(sc0.pool.size()) - p0;
    // erase + re-create (sipp.hpp:247-251): an empty list restores the default single interval
    if (cellIdx[cell]) {
      const int k = cellIdx[cell] - 1;
      if (cnt == 0) {
        sc0.first[k] = static_cast<uint32_t>(sc0.pool.size());
        sc0.pool.push_back(Iv{0, INT32_MAX});
        sc0.count[k] = 1;
      } else {
        sc0.first[k] = p0;
        sc0.count[k] = nSafe;
      }
    } else if (cnt > 0) {
      sc0.first.push_back(p0);
      sc0.count.push_back(nSafe);
      cellIdx[cell] = static_cast<int32_t>(sc0.first.size());
    }
  }
  const uint32_t K = static_cast<uint32_t>(sc0.first.size());
  uint32_t total = 0;
  for (uint32_t k = 0; k < K; ++k) total += sc0.count[k];
  d.algo = MRP_LL_SIPP;
  d.max_expansions = j.max_expansions;
  d.vc_off = static_cast<uint32_t>(cs.size());
  {  // cellIdx[cells], specFirst[K + 1], ivals[total][2]
    const size_t cw = (static_cast<size_t>(cells) + 1) / 2;  // cellIdx travels as halfwords
    uint32_t* w = cs.grow(cw + K + 1 + 2 * static_cast<size_t>(total));
    if (!w) return false;
    w[cw - 1] = 0;
    uint16_t* w16 = reinterpret_cast<uint16_t*>(w);
    for (int c = 0; c < cells; ++c) w16[c] = static_cast<uint16_t>(cellIdx[c]);
    w += cw;
    uint32_t run = 0;
    for (uint32_t k = 0; k < K; ++k) {
      w[k] = run;
      run += sc0.count[k];
    }
    w[K] = run;
    w += K + 1;
    for (uint32_t k = 0; k < K; ++k) {
      if (sc0.count[k]) std::memcpy(w, sc0.pool.data() + sc0.first[k], sizeof(Iv) * sc0.count[k]);
      w += 2 * sc0.count[k];
    }
  }
  d.n_vc = K;
  d.n_ec = total;
  d.ec_off = 0;
  d.n_agents_pad = 0;
  d.path_off = 0;
  // SIPP::search(..., startTime) (sipp.hpp:92-103): carried in the field the A* kernels use for m_lastGoalConstraint
  const int32_t startTime = j.initial_cost;
  if (startTime > static_cast<int32_t>(kGMask)) return false;
  d.last_goal_constraint = startTime;
  const int sc = j.start_y * mp.dimx + j.start_x;
  const bool special = cellIdx[sc] != 0;
  d.t_pad = sippStartWord(special ? sc0.pool.data() + sc0.first[cellIdx[sc] - 1] : nullptr, special ? sc0.count[cellIdx[sc] - 1] : 0,
                          special, startTime);
  return !cs.failed;
}

// ---- the word formats of ll_device.h, one function each (packJob below; tests/support/emu_ll.cpp) ---------------------
// Vertex constraints [n][3] = t, x, y -> words t << 16 | y << 8 | x pushed to `cs`; one that can never match a generated
// state (outside the grid, t >= horizon) is dropped.  Returns setLowLevelContext's m_lastGoalConstraint (ecbs.cpp:264-274):
// the last vertex constraint on the goal cell — of ANY cell when the agent has no task (anyCell; cbs_ta.cpp:283-303).
template <class ConsSink>
static inline int packVertexWords(const int32_t* vc, int n, int dimx, int dimy, int horizon, int gx, int gy, bool anyCell, ConsSink& cs) {
  int lastGoal = -1;
  for (int i = 0; i < n; ++i) {
    const int32_t* v = vc + 3 * i;
    if (anyCell || (v[1] == gx && v[2] == gy)) lastGoal = std::max(lastGoal, v[0]);
    if (v[0] < 0 || v[0] >= horizon || v[1] < 0 || v[1] >= dimx || v[2] < 0 || v[2] >= dimy) continue;
    cs.push((static_cast<uint32_t>(v[0]) << 16) | (static_cast<uint32_t>(v[2]) << 8) | static_cast<uint32_t>(v[1]));  // t, y, x
  }
  return lastGoal;
}
// Edge constraints [n][5] = t, x1, y1, x2, y2 -> words t << 19 | cell << 3 | k (k: neighborIndexFromDelta); an edge between
// cells that are no neighbours, from outside the grid or at t >= horizon is dropped.
template <class ConsSink>
static inline void packEdgeWords(const int32_t* ec, int n, int dimx, int dimy, int horizon, ConsSink& cs) {
  for (int i = 0; i < n; ++i) {
    const int32_t* e = ec + 5 * i;
    const int k = neighborIndexFromDelta(e[3] - e[1], e[4] - e[2]);
    if (k < 0 || e[0] < 0 || e[0] >= horizon || e[1] < 0 || e[1] >= dimx || e[2] < 0 || e[2] >= dimy) continue;
    cs.push((static_cast<uint32_t>(e[0]) << 19) | (static_cast<uint32_t>(e[2] * dimx + e[1]) << 3) | static_cast<uint32_t>(k));
  }
}
// Rows of the focal table of a context: the longest path among the other agents (0: no table).
static inline int focalTableRows(int nAgents, int agentIdx, const int32_t* pathLen) {
  int tpad = 0;
  for (int a = 0; a < nAgents; ++a)
    if (a != agentIdx && pathLen[a] > 0) tpad = std::max(tpad, pathLen[a]);
  return tpad;
}
// Focal context: the time-major table tab[tpad][npad] of the other agents' cells (x | y << 8), each path extended by its
// last cell; the own column, an empty path's column and a state outside the grid hold kEmptyCell.
static inline void fillFocalTable(uint16_t* tab, int tpad, uint32_t npad, int nAgents, int agentIdx, const int32_t* pathLen,
                                  const int32_t* const* pathXy, int dimx, int dimy) {
  const uint16_t none = static_cast<uint16_t>(kEmptyCell);
  for (size_t q = 0; q < static_cast<size_t>(tpad) * npad; ++q) tab[q] = none;
  for (int a = 0; a < nAgents; ++a) {
    const int len = pathLen[a];
    if (a == agentIdx || len <= 0) continue;
    const int32_t* xy = pathXy[a];
    uint16_t cell = none;
    for (int tt = 0; tt < tpad; ++tt) {
      if (tt < len) {
        const int x = xy[2 * tt], y = xy[2 * tt + 1];
        cell = (x >= 0 && x < dimx && y >= 0 && y < dimy) ? static_cast<uint16_t>(x | (y << 8)) : none;
      }
      tab[static_cast<size_t>(tt) * npad + a] = cell;
    }
  }
}

// Pack one job; returns false if the job is rejected (MRP_LL_BAD_JOB).  `out` names the constraint set the job writes, if
// any: the caller commits it once the job has been accepted (commitSet).
// `const PackEnv&` means that no STATE of the engine changes here, not that nothing is written: a SIPP job uses
// env.sippScratch as its work space and a resident one updates the job's own mrp_ll_sipp_table.  One packJob at a time per
// env (the callers hold the submit path: one thread, or coMu).
template <class ConsSink, class PathSink>
static inline bool packJob(const PackEnv& env, const mrp_ll_job& j, const PackArgs& args, ConsSink& cs, PathSink& ps, DevJob& d,
                           PendingSet& out) {
  out.slot = -1;
  if (j.map_id < 0 || j.map_id >= static_cast<int32_t>(env.maps.size())) return false;
  const MapRec& mp = env.maps[j.map_id];
  if (j.algo != MRP_LL_ASTAR && j.algo != MRP_LL_ASTAR_EPS && j.algo != MRP_LL_SIPP && j.algo != MRP_LL_ASTAR_TA &&
      j.algo != MRP_LL_ASTAR_EPS_TA)
    return false;
  if (j.algo == MRP_LL_ASTAR_EPS && j.initial_cost != 0) return false;  // AStarEpsilon::search has no initialCost
  const bool epsTa = j.algo == MRP_LL_ASTAR_EPS_TA;
  // MRP_LL_ASTAR_EPS_TA serves ecbs_ta.hpp's calls only: no initial cost, no root chain, no tier hint (and, below, no
  // constraint set and no conflict scan: both ask for MRP_LL_ASTAR / MRP_LL_ASTAR_EPS); the path store as MRP_LL_ASTAR_EPS has it
  if (epsTa && (j.initial_cost != 0 || (j.flags & (MRP_LL_JOB_ROOT_CHAIN | MRP_LL_JOB_HEAVY)))) return false;
  if (j.initial_cost < 0 || j.initial_cost >= 0x40000000) return false;  // (bit 30 of the per-job word marks MRP_LL_ASTAR_TA, jobInitOf)
  // MRP_LL_JOB_TABLE_H (mrp_ll.h): h from a shortest-path table.  A plain search of the mixed kernels: none of the stores, hints
  // and scans, no one-algorithm session — refused, never run as a Manhattan search.
  const bool tableH = (j.flags & MRP_LL_JOB_TABLE_H) != 0 && (j.algo == MRP_LL_ASTAR || j.algo == MRP_LL_ASTAR_EPS);
  if (tableH) {
    if ((j.flags & (MRP_LL_JOB_STORE_RESULT | MRP_LL_JOB_ROOT_CHAIN | MRP_LL_JOB_HEAVY | MRP_LL_JOB_SCAN_CONFLICTS |
                    MRP_LL_JOB_SCAN_FROM_PARENT | MRP_LL_JOB_CONSTRAINT_SET)) != 0 || j.path_ids)
      return false;
    if (env.session.active && (env.session.sipp || env.session.kind != 0)) return false;
    if (j.heuristic_id < 0 || j.heuristic_id >= static_cast<int32_t>(env.heurs.size()) || env.heurs[j.heuristic_id].mapId != j.map_id)
      return false;
  }
  // The agent's set by its slot in the constraint store (mrp_ll.h mrp_ll_submit_sets): the arrays are the additions.
  const bool bySet = (j.flags & MRP_LL_JOB_CONSTRAINT_SET) != 0;
  const ConsSetRec* baseSet = nullptr;
  if (bySet) {
    const mrp_ll_constraint_ref* ref = args.ref;
    if (!ref || !env.consStoreSlots || (j.algo != MRP_LL_ASTAR && j.algo != MRP_LL_ASTAR_EPS) || (j.flags & MRP_LL_JOB_ROOT_CHAIN))
      return false;
    const int32_t nSets = static_cast<int32_t>(env.consStoreSlots);
    if (ref->base_set_id < -1 || ref->base_set_id >= nSets || ref->result_set_id < -1 || ref->result_set_id >= nSets) return false;
    // (a search that a front workgroup hands to a heavy one stages twice and must find the same base both times)
    if (ref->base_set_id >= 0 && ref->base_set_id == ref->result_set_id) return false;
    if (ref->base_set_id >= 0) {
      baseSet = &env.consSets[ref->base_set_id];
      if (!baseSet->written || baseSet->inFlight || baseSet->mapId != j.map_id || baseSet->gx != j.goal_x || baseSet->gy != j.goal_y)
        return false;
    }
  }
  const bool scan = (j.flags & MRP_LL_JOB_SCAN_CONFLICTS) != 0;
  const bool fromParent = (j.flags & MRP_LL_JOB_SCAN_FROM_PARENT) != 0;
  if (fromParent && (!scan || !args.base)) return false;  // only with a scan, and only through mrp_ll_submit_node
  if (scan) {
    // the conflicts of the node come back through mrp_ll_submit_scan's array alone, and the workgroup scans what it holds:
    // an A*-epsilon search whose context names EVERY other agent's path by its path-store slot (mrp_ll.h)
    if (!args.scanAllowed || j.algo != MRP_LL_ASTAR_EPS || (j.flags & MRP_LL_JOB_ROOT_CHAIN)) return false;
    if (!j.path_ids || !j.path_len || !env.pathStoreSlots || j.n_agents < 1 || j.agent_idx < 0 || j.agent_idx >= j.n_agents) return false;
    for (int a = 0; a < j.n_agents; ++a)
      if (a != j.agent_idx && (j.path_ids[a] < 0 || j.path_len[a] < 1)) return false;
    // from the parent: the searching agent's entry names the slot of the path this search REPLACES (mrp_ll.h)
    if (fromParent && (j.path_ids[j.agent_idx] < 0 || static_cast<uint32_t>(j.path_ids[j.agent_idx]) >= env.pathStoreSlots ||
                       j.path_len[j.agent_idx] < 1 || args.base->parent_count < 0 || args.base->clean_before < 0))
      return false;
  }
  if (j.flags & MRP_LL_JOB_ROOT_CHAIN) {  // the root step of an ECBS conflict tree as one job (mrp_ll.h; ll_device.h kCtxChain)
    const int n = j.n_agents, first = j.agent_idx;
    if (j.algo != MRP_LL_ASTAR_EPS || !env.session.active || env.session.sipp || env.session.kind != 1) return false;
    if (n < 1 || n > static_cast<int>(kChainMaxAgents) || first < 0 || first >= n) return false;
    if (!j.path_ids || !j.chain_starts_goals_xy || !env.pathStoreSlots || mp.dimx > 32 || mp.dimy > 32) return false;
    {  // what runChain (ll_jobs.h) needs of the session: the compact tier, room for its focal table in the window,
       // an arena slot that holds the cameFrom table and the (time, cell) bitmap, room for the output in the job's host area
      const uint32_t npad = static_cast<uint32_t>((n + 15) & ~15);
      if (env.ldsNodes == 0 || env.session.ldsPathBytes == 0 || kChainRows * npad * 2u > env.session.ldsPathBytes ||
          static_cast<uint64_t>(env.arenaNodes) * 16u < 64u * 1024u + 8192u ||
          static_cast<uint64_t>(n) * kChainEntryWords * 2u + static_cast<uint64_t>(n) * 64u > env.session.outStride)
        return false;
    }
    std::memset(&d, 0, sizeof(d));
    d.map_word_off = mp.wordOff;
    d.dimx = mp.dimx;
    d.dimy = mp.dimy;
    d.words_per_row = mp.wpr;
    d.algo = j.algo;
    d.w = j.w;
    d.max_expansions = j.max_expansions;
    d.last_goal_constraint = -1;
    d.ctx_flags = kCtxChain;
    d.n_ctx = static_cast<uint32_t>(n);
    d.t_pad = static_cast<uint32_t>(first);
    d.n_agents_pad = static_cast<uint32_t>((n + 15) & ~15);
    d.store_out_id = kNoStoreSlot;
    d.reserved = static_cast<uint32_t>(j.chain_count > 0 ? std::min(n, first + j.chain_count) : n);  // one past the last agent planned
    d.vc_off = static_cast<uint32_t>(cs.size());
    for (int a = 0; a < n; ++a) {
      const int32_t* q = j.chain_starts_goals_xy + 4 * a;
      if (q[0] < 0 || q[0] >= mp.dimx || q[1] < 0 || q[1] >= mp.dimy || q[2] < 0 || q[2] >= mp.dimx || q[3] < 0 || q[3] >= mp.dimy)
        return false;
      cs.push(static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16) |
              (static_cast<uint32_t>(q[3]) << 24));
    }
    for (int a = 0; a < n; ++a) {
      if (j.path_ids[a] < 0 || static_cast<uint32_t>(j.path_ids[a]) >= env.pathStoreSlots) return false;
      cs.push(static_cast<uint32_t>(j.path_ids[a]));
    }
    return !cs.failed;
  }
  auto inGrid = [&](int x, int y) { return x >= 0 && x < mp.dimx && y >= 0 && y < mp.dimy; };
  if (!inGrid(j.start_x, j.start_y)) return false;
  if (j.n_vertex_constraints < 0 || j.n_edge_constraints < 0 || j.n_agents < 0) return false;
  if (j.n_vertex_constraints > 0 && !j.vertex_constraints) return false;
  if (j.n_edge_constraints > 0 && !j.edge_constraints) return false;
  const int horizon = env.maxHorizon;
  std::memset(&d, 0, sizeof(d));
  d.map_word_off = mp.wordOff;
  d.dimx = mp.dimx;
  d.dimy = mp.dimy;
  d.words_per_row = mp.wpr;
  d.sx = j.start_x;
  d.sy = j.start_y;
  const bool taNoGoal = (j.algo == MRP_LL_ASTAR_TA || epsTa) && (j.flags & MRP_LL_JOB_NO_GOAL) != 0;
  // a goal outside the grid can never be reached; keep the reference behaviour (search until open is exhausted /
  // capped) by parking it on an unreachable coordinate that still fits the 8-bit fields only if in range
  if (!taNoGoal && !inGrid(j.goal_x, j.goal_y)) return false;
  d.gx = taNoGoal ? 0 : j.goal_x;
  d.gy = taNoGoal ? 0 : j.goal_y;
  d.algo = j.algo;
  d.w = j.w;
  d.max_expansions = j.max_expansions;
  if (j.algo == MRP_LL_SIPP) return packSipp(env, j, mp, cs, d);
  uint32_t heurOff = 0;
  if (j.algo == MRP_LL_ASTAR_TA || epsTa) {
    // (MRP_LL_ASTAR_TA: the compact tier serves what fits it — maps up to 32 x 32, 64 + 64 constraints —, the arena tier
    // the rest; MRP_LL_ASTAR_EPS_TA: arena tier only)
    if (j.initial_cost != 0) return false;
    if (!taNoGoal) {
      if (j.heuristic_id < 0 || j.heuristic_id >= static_cast<int32_t>(env.heurs.size()) ||
          env.heurs[j.heuristic_id].mapId != j.map_id)
        return false;
      heurOff = env.heurs[j.heuristic_id].wordOff;
    } else {
      d.ctx_flags |= kTaNoGoal;
    }
  }
  d.vc_off = static_cast<uint32_t>(cs.size());
  d.last_goal_constraint =
      packVertexWords(j.vertex_constraints, j.n_vertex_constraints, mp.dimx, mp.dimy, horizon, j.goal_x, j.goal_y, taNoGoal, cs);
  d.n_vc = static_cast<uint32_t>(cs.size()) - d.vc_off;
  d.ec_off = static_cast<uint32_t>(cs.size());  // == vc_off + n_vc: the kernels copy both lists as one run (stageConstraints)
  packEdgeWords(j.edge_constraints, j.n_edge_constraints, mp.dimx, mp.dimy, horizon, cs);
  d.n_ec = static_cast<uint32_t>(cs.size()) - d.ec_off;
  if (cs.failed) return false;
  if (bySet) {
    // n_vc / n_ec become the UNION's counts (the tier choices keep working), the last goal constraint the larger of the
    // base's and the additions'; base slot, base counts and result slot travel in pad_ (ll_device.h)
    const mrp_ll_constraint_ref& ref = *args.ref;
    const uint32_t bVc = baseSet ? baseSet->nVc : 0u, bEc = baseSet ? baseSet->nEc : 0u;
    if (static_cast<uint64_t>(bVc) + bEc + d.n_vc + d.n_ec > env.consStoreStride) return false;
    d.n_vc += bVc;
    d.n_ec += bEc;
    if (baseSet) d.last_goal_constraint = std::max(d.last_goal_constraint, baseSet->lastGoal);
    d.pad_[0] = baseSet ? static_cast<uint32_t>(ref.base_set_id) + 1u : 0u;
    d.pad_[1] = bVc | (bEc << 16);
    d.pad_[2] = ref.result_set_id >= 0 ? static_cast<uint32_t>(ref.result_set_id) + 1u : 0u;
    if (ref.result_set_id >= 0) {
      ConsSetRec& r = out.rec;
      r.nVc = d.n_vc; r.nEc = d.n_ec;
      r.lastGoal = d.last_goal_constraint;
      r.mapId = j.map_id; r.gx = j.goal_x; r.gy = j.goal_y;
      out.slot = ref.result_set_id;  // (the job may still be rejected below: the caller commits, commitSet)
    }
  }
  if (j.algo == MRP_LL_ASTAR_TA) {
    d.n_agents_pad = 0;
    d.t_pad = 0;
    d.path_off = heurOff;
    d.store_out_id = kNoStoreSlot;
    return true;
  }
  // focal context: time-major table of the other agents' cells, each path extended by its last cell
  d.n_agents_pad = 0;
  d.t_pad = 0;
  d.path_off = 0;
  d.heur_off = epsTa ? heurOff : 0;  // (MRP_LL_ASTAR_EPS_TA needs both: the heuristic table and the focal path table)
  if (tableH) {
    d.heur_off = env.heurs[j.heuristic_id].wordOff;
    d.ctx_flags |= kCtxTableH;
    d.algo = kAlgoTableH | static_cast<uint32_t>(j.algo);
  }
  if ((j.flags & MRP_LL_JOB_HEAVY) && j.algo == MRP_LL_ASTAR_EPS) d.ctx_flags |= kCtxHeavy;
  if ((j.flags & MRP_LL_JOB_TRY_LDS) && epsTa) d.ctx_flags |= kCtxTryLds;  // (a hint of this algorithm's; the others ignore it)
  // the result path also goes to a path-store slot only when the caller says so (a zero-initialised job names no slot)
  const bool storeResult = (j.flags & MRP_LL_JOB_STORE_RESULT) != 0;
  d.store_out_id = (storeResult && j.result_path_id >= 0 && static_cast<uint32_t>(j.result_path_id) < env.pathStoreSlots)
                       ? static_cast<uint32_t>(j.result_path_id)
                       : kNoStoreSlot;
  if (storeResult && d.store_out_id == kNoStoreSlot) return false;  // no such slot (or no store reserved)
  if ((j.algo == MRP_LL_ASTAR_EPS || epsTa) && j.n_agents > 0 && j.path_ids) {
    // f2: the CT node's paths by their path-store slots; the workgroup builds the table (ll_jobs.h runJob, ll_ta.h
    // runJobTaEps: path_off names the ids, heur_off the heuristic table)
    if (!j.path_len || !env.pathStoreSlots) return false;
    int tpad = 0;
    for (int a = 0; a < j.n_agents; ++a)
      if (a != j.agent_idx && j.path_len[a] > 0) {
        if (j.path_ids[a] < 0 || static_cast<uint32_t>(j.path_ids[a]) >= env.pathStoreSlots) return false;
        tpad = std::max(tpad, j.path_len[a]);
      }
    // The workgroup builds the table in LDS or in its arena slot's path area (MRP_LL_ASTAR_EPS_TA: there only); a table that fits neither (a caller's
    // path_len beyond max_horizon, a very wide solution) is refused here rather than written past the slot.
    if (tpad > horizon ||
        static_cast<uint64_t>(tpad) * ((static_cast<uint32_t>(j.n_agents) + 15u) & ~15u) * 2u > env.arenaPathsBytes)
      return false;
    if (tpad > 0) {
      d.path_off = static_cast<uint32_t>(cs.size());
      for (int a = 0; a < j.n_agents; ++a)
        cs.push(a != j.agent_idx && j.path_len[a] > 0 ? static_cast<uint32_t>(j.path_ids[a]) : kNoStoreSlot);
      if (fromParent) {
        // behind the ids, never among them (the search must not see its own agent's column): the replaced path's slot and
        // what the caller knows of the parent node (ll_device.h kCtxScanParent)
        cs.push(static_cast<uint32_t>(j.path_ids[j.agent_idx]));
        cs.push(static_cast<uint32_t>(args.base->parent_count));
        cs.push(static_cast<uint32_t>(args.base->clean_before));
        d.ctx_flags |= kCtxScanParent;
      }
      if (cs.failed) return false;
      d.ctx_flags |= kCtxById;
      d.n_ctx = static_cast<uint32_t>(j.n_agents);
      d.n_agents_pad = (static_cast<uint32_t>(j.n_agents) + 15u) & ~15u;
      d.t_pad = static_cast<uint32_t>(tpad);
    }
  } else if ((j.algo == MRP_LL_ASTAR_EPS || epsTa) && j.n_agents > 0) {
    if (!j.path_len || !j.path_xy) return false;
    for (int a = 0; a < j.n_agents; ++a)
      if (a != j.agent_idx && j.path_len[a] > 0 && !j.path_xy[a]) return false;
    const int tpad = focalTableRows(j.n_agents, j.agent_idx, j.path_len);
    if (tpad > 0) {
      const uint32_t npad = (static_cast<uint32_t>(j.n_agents) + 15u) & ~15u;
      uint32_t off = 0;
      uint16_t* tab = ps.alloc(static_cast<size_t>(tpad) * npad, off);
      if (!tab) return false;
      d.path_off = off;
      d.n_agents_pad = npad;
      d.t_pad = static_cast<uint32_t>(tpad);
      fillFocalTable(tab, tpad, npad, j.n_agents, j.agent_idx, j.path_len, j.path_xy, mp.dimx, mp.dimy);
    }
  }
  if (scan) {
    if (j.n_agents >= 2 && !(d.ctx_flags & kCtxById)) return false;
    d.ctx_flags |= kCtxScan;
    d.reserved = static_cast<uint32_t>(j.agent_idx);
  }
  return true;
}

// The job packed last has been accepted (ok) or not: only an accepted one creates its result set in the mirror.  slot /
// seq: what the collection of its result hands to setCollected.
static inline void commitSet(PackEnv& env, bool ok, const PendingSet& p, int32_t& slot, uint32_t& seq) {
  slot = -1;
  seq = 0;
  if (!ok || p.slot < 0) return;
  ConsSetRec& r = env.consSets[p.slot];
  r = p.rec;
  r.written = true;
  r.inFlight = true;
  r.seq = ++env.consSetSeq;
  slot = p.slot;
  seq = r.seq;
}
// The result of the job that wrote `slot` has been collected: later jobs may name the set as their base.
static inline void setCollected(PackEnv& env, int32_t slot, uint32_t seq) {
  if (slot < 0 || slot >= static_cast<int32_t>(env.consSets.size())) return;
  ConsSetRec& r = env.consSets[slot];
  if (r.seq == seq) r.inFlight = false;
}

// What the device runs in place of a rejected job: a trivially capped search.
static inline void trivialRejectedJob(const PackEnv& env, DevJob& d) {
  std::memset(&d, 0, sizeof(d));
  d.dimx = 1; d.dimy = 1; d.words_per_row = 1;
  d.map_word_off = env.maps.empty() ? 0 : env.maps[0].wordOff;
  d.gx = 0; d.gy = 0; d.algo = 0; d.last_goal_constraint = -1;
  d.max_expansions = 0;
}

}  // namespace host
}  // namespace mrp
