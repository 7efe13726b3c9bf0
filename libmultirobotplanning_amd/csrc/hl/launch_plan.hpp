// What a CBS / ECBS solve call (mrp_hl.h mrp_hl_solver_solve_stream) decides before it starts its worker threads, as plain
// data and pure functions: nothing here calls the engine or reads the environment, so every branch can be exercised
// without a solve.  The engine is asked in two rounds — its occupancy and tier geometry depend on the tiers configured
// first — so the plan comes in two steps: tierChoice(), then residency() from what the engine reported.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../../include/mrp_hl.h"
#include "solve_knobs.hpp"

namespace mrp_hl {

struct LaunchInput {
  int32_t algo = MRP_HL_ECBS, mode = 0;  // mrp_hl_options
  int32_t nEngines = 1;                  // engines of this call: those that hold every batch's maps, at most one per instance
  int32_t workersAsked = 1;              // host worker threads mrp_hl_solver_create was asked for
  int32_t nInst = 0, maxAgents = 1;      // instances of the call, agents of the largest one
  int32_t slots = 512, ldsNodes = 0;     // mrp_ll_options: job slots per engine; 0 = the call picks the tier geometry, < 0 = no LDS tier
  bool engineHasConstraintStore = false;
  SolveKnobs knobs;
  bool session() const { return mode != 1; }                  // (mode 1: the round-based schedule launches nothing resident)
  bool sharedPool() const { return !knobs.staticSplit; }      // one pool of instances for all workers
};

// LDS tier sized for two resident searches per SIMD (8 per CU): one wavefront alone leaves about half of its SIMD's
// issue slots idle (waiting on LDS / memory), a second one fills them.  The focal path table of a search is
// [time][agents rounded up to 16] halfwords; 64 time steps of it are kept in LDS, the rest of a longer table lives in
// the search's arena slot.
struct TierChoice {
  bool configure = false;  // the caller did not choose a geometry: mrp_ll_configure_tiers(nodes, rows, pathBytes) on every engine
  int32_t nodes = 2048, rows = 64;  // the compact tier at its full size (open list: nodes / 2 entries)
  int32_t pathBytes = 32;
  bool askGeometry = false;  // ECBS with an LDS tier: mrp_ll_session_tiers_geometry decides the heavy workgroups
};
inline TierChoice tierChoice(const LaunchInput& in) {
  TierChoice t;
  const bool ecbs = in.algo == MRP_HL_ECBS;
  t.configure = in.ldsNodes == 0 && in.session();
  const int32_t agentsPad = (in.maxAgents + 15) & ~15;
  if (ecbs) t.pathBytes = std::min(16384, std::max(2048, agentsPad * 2 * 64));
  if (in.knobs.tierSet) {
    t.nodes = in.knobs.tierNodes;
    t.rows = in.knobs.tierRows;
    if (ecbs) t.pathBytes = in.knobs.tierPathBytes;
  }
  t.askGeometry = ecbs && in.session() && in.ldsNodes >= 0;
  return t;
}

// What the engine answered after the tiers were configured.
struct EngineReport {
  int32_t occupancy = 4;  // mrp_ll_configure_tiers / mrp_ll_session_occupancy: resident workgroups per CU of this call's kernels
  int32_t frontOcc = 0, frontLds = 0, heavyLds = 0;  // mrp_ll_session_tiers_geometry (frontOcc 0: not asked, or it failed)
};

struct Residency {
  int32_t sessionWgs = 0;  // resident (front) wavefronts per engine
  int32_t heavyPer = 0;    // ECBS: heavy workgroups per engine (0: one launch serves all)
  bool pathStore = false;  // this call sizes the engines' path stores (else they stay as they are, unused)
  int32_t pathSlots = 0;   // ... with this many slots each (0: jobs ship their context as tables)
  bool consStore = false;  // this call sizes the engines' constraint stores (else they stay as they are, unused)
  int32_t consSlots = 0, consWords = 0;
  int32_t nWork = 1;       // worker threads
};
inline Residency residency(const LaunchInput& in, const EngineReport& rep) {
  Residency r;
  const int32_t nRun = in.nEngines;
  const bool ecbs = in.algo == MRP_HL_ECBS;
  // resident wavefronts per engine: the chip holds 256 CUs x `occupancy` workgroups of this kernel at once
  r.sessionWgs = std::max(16, std::min<int32_t>(in.slots, (256 * rep.occupancy) / nRun));
  // ECBS: some of the device's LDS goes to heavy workgroups (wide LDS tier + arena tier: the searches that outgrow the
  // front tier — 6 % of the expansions at ten agents, 17 % at a hundred, scripts/search_stats.py).  One takes the LDS of
  // `displaced` front workgroups; five eighths / three quarters / all of the CUs get one.
  if (tierChoice(in).askGeometry && rep.frontOcc > 0 && rep.frontLds > 0) {
    // (measured, eight workers: ten agents 160 > 192 > 128 > 256; fifty 192 > 256 > 128; a hundred 256)
    int32_t heavyTotal = in.maxAgents <= 16 ? 160 : in.maxAgents <= 64 ? 192 : 256;
    if (in.knobs.heavyWgs >= 0) heavyTotal = in.knobs.heavyWgs;
    r.heavyPer = heavyTotal / nRun + (heavyTotal % nRun ? 1 : 0);
    if (r.heavyPer > 0) {
      const int32_t granule = 512;  // LDS allocation granularity
      // (a window beyond 32 KB takes room as if it had 64 KB — measured, ll_compact.h MRP_CT_WIDE_GROUPS)
      const int32_t fl = (rep.frontLds + granule - 1) / granule * granule;
      const int32_t hl = rep.heavyLds > 32768 ? 65536 : (rep.heavyLds + granule - 1) / granule * granule;
      const int32_t cuLds = 160 * 1024;
      const int32_t frontPerCu = std::min(rep.frontOcc, cuLds / fl);
      const int32_t frontBeside = std::max(0, (cuLds - hl) / fl);  // front workgroups on a CU that hosts a heavy one
      // (beyond five heavy workgroups per eight CUs some CUs get two, and the second one costs more: measured, 192 / 224 /
      // 256 of them displace 3.6 front workgroups each, 160 exactly 3)
      const int32_t displaced = std::max(0, frontPerCu - frontBeside) + (r.heavyPer * nRun > 160 ? 1 : 0);
      const int32_t frontTotal = 256 * frontPerCu - displaced * r.heavyPer * nRun;
      // (never more than fits: a grid the device cannot place completely blocks its hardware pipe, and a launch queued
      // behind it — another worker's front workgroups — does not start until a resident kernel ends)
      r.sessionWgs = std::max(16, std::min<int32_t>(in.slots - r.heavyPer, frontTotal / nRun - 2));
      if (r.sessionWgs + r.heavyPer > in.slots || frontTotal <= 0) r.heavyPer = 0;  // (tiny engines: one launch serves all)
    }
  }
  if (in.knobs.sessionWgs > 0) r.sessionWgs = in.knobs.sessionWgs;
  // every live conflict-tree node of every active instance holds one slot per replaced path: a worker with 16384
  // active instances (few threads, big batch) needs millions of them, and a slot is max_horizon halfwords
  const int32_t slotsPerEngine = std::max(1 << 18, std::min(1 << 22, (1 << 22) / std::max(nRun, 1)));
  // f2: the engines' device-resident path stores (ECBS only: CBS's low level has no focal context).  A search leaves its
  // path there, and later jobs name the paths of their CT node by slot instead of shipping a [t][agent] table.
  // Used for conflict trees of up to 128 agents (MRP_HL_STORE_MAX_AGENTS; beyond that a table row no longer fits the
  // kernel's two 64-lane row loads and the job ships its table): bytes staged per search 1134 -> 134 (10 agents),
  // 5900 -> 303 (50), 12 087 -> 572 (100); steps 7 % / 3 % / 2 % faster.
  r.pathStore = ecbs && in.session() && in.maxAgents <= in.knobs.storeMaxAgents;
  if (r.pathStore) r.pathSlots = in.knobs.pathSlots >= 0 ? in.knobs.pathSlots : slotsPerEngine;
  // MRP_HL_DEVICE_CONSTRAINTS=1: the engines' device-resident constraint stores.  A live conflict-tree node holds one set
  // slot per constraint it added, as it holds one path slot per path it replaced, so the store has as many slots as the
  // path store would; a set of more than MRP_HL_CONS_WORDS constraints (default 64: 256 bytes a slot, 64 MiB to 1 GiB per
  // engine) ships flat.  Engines without the calls (weak references) leave the switch off.
  r.consStore = in.session() && in.knobs.deviceCons && in.engineHasConstraintStore;
  if (r.consStore) {
    r.consSlots = in.knobs.consSlots >= 0 ? in.knobs.consSlots : slotsPerEngine;
    r.consWords = in.knobs.consWords;
  }
  // session mode with the shared pool: worker threads beyond the engines join them as co-workers, two per engine
  r.nWork = nRun;
  if (in.session() && in.sharedPool()) {
    const int32_t want = in.knobs.workers > 0 ? in.knobs.workers : in.workersAsked;
    r.nWork = std::max(nRun, std::min(want, 2 * nRun));
    r.nWork = std::min(r.nWork, std::max(nRun, in.nInst));
  }
  return r;
}

}  // namespace mrp_hl
