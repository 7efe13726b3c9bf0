// The MRP_HL_* environment knobs of a CBS / ECBS solve call (mrp_hl.h mrp_hl_solver_solve_stream): read here, once per
// call, into one record.  launch_plan.hpp decides with the first group, SessionWorker (ct_session.hpp) runs by the second.
// (MRP_HL_MAX_ENGINES and MRP_HL_TICKETS belong to mrp_hl_solver_create, MRP_HL_PIN to pinWorker, the MRP_HL_SIPP_* knobs
// to sipp_drivers.hpp.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace mrp_hl {

struct SolveKnobs {
  // ---- what the call launches and reserves (launch_plan.hpp) ----
  bool staticSplit = false;  // MRP_HL_STATIC_SPLIT (set): the fixed interleaved split instead of one pool of instances for all workers
  bool tierSet = false;      // MRP_HL_TIER="nodes,rows,pathBytes": the compact tier's geometry (CBS ignores the third field)
  int32_t tierNodes = 0, tierRows = 0, tierPathBytes = 0;
  int32_t heavyWgs = -1;         // MRP_HL_HEAVY_WGS: heavy workgroups over all engines (0: one launch; -1 unset: by agent count)
  int32_t sessionWgs = 0;        // MRP_HL_SESSION_WGS: resident front wavefronts per engine, at least 1 (0 unset: what fits)
  int32_t storeMaxAgents = 128;  // MRP_HL_STORE_MAX_AGENTS: largest conflict tree that uses the device path store
  int32_t pathSlots = -1;        // MRP_HL_PATH_SLOTS: slots of every engine's path store (0 = ship tables; -1 unset: by engine count)
  // MRP_HL_DEVICE_CONSTRAINTS=1 (session mode, CBS and ECBS): an agent's constraint set stays in the engine's constraint store —
  // a child's search names its parent's set by slot and ships the one constraint it adds (mrp_ll_submit_sets) instead of the
  // whole set.  Same results; off by default.
  bool deviceCons = false;
  int32_t consSlots = -1;  // MRP_HL_CONS_SLOTS: slots of every engine's constraint store (-1 unset: as many as the path store would have)
  int32_t consWords = 64;  // MRP_HL_CONS_WORDS: constraints a slot holds, 1..2048; a larger set ships flat
  // MRP_HL_FRONT_TABLES=memory|lds (ECBS sessions with heavy workgroups): where the front workgroups keep a search's focal path
  // table (mrp_ll.h mrp_ll_session_front_tables).  memory: the front window is the same 10 880 bytes for every agent count and
  // more searches fit a CU, each a little slower; lds: the table behind the window, as the tier choice sized it.  Same results.
  // Unset (-1): memory up to 64 agents — one pair of row loads per expansion; measured +4 % at ten agents, +4 … 13 % at fifty —,
  // lds beyond, where a row is two loads wide and the leg is bound by its dependent chains (a hundred agents: -2 … -8 %;
  // DESIGN.md section 5).
  int32_t frontTables = -1;
  int32_t workers = 0;     // MRP_HL_WORKERS: worker threads of the call, at least 1 (0 unset: what mrp_hl_solver_create was asked for)
  // ---- how a session worker runs (ct_session.hpp) ----
  // MRP_HL_SPEC=k, speculation width of the conflict-tree machines (ct_solver.hpp).  Default 2: measured on the shipped
  // 8x8 CBS inputs (scripts/spec_probe.py) one node of look-ahead halves the time of a small batch (agents8 0.74 -> 0.37 s,
  // agents10-12 1.78 -> 0.91 s) and wider windows give it back (their searches queue in front of the popped node's own);
  // ECBS pops a fresh child next almost every time, so looking ahead buys it 0-6 %.
  int32_t specWidth = 2;
  bool chainDebug = false;  // MRP_HL_CHAIN_DEBUG: one line per chain answer on stderr
  bool timing = false;      // MRP_HL_TIMING: where every worker's time went, on stderr
  bool rootChains = true;   // MRP_HL_ROOT_CHAIN=0: every root search is its own job (A/B; results are the same)
  bool rootFast = true;     // MRP_HL_ROOT_FAST=0: every instance goes through its conflict-tree machine (A/B; same results)
  int32_t chainChunk = 8;   // MRP_HL_CHAIN_CHUNK: searches per root-chain job of an instance with many agents
  // MRP_HL_CHAIN_CHUNK_FROM.  Between 33 and 63 agents the root step goes out one job per search: measured at fifty agents
  // every form of chain (whole, or in jobs of 4 / 8 / 16 searches) is 5-25 % slower than that, at a hundred agents jobs of
  // eight are 15 % faster (scripts/r4_run19.sh, r4_run20.sh)
  int32_t chainChunkFrom = 64;
  int64_t ringDepth = 0;    // MRP_HL_RING_DEPTH: searches published per worker at a time (0: twice its resident wavefronts)
  int32_t activeLimit = 0;  // MRP_HL_ACTIVE_LIMIT: instances a worker keeps active at a time (0: its fair share of the pool)
  // MRP_HL_DEVICE_SCAN=1 (ECBS with a path store): a child's conflicts come back with its low-level search
  // (mrp_ll_submit_scan) instead of being scanned here at commit and at pop time.  Same results; off by default.
  bool deviceScan = false;
  // MRP_HL_DEVICE_SCAN_INCREMENTAL=1 (ECBS with a path store, an engine that exports mrp_ll_submit_node): the same, and the
  // child's job also says what the parent's scan established — its conflict count, the time of the conflict it is split
  // on, the slot of the replaced path — so that the workgroup counts in linear work (MRP_LL_JOB_SCAN_FROM_PARENT).  Same
  // results; off by default; without the export the driver behaves as with the variable unset.
  bool deviceScanIncremental = false;

  static SolveKnobs read() {
    auto num = [](const char* name, int64_t dflt) {
      const char* e = std::getenv(name);
      return e ? std::atoll(e) : dflt;
    };
    auto i32 = [](const char* name, int32_t dflt) {
      const char* e = std::getenv(name);
      return e ? std::atoi(e) : dflt;
    };
    auto isSet = [](const char* name) { return std::getenv(name) != nullptr; };
    SolveKnobs k;
    k.staticSplit = isSet("MRP_HL_STATIC_SPLIT");
    if (const char* e = std::getenv("MRP_HL_TIER"))
      k.tierSet = std::sscanf(e, "%d,%d,%d", &k.tierNodes, &k.tierRows, &k.tierPathBytes) == 3;
    if (isSet("MRP_HL_HEAVY_WGS")) k.heavyWgs = std::max(0, i32("MRP_HL_HEAVY_WGS", 0));
    if (isSet("MRP_HL_SESSION_WGS")) k.sessionWgs = std::max(1, i32("MRP_HL_SESSION_WGS", 0));
    k.storeMaxAgents = i32("MRP_HL_STORE_MAX_AGENTS", 128);
    if (isSet("MRP_HL_PATH_SLOTS")) k.pathSlots = std::max(0, i32("MRP_HL_PATH_SLOTS", 0));
    k.deviceCons = num("MRP_HL_DEVICE_CONSTRAINTS", 0) != 0;
    if (isSet("MRP_HL_CONS_SLOTS")) k.consSlots = std::max(0, i32("MRP_HL_CONS_SLOTS", 0));
    k.consWords = std::max(1, std::min(2048, i32("MRP_HL_CONS_WORDS", 64)));
    if (const char* e = std::getenv("MRP_HL_FRONT_TABLES")) k.frontTables = (e[0] == 'l' || e[0] == 'L' || e[0] == '0') ? 0 : 1;
    if (isSet("MRP_HL_WORKERS")) k.workers = std::max(1, i32("MRP_HL_WORKERS", 0));
    k.specWidth = static_cast<int32_t>(std::max<int64_t>(1, num("MRP_HL_SPEC", 2)));
    k.chainDebug = isSet("MRP_HL_CHAIN_DEBUG");
    k.timing = isSet("MRP_HL_TIMING");
    k.rootChains = num("MRP_HL_ROOT_CHAIN", 1) != 0;
    k.rootFast = num("MRP_HL_ROOT_FAST", 1) != 0;
    k.chainChunk = static_cast<int32_t>(std::max<int64_t>(1, num("MRP_HL_CHAIN_CHUNK", 8)));
    k.chainChunkFrom = static_cast<int32_t>(num("MRP_HL_CHAIN_CHUNK_FROM", 64));
    k.ringDepth = std::max<int64_t>(0, num("MRP_HL_RING_DEPTH", 0));
    k.activeLimit = isSet("MRP_HL_ACTIVE_LIMIT") ? static_cast<int32_t>(std::max<int64_t>(1, num("MRP_HL_ACTIVE_LIMIT", 1))) : 0;
    k.deviceScan = num("MRP_HL_DEVICE_SCAN", 0) != 0;
    k.deviceScanIncremental = num("MRP_HL_DEVICE_SCAN_INCREMENTAL", 0) != 0;
    return k;
  }
};

// MRP_HL_TA_EPS_LDS=1 (mrp_hl_solve_ecbs_ta_batch, read once per call; off by default, same results): every
// MRP_LL_ASTAR_EPS_TA search the call sends as an ordinary job — the children's, and the roots' when they go out as dependent
// jobs — carries MRP_LL_JOB_TRY_LDS and starts in that search's LDS tier (mrp_ll.h).  Roots planned by the root kernels are
// not jobs and stay as they are.
struct TaEpsKnobs {
  bool tryLds = false;
  static TaEpsKnobs read() {
    TaEpsKnobs k;
    if (const char* e = std::getenv("MRP_HL_TA_EPS_LDS")) k.tryLds = std::atoi(e) != 0;
    return k;
  }
};

}  // namespace mrp_hl
