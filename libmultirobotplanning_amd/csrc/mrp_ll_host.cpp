// C-ABI of the MI355X low-level search engine (include/mrp_ll.h).  The one host translation unit; its subjects live in
// headers under host/:
//   host/ll_pack.h          the packer (HIP-free: jobs -> device words), with host/ll_sipp_table.h (safe-interval tables)
//                           and host/ll_unpack.h (device results -> the caller's results)
//   host/ll_ctx.h           mrp_ll_ctx, tickets, the session ring, the per-job record and its collection
//   host/ll_maps.h          the maps buffer: uploads, copies to the device, release
//   host/ll_heur_host.h     heuristic tables (upload, compute, read, lookup) and the stand-alone conflict scan
//   host/ll_assign_host.h   min-cost task assignment and its next-best series, with host/assign_pack.h (HIP-free: problems
//                           -> device words and back) and host/assign_series.h (HIP-free: open list and partition)
//   host/ll_stores.h        path store, constraint store, SIPP tables
//   host/ll_batch.h         batch mode: launch parameters, submit, wait
//   host/ll_ta_root_host.h  the roots of CBS-TA and ECBS-TA conflict trees in one launch, one launcher for both, with
//                           host/ta_root_pack.h and host/ta_eps_root_pack.h (HIP-free: roots -> device words and back); a root
//                           whose table outgrew its slot is finished here with ordinary jobs and the stand-alone scan
//   host/ll_session.h       session mode: begin (allocation, reset, launch), end, heartbeat
//   host/ll_session_jobs.h  session mode: submit, poll, completion queue
//   host/ll_submit.h        the submit / poll / wait entry points
//   here                    create / destroy, tier configuration and geometry, statistics, version
// No CPU fallback: every entry point needs a working HIP device.
#include "host/ll_ctx.h"
#include "host/ll_maps.h"
#include "host/ll_heur_host.h"
#include "host/ll_assign_host.h"
#include "host/ll_stores.h"
#include "host/ll_batch.h"
#include "host/ll_ta_root_host.h"
#include "host/ll_session.h"
#include "host/ll_session_jobs.h"
#include "host/ll_submit.h"
#include "ll_slot.h"

namespace {
// Resident workgroups per CU when the runtime gives no answer: what the LDS window alone allows, 1 .. 16.
int occupancyByLds(uint32_t bytes) { return static_cast<int>(std::max<uint32_t>(1, std::min<uint32_t>(16, (160u * 1024u) / bytes))); }
}  // namespace

extern "C" {

const char* mrp_ll_version(void) { return "mrp_ll 0.1 (gfx950, HIP)"; }

const char* mrp_ll_last_error(const mrp_ll_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mrp_ll_create(const mrp_ll_options* optIn, mrp_ll_ctx** out) {
  if (!out) return MRP_LL_E_INVALID;
  *out = nullptr;
  mrp_ll_options o;
  std::memset(&o, 0, sizeof(o));
  if (optIn) o = *optIn;
  if (o.n_tickets <= 0) o.n_tickets = 4;
  if (o.slots <= 0) o.slots = 1024;
  if (o.arena_nodes <= 0) o.arena_nodes = 131072;
  if (o.arena_nodes > static_cast<int32_t>(mrp::kMaxArenaNodes)) o.arena_nodes = mrp::kMaxArenaNodes;
  o.arena_nodes &= ~1;
  if (o.max_horizon <= 0) o.max_horizon = 512;
  if (o.max_horizon > static_cast<int32_t>(mrp::kMaxHorizon)) o.max_horizon = mrp::kMaxHorizon;
  if (o.max_cells <= 0) o.max_cells = 4096;
  if (o.max_cells > 255 * 255) o.max_cells = 255 * 255;
  if (o.lds_nodes == 0) o.lds_nodes = mrp::kLdsMaxNodes;
  if (o.lds_nodes < 0) o.lds_nodes = 0;
  o.lds_nodes = std::min<int32_t>(o.lds_nodes, mrp::kLdsMaxNodes);  // the compact tier's open list holds lds_nodes / 2 entries
  o.lds_nodes &= ~3;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || o.device < 0 || o.device >= ndev) {
    return MRP_LL_E_DEVICE;  // no fallback: the engine is HIP-only
  }
  mrp_ll_ctx* ctx = new mrp_ll_ctx();
  ctx->opt = o;
  ctx->device = o.device;
  ctx->env.owner = ctx;
  ctx->env.maxHorizon = o.max_horizon;
  ctx->env.ldsNodes = o.lds_nodes;
  ctx->env.arenaNodes = o.arena_nodes;
  std::memset(&ctx->stats, 0, sizeof(ctx->stats));
  if (hipSetDevice(o.device) != hipSuccess) {
    delete ctx;
    return MRP_LL_E_DEVICE;
  }
  ctx->arenaRowWords = (static_cast<uint32_t>(o.max_cells) + 31u) / 32u;
  ctx->env.arenaPathsBytes = 128 * 1024;
  if (const char* e = std::getenv("MRP_LL_ARENA_PATHS_BYTES"))  // tuning knob (tests: a path area too small for a root's table)
    ctx->env.arenaPathsBytes = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 4096), 128 * 1024)) & ~255u;
  if (const char* e = std::getenv("MRP_LL_ASSIGN_LDS_BYTES"))  // tuning knob (tests: a small wide problem on memory rows)
    ctx->assignLdsBudget = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 0), static_cast<int>(mrp::as::kLdsBudgetWide)));
  ctx->arenaScratchOff = static_cast<uint32_t>(mrp::slot::scratchOff(o.arena_nodes, o.max_horizon, ctx->arenaRowWords));
  const uint64_t stride = mrp::slot::stride(o.arena_nodes, o.max_horizon, ctx->arenaRowWords, ctx->env.arenaPathsBytes);
  ctx->arenaStride = stride;
  ctx->tickets.resize(o.n_tickets);
  for (auto& t : ctx->tickets) {
    hipError_t e = hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&t.evK0);
    if (e == hipSuccess) e = hipEventCreate(&t.evK1);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t.queueHead), 256);
    if (e == hipSuccess) e = hipMemset(t.queueHead, 0, 256);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t.arena), stride * static_cast<uint64_t>(o.slots));
    if (e != hipSuccess) {
      ctx->err = std::string("mrp_ll_create: ") + hipGetErrorString(e);
      mrp_ll_destroy(ctx);
      return e == hipErrorOutOfMemory ? MRP_LL_E_NOMEM : MRP_LL_E_DEVICE;
    }
  }
  *out = ctx;
  return MRP_LL_SUCCESS;
}

void mrp_ll_destroy(mrp_ll_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->env.session.active) (void)mrp_ll_session_end(ctx);
  if (ctx->ring.ev0) (void)hipEventDestroy(ctx->ring.ev0);
  if (ctx->ring.ev1) (void)hipEventDestroy(ctx->ring.ev1);
  if (ctx->ring.ev2) (void)hipEventDestroy(ctx->ring.ev2);
  if (ctx->ring.stream2) (void)hipStreamDestroy(ctx->ring.stream2);
  if (ctx->ring.block) (void)hipHostFree(ctx->ring.block);
  if (ctx->ring.push) (void)(ctx->ring.pushInDevice ? hipFree(ctx->ring.push) : hipHostFree(ctx->ring.push));
  if (ctx->ring.sippCons) (void)hipHostFree(ctx->ring.sippCons);
  if (ctx->ring.compCountDev) (void)hipFree(ctx->ring.compCountDev);
  if (ctx->ring.heavyQ) (void)hipFree(ctx->ring.heavyQ);
  if (ctx->ring.heavyCtr) (void)hipFree(ctx->ring.heavyCtr);
  if (ctx->ring.heavyAlive) (void)hipHostFree(ctx->ring.heavyAlive);
  if (ctx->ring.ticksDev) (void)hipFree(ctx->ring.ticksDev);
  for (auto& t : ctx->tickets) {
    if (t.inFlight && t.evK1) (void)hipEventSynchronize(t.evK1);
    if (t.stream) (void)hipStreamSynchronize(t.stream);
    t.jobs.release();
    t.cons.release();
    t.paths.release();
    t.results.release();
    t.outPaths.release();
    if (t.queueHead) (void)hipFree(t.queueHead);
    if (t.arena) (void)hipFree(t.arena);
    if (t.evK0) (void)hipEventDestroy(t.evK0);
    if (t.evK1) (void)hipEventDestroy(t.evK1);
    if (t.stream) (void)hipStreamDestroy(t.stream);
  }
  if (ctx->mapsDev) (void)hipFree(ctx->mapsDev);
  if (ctx->scanDev) (void)hipFree(ctx->scanDev);
  if (ctx->heurEv0) (void)hipEventDestroy(ctx->heurEv0);
  if (ctx->heurEv1) (void)hipEventDestroy(ctx->heurEv1);
  if (ctx->scanStream) (void)hipStreamDestroy(ctx->scanStream);
  if (ctx->pathStore) (void)hipFree(ctx->pathStore);
  if (ctx->consStore) (void)hipFree(ctx->consStore);
  for (uint8_t* c : ctx->env.sippTabChunks) (void)hipFree(c);
  delete ctx;
}

int mrp_ll_configure_tiers(mrp_ll_ctx* ctx, int32_t ldsNodes, int32_t ldsRows, int32_t ldsPathBytes, int32_t* occOut) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (engineBusy(ctx)) return MRP_LL_E_BUSY;
  if (ldsNodes < 0) ctx->env.ldsNodes = 0;
  // the compact LDS tier holds up to 1023 open entries (lds_nodes / 2) and 64 time steps; its LDS window has a fixed size
  if (ldsNodes > 0) ctx->env.ldsNodes = std::max(8, std::min<int32_t>(ldsNodes, mrp::kLdsMaxNodes) & ~3);
  if (ldsRows > 0) ctx->tierRows = static_cast<uint32_t>(std::min(std::max(ldsRows, 8), 64));
  if (ldsPathBytes > 0) ctx->tierPathBytes = static_cast<uint32_t>(std::min(ldsPathBytes, 65536)) & ~31u;
  if (occOut) {
    const uint32_t rowWords = (ctx->maxWpr + 3u) & ~3u;
    const uint32_t bytes = ctx->env.ldsNodes
                               ? mrp_ll_lds_bytes(0, static_cast<uint32_t>(ctx->env.ldsNodes), ctx->tierRows, rowWords, ctx->tierPathBytes) + 256
                               : 0;
    *occOut = bytes ? occupancyByLds(bytes) : 16;
  }
  return MRP_LL_SUCCESS;
}

int mrp_ll_session_occupancy(mrp_ll_ctx* ctx, int32_t algo, int32_t* occOut) {
  if (!ctx || !occOut) return MRP_LL_E_INVALID;
  if (algo != MRP_LL_ASTAR && algo != MRP_LL_ASTAR_EPS && algo != MRP_LL_ASTAR_TA && algo != MRP_LL_SIPP) return MRP_LL_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (algo == MRP_LL_SIPP) {  // the resident SIPP kernel: a fixed LDS tier (ll_sipp.h MRP_LL_SIPP_LDS_NODES)
    const int occS = mrp_ll_sipp_persistent_occupancy();
    *occOut = occS > 0 ? std::min(occS, 32) : 6;
    return MRP_LL_SUCCESS;
  }
  const int kind = algo == MRP_LL_ASTAR_EPS ? 1 : 2;
  const uint32_t rowWords = (ctx->maxWpr + 3u) & ~3u;
  const uint32_t bytes = mrp_ll_lds_bytes(kind, static_cast<uint32_t>(ctx->env.ldsNodes), ctx->tierRows, rowWords,
                                          ctx->env.ldsNodes ? ctx->tierPathBytes : 0);
  int occ = mrp_ll_persistent_occupancy(kind, bytes);  // what the runtime grants this kernel with this much dynamic LDS
  if (occ <= 0) occ = occupancyByLds(bytes + 256u);
  *occOut = std::min(occ, 16);
  return MRP_LL_SUCCESS;
}

int mrp_ll_session_tiers_geometry(mrp_ll_ctx* ctx, int32_t* frontOcc, int32_t* frontLds, int32_t* heavyLds) {
  if (!ctx) return MRP_LL_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t rowWords = (ctx->maxWpr + 3u) & ~3u;
  // (mrp_ll_session_front_tables: the front window holds no table)
  const uint32_t bytes = mrp_ll_lds_bytes(1, static_cast<uint32_t>(ctx->env.ldsNodes), ctx->tierRows, rowWords,
                                          ctx->env.ldsNodes && !ctx->frontTablesInMemory ? ctx->tierPathBytes : 0);
  if (frontOcc) {
    int occ = mrp_ll_front_heavy_occupancy(ctx->env.ldsNodes && ctx->frontTablesInMemory ? 2 : 0, bytes);
    if (occ <= 0) occ = occupancyByLds(bytes + 256u);
    *frontOcc = std::min(occ, 16);
  }
  if (frontLds) *frontLds = static_cast<int32_t>(bytes);
  if (heavyLds) *heavyLds = static_cast<int32_t>(mrp_ll_heavy_lds_bytes());
  return MRP_LL_SUCCESS;
}

int mrp_ll_session_front_tables(mrp_ll_ctx* ctx, int32_t inMemory) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (engineBusy(ctx)) return MRP_LL_E_BUSY;
  ctx->frontTablesInMemory = inMemory != 0;
  return MRP_LL_SUCCESS;
}

int mrp_ll_get_stats(const mrp_ll_ctx* ctx, mrp_ll_stats* out) {
  if (!ctx || !out) return MRP_LL_E_INVALID;
  *out = ctx->stats;
  return MRP_LL_SUCCESS;
}

int mrp_ll_reset_stats(mrp_ll_ctx* ctx) {
  if (!ctx) return MRP_LL_E_INVALID;
  std::memset(&ctx->stats, 0, sizeof(ctx->stats));
  return MRP_LL_SUCCESS;
}

}  // extern "C"
