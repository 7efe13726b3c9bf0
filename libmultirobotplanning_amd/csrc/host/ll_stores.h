// What lives on the device between jobs: the path store, the constraint store and the SIPP tables.
#pragma once
#include "ll_ctx.h"

namespace {
// Allocated as ordinary device memory.  A slot is written by one workgroup of a resident kernel and read by workgroups on
// other CUs / XCDs of the SAME launch.  Ordering is carried by the host (a reader's job is published only after the
// writer's completion was seen: the writer's stores sit in front of a system-scope release); the reader drops stale cached
// copies with one agent-scope acquire per job (ll_jobs.h runJob), so ordinary cached device memory is enough — and the
// paths of a conflict-tree node, read again by job after job, are served from L2.  MRP_LL_STORE_UNCACHED=1: uncached
// allocation instead (measured: agents100 steps 23 % longer — every table build then reads HBM).
int allocStore(mrp_ll_ctx* ctx, const char* who, size_t bytes, void** out) {
  hipError_t e = std::getenv("MRP_LL_STORE_UNCACHED") ? hipExtMallocWithFlags(out, bytes, hipDeviceMallocUncached)
                                                      : hipMalloc(out, bytes);
  if (e == hipSuccess) return MRP_LL_SUCCESS;
  ctx->err = std::string(who) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? MRP_LL_E_NOMEM : MRP_LL_E_DEVICE;
}
}  // namespace

extern "C" {

int mrp_ll_path_store_reserve(mrp_ll_ctx* ctx, int32_t nSlots) {
  if (!ctx || nSlots < 0) return MRP_LL_E_INVALID;
  if (engineBusy(ctx)) return MRP_LL_E_BUSY;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->pathStore) HIPCHK(ctx, hipFree(ctx->pathStore));
  ctx->pathStore = nullptr;
  ctx->env.pathStoreSlots = 0;
  if (nSlots == 0) return MRP_LL_SUCCESS;
  // [len][cells...]: one halfword in front of up to max_horizon states, rounded up to 16 bytes
  ctx->pathStoreStride = (static_cast<uint32_t>(ctx->env.maxHorizon) + 1u + 7u) & ~7u;
  const size_t bytes = static_cast<size_t>(nSlots) * ctx->pathStoreStride * sizeof(uint16_t);
  void* p = nullptr;
  int rc = allocStore(ctx, "mrp_ll_path_store_reserve", bytes, &p);
  if (rc != MRP_LL_SUCCESS) return rc;
  ctx->pathStore = static_cast<uint16_t*>(p);
  ctx->env.pathStoreSlots = static_cast<uint32_t>(nSlots);
  HIPCHK(ctx, hipMemset(ctx->pathStore, 0, bytes));
  return MRP_LL_SUCCESS;
}

int mrp_ll_constraint_store_reserve(mrp_ll_ctx* ctx, int32_t nSlots, int32_t wordsPerSlot) {
  if (!ctx || nSlots < 0 || wordsPerSlot < 0 || wordsPerSlot > static_cast<int32_t>(mrp::kConsLocalWords) ||
      (nSlots > 0 && wordsPerSlot == 0))
    return MRP_LL_E_INVALID;
  if (engineBusy(ctx)) return MRP_LL_E_BUSY;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->consStore) HIPCHK(ctx, hipFree(ctx->consStore));
  ctx->consStore = nullptr;
  ctx->env.consStoreSlots = 0;
  ctx->env.consStoreStride = 0;
  ctx->env.consSets.clear();
  if (nSlots == 0) return MRP_LL_SUCCESS;
  // (a slot is written by one workgroup and read by others of the same launch with agent-scope stores and loads; the host
  // orders them: a reader's job is accepted only after the writer's result has been collected)
  const size_t bytes = static_cast<size_t>(nSlots) * static_cast<size_t>(wordsPerSlot) * sizeof(uint32_t);
  void* p = nullptr;
  int rc = allocStore(ctx, "mrp_ll_constraint_store_reserve", bytes, &p);
  if (rc != MRP_LL_SUCCESS) return rc;
  ctx->consStore = static_cast<uint32_t*>(p);
  ctx->env.consStoreSlots = static_cast<uint32_t>(nSlots);
  ctx->env.consStoreStride = static_cast<uint32_t>(wordsPerSlot);
  ctx->env.consSets.assign(static_cast<size_t>(nSlots), ConsSetRec());
  HIPCHK(ctx, hipMemset(ctx->consStore, 0xFF, bytes));
  return MRP_LL_SUCCESS;
}

int mrp_ll_sipp_table_create(mrp_ll_ctx* ctx, int32_t mapId, mrp_ll_sipp_table** out) {
  if (!ctx || !out || mapId < 0 || mapId >= static_cast<int32_t>(ctx->env.maps.size())) return MRP_LL_E_INVALID;
  PackEnv& env = ctx->env;
  auto* t = new mrp_ll_sipp_table();
  t->mapId = mapId;
  t->dimx = env.maps[mapId].dimx;
  t->dimy = env.maps[mapId].dimy;
  t->cellIdx.assign(static_cast<size_t>(t->dimx) * t->dimy, 0);
  t->cellIdx16.assign(static_cast<size_t>(t->dimx) * t->dimy, 0);
  t->isDirty.assign(static_cast<size_t>(t->dimx) * t->dimy, 0);
  t->owner = ctx;
  // a slot of the device-resident table pool (grown by chunks; existing tables never move).  Failure to allocate is not
  // an error: such a table simply ships its whole contents with every job.
  if (env.sippTabStride == 0) {
    const size_t maxCells = static_cast<size_t>(ctx->opt.max_cells);
    env.sippTabStride = maxCells * mrp::kSippRowWords * 8;  // a bounds row and a status row per cell (ll_device.h)
    env.sippTabsPerChunk = static_cast<int32_t>(std::max<size_t>(1, std::min<size_t>(64, (size_t(64) << 20) / env.sippTabStride)));
  }
  if (!ctx->sippTabFree.empty()) {
    t->devIndex = ctx->sippTabFree.back();
    ctx->sippTabFree.pop_back();
  } else {
    if (ctx->sippTabNext == static_cast<int32_t>(env.sippTabChunks.size()) * env.sippTabsPerChunk) {
      // The device-resident SIPP tables live in uncached device memory: consecutive jobs of a table run on different XCDs, whose
      // L2s are not coherent with each other, so cached tables needed an acquire fence at every job start and a release at its
      // end (an invalidate / write-back of the XCD's whole L2, shared with ~190 other searches); uncached, every table access
      // goes to memory and no fence is needed.  Measured on the three prioritized-SIPP legs: 2-3 % faster per expansion.  The
      // cached form is gone: besides being slower, its commit test (sipp_commit with the fence pair per job) returned ONE
      // expansion count that differed from the oracle's in one of seven otherwise green runs in round 4 — never seen with
      // uncached tables — and a protocol that rests on L2 invalidates across XCDs is not worth keeping as an option nobody
      // measures.  A device without uncached allocations keeps no resident tables (jobs ship whole tables: same results).
      void* c = nullptr;
      if (hipSetDevice(ctx->device) == hipSuccess &&
          hipExtMallocWithFlags(&c, env.sippTabStride * env.sippTabsPerChunk, hipDeviceMallocUncached) == hipSuccess)
        env.sippTabChunks.push_back(static_cast<uint8_t*>(c));
    }
    if (ctx->sippTabNext < static_cast<int32_t>(env.sippTabChunks.size()) * env.sippTabsPerChunk) t->devIndex = ctx->sippTabNext++;
  }
  *out = t;
  return MRP_LL_SUCCESS;
}

int mrp_ll_sipp_table_add(mrp_ll_sipp_table* t, int32_t x, int32_t y, int32_t start, int32_t end) {
  if (!t) return MRP_LL_E_INVALID;
  if (x < 0 || x >= t->dimx || y < 0 || y >= t->dimy) return MRP_LL_SUCCESS;  // never visited
  if (!t->log.empty()) sippTableSync(t);
  sippTableAddCell(t, static_cast<size_t>(y) * t->dimx + x, start, end, true);
  return MRP_LL_SUCCESS;
}

void mrp_ll_sipp_table_destroy(mrp_ll_sipp_table* t) {
  if (!t) return;
  if (mrp_ll_ctx* ctx = static_cast<mrp_ll_ctx*>(t->owner)) {
    // a job on this table may still be in flight (its note reports back to the table, and with sipp_commit a workgroup
    // may still be writing the device copy): forget the note's reference, and do not hand the device copy to a new
    // table — its pool index is simply retired (0.8 MB of device memory per such destroy, until the engine goes)
    bool referenced = false;
    auto forget = [&](std::vector<JobNote>& notes) {
      for (JobNote& n : notes)
        if (n.table == t) {
          n.table = nullptr;
          referenced = true;
        }
    };
    forget(ctx->ring.notes);
    for (Ticket& tk : ctx->tickets) forget(tk.notes);
    if (t->devIndex >= 0 && !referenced && !t->inFlight) ctx->sippTabFree.push_back(t->devIndex);
  }
  delete t;
}

}  // extern "C"
