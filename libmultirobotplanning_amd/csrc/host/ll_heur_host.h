// Shortest-path heuristic tables (MRP_LL_ASTAR_TA / _EPS_TA): upload, computation on the device, read-back, lookup — and
// the stand-alone conflict scan, which shares their device staging.
#pragma once
#include "ll_ctx.h"
#include "ll_maps.h"

namespace {

// device staging of the table calls and of mrp_ll_conflict_scan: neither keeps anything there between calls
int reserveScanDev(mrp_ll_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->scanDevCap) return MRP_LL_SUCCESS;
  if (ctx->scanDev) HIPCHK(ctx, hipFree(ctx->scanDev));
  ctx->scanDev = nullptr;
  ctx->scanDevCap = 0;
  HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->scanDev), bytes * 2));
  ctx->scanDevCap = bytes * 2;
  return MRP_LL_SUCCESS;
}
int heurEvents(mrp_ll_ctx* ctx) {
  if (!ctx->heurEv0) HIPCHK(ctx, hipEventCreate(&ctx->heurEv0));
  if (!ctx->heurEv1) HIPCHK(ctx, hipEventCreate(&ctx->heurEv1));
  return MRP_LL_SUCCESS;
}
void heurKernelDone(mrp_ll_ctx* ctx) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ctx->heurEv0, ctx->heurEv1) == hipSuccess) ctx->stats.kernel_ms += ms;
  ctx->stats.launches += 1;
}
// The conflict scan's stream: one of its own, because the scan also runs beside a session's resident kernel.
int auxStream(mrp_ll_ctx* ctx, hipStream_t* out) {
  if (!ctx->scanStream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->scanStream, hipStreamNonBlocking));
  *out = ctx->scanStream;
  return MRP_LL_SUCCESS;
}

}  // namespace

extern "C" {

int mrp_ll_upload_heuristic(mrp_ll_ctx* ctx, int32_t mapId, const int32_t* dist, int32_t* heurId) {
  if (!ctx || !dist || !heurId || mapId < 0 || mapId >= static_cast<int32_t>(ctx->env.maps.size())) return MRP_LL_E_INVALID;
  if (ctx->env.session.active) return MRP_LL_E_BUSY;  // (the maps buffer may have to grow)
  const MapRec& mp = ctx->env.maps[mapId];
  if (ctx->mapsBase + ctx->mapWords.size() + 31u + heurTableWords(mp) > UINT32_MAX) return MRP_LL_E_NOMEM;
  while ((ctx->mapsBase + ctx->mapWords.size()) & 31u) ctx->mapWords.push_back(0);  // own 128-byte lines, as the bitmaps
  HeurRec h;
  h.mapId = mapId;
  h.wordOff = static_cast<uint32_t>(ctx->mapsBase + ctx->mapWords.size());
  // halfwords, 0xFFFF = unreachable (the reference's table holds INT_MAX there)
  const int stride = heurStride(mp);
  ctx->mapWords.resize(ctx->mapWords.size() + heurTableWords(mp), 0xFFFFFFFFu);
  uint16_t* t16 = reinterpret_cast<uint16_t*>(ctx->mapWords.data() + (h.wordOff - ctx->mapsBase));
  for (int y = 0; y < mp.dimy; ++y)
    for (int x = 0; x < mp.dimx; ++x) {
      const int32_t v = dist[y * mp.dimx + x];
      t16[y * stride + x] = (v < 0 || v > 0xFFFE) ? 0xFFFFu : static_cast<uint16_t>(v);
    }
  ctx->env.heurs.push_back(h);
  *heurId = static_cast<int32_t>(ctx->env.heurs.size()) - 1;
  return MRP_LL_SUCCESS;
}

int mrp_ll_compute_heuristics(mrp_ll_ctx* ctx, int32_t n, const int32_t* mapIds, const int32_t* goalsXY, int32_t* heurIds) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!mapIds || !goalsXY || !heurIds))) {
    ctx->err = "mrp_ll_compute_heuristics: invalid argument";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_compute_heuristics: a session is active or a batch is in flight (the maps buffer may have to grow)";
    return MRP_LL_E_BUSY;
  }
  const std::vector<MapRec>& maps = ctx->env.maps;
  for (int32_t k = 0; k < n; ++k) {
    if (mapIds[k] < 0 || mapIds[k] >= static_cast<int32_t>(maps.size())) {
      ctx->err = "mrp_ll_compute_heuristics: unknown map id";
      return MRP_LL_E_INVALID;
    }
    const MapRec& mp = maps[mapIds[k]];
    const int32_t gx = goalsXY[2 * k], gy = goalsXY[2 * k + 1];
    if (gx < 0 || gx >= mp.dimx || gy < 0 || gy >= mp.dimy) {
      ctx->err = "mrp_ll_compute_heuristics: goal outside its map";
      return MRP_LL_E_INVALID;
    }
  }
  if (n == 0) return MRP_LL_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the bitmaps the kernel reads must be on the device; after this the layout ends at mapsBase
  int rc = syncMaps(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  // the tables go behind everything else, each on its own 128-byte lines, and exist on the device only
  std::vector<mrp::hb::HeurJob> jobs(static_cast<size_t>(n));
  size_t off = (ctx->mapsBase + 31u) & ~size_t(31);
  uint32_t ldsBytes = 0;
  for (int32_t k = 0; k < n; ++k) {
    const MapRec& mp = maps[mapIds[k]];
    if (off + heurTableWords(mp) + 31u > UINT32_MAX) {
      ctx->err = "mrp_ll_compute_heuristics: the maps buffer is full (2^32 words)";
      return MRP_LL_E_NOMEM;
    }
    mrp::hb::HeurJob& j = jobs[k];
    j.mapOff = mp.wordOff;
    j.tabOff = static_cast<uint32_t>(off);
    j.dims = static_cast<uint32_t>(mp.dimx) | static_cast<uint32_t>(mp.dimy) << 8;
    j.goal = static_cast<uint32_t>(goalsXY[2 * k]) | static_cast<uint32_t>(goalsXY[2 * k + 1]) << 8;
    ldsBytes = std::max(ldsBytes, mrp::hb::ldsBytes(static_cast<uint32_t>(mp.dimx), static_cast<uint32_t>(mp.dimy)));
    off = (off + heurTableWords(mp) + 31u) & ~size_t(31);
  }
  rc = reserveMapsDev(ctx, off);
  if (rc != MRP_LL_SUCCESS) return rc;
  const size_t jobBytes = jobs.size() * sizeof(mrp::hb::HeurJob);
  rc = reserveScanDev(ctx, jobBytes);
  if (rc != MRP_LL_SUCCESS) return rc;
  hipStream_t st = ctx->tickets[0].stream;  // idle: no session, no batch in flight (engineBusy above)
  rc = heurEvents(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev, jobs.data(), jobBytes, hipMemcpyHostToDevice, st));
  mrp::HeurParams P;
  P.maps = ctx->mapsDev;
  P.jobs = reinterpret_cast<const mrp::hb::HeurJob*>(ctx->scanDev);
  P.n = static_cast<uint32_t>(n);
  HIPCHK(ctx, hipEventRecord(ctx->heurEv0, st));
  HIPCHK(ctx, mrp_ll_launch_heur_bfs(&P, ldsBytes, st));  // ONE launch, one wavefront per table
  HIPCHK(ctx, hipEventRecord(ctx->heurEv1, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  heurKernelDone(ctx);
  ctx->stats.staged_bytes += static_cast<int64_t>(jobBytes);
  for (int32_t k = 0; k < n; ++k) {
    ctx->env.heurs.push_back(HeurRec{mapIds[k], jobs[k].tabOff});
    heurIds[k] = static_cast<int32_t>(ctx->env.heurs.size()) - 1;
  }
  ctx->mapsBase = off;
  return MRP_LL_SUCCESS;
}

int mrp_ll_read_heuristic(mrp_ll_ctx* ctx, int32_t heurId, int32_t* dist) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (!dist || heurId < 0 || heurId >= static_cast<int32_t>(ctx->env.heurs.size())) {
    ctx->err = "mrp_ll_read_heuristic: invalid argument (NULL pointer or unknown heuristic id)";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_read_heuristic: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = syncMaps(ctx);  // an uploaded table is read back from where the searches read it
  if (rc != MRP_LL_SUCCESS) return rc;
  const HeurRec& h = ctx->env.heurs[heurId];
  const MapRec& mp = ctx->env.maps[h.mapId];
  std::vector<uint32_t> words(heurTableWords(mp));
  HIPCHK(ctx, hipMemcpy(words.data(), ctx->mapsDev + h.wordOff, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const uint16_t* t16 = reinterpret_cast<const uint16_t*>(words.data());
  const int stride = heurStride(mp);
  for (int y = 0; y < mp.dimy; ++y)
    for (int x = 0; x < mp.dimx; ++x) {
      const uint16_t v = t16[y * stride + x];
      dist[y * mp.dimx + x] = v == 0xFFFFu ? INT32_MAX : static_cast<int32_t>(v);
    }
  return MRP_LL_SUCCESS;
}

int mrp_ll_heuristic_lookup(mrp_ll_ctx* ctx, int32_t n, const int32_t* heurIds, const int32_t* cellsXY, int32_t* out) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!heurIds || !cellsXY || !out))) {
    ctx->err = "mrp_ll_heuristic_lookup: invalid argument";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_heuristic_lookup: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  std::vector<mrp::hb::LookupJob> jobs(static_cast<size_t>(n));
  for (int32_t k = 0; k < n; ++k) {
    if (heurIds[k] < 0 || heurIds[k] >= static_cast<int32_t>(ctx->env.heurs.size())) {
      ctx->err = "mrp_ll_heuristic_lookup: unknown heuristic id";
      return MRP_LL_E_INVALID;
    }
    const HeurRec& h = ctx->env.heurs[heurIds[k]];
    const MapRec& mp = ctx->env.maps[h.mapId];
    const int32_t x = cellsXY[2 * k], y = cellsXY[2 * k + 1];
    if (x < 0 || x >= mp.dimx || y < 0 || y >= mp.dimy) {
      ctx->err = "mrp_ll_heuristic_lookup: cell outside its map";
      return MRP_LL_E_INVALID;
    }
    jobs[k].tabOff = h.wordOff;
    jobs[k].half = static_cast<uint32_t>(y * heurStride(mp) + x);
  }
  if (n == 0) return MRP_LL_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = syncMaps(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  const size_t jobBytes = (jobs.size() * sizeof(mrp::hb::LookupJob) + 255) & ~size_t(255), outBytes = static_cast<size_t>(n) * 4;
  rc = reserveScanDev(ctx, jobBytes + outBytes);
  if (rc != MRP_LL_SUCCESS) return rc;
  hipStream_t st = ctx->tickets[0].stream;  // idle: no session, no batch in flight (engineBusy above)
  rc = heurEvents(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev, jobs.data(), jobs.size() * sizeof(mrp::hb::LookupJob), hipMemcpyHostToDevice, st));
  mrp::LookupParams P;
  P.maps = ctx->mapsDev;
  P.jobs = reinterpret_cast<const mrp::hb::LookupJob*>(ctx->scanDev);
  P.out = reinterpret_cast<int32_t*>(ctx->scanDev + jobBytes);
  P.n = static_cast<uint32_t>(n);
  HIPCHK(ctx, hipEventRecord(ctx->heurEv0, st));
  HIPCHK(ctx, mrp_ll_launch_heur_lookup(&P, st));
  HIPCHK(ctx, hipEventRecord(ctx->heurEv1, st));
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->scanDev + jobBytes, outBytes, hipMemcpyDeviceToHost, st));  // n words, no table moves
  HIPCHK(ctx, hipStreamSynchronize(st));
  heurKernelDone(ctx);
  return MRP_LL_SUCCESS;
}

int mrp_ll_conflict_scan(mrp_ll_ctx* ctx, int32_t nSets, const int32_t* setFirstAgent, const int32_t* pathFirstState,
                         const int32_t* statesXY, mrp_ll_conflict* out) {
  if (!ctx || nSets < 0 || (nSets > 0 && (!setFirstAgent || !pathFirstState || !out))) return MRP_LL_E_INVALID;
  if (nSets == 0) return MRP_LL_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t nAgents = setFirstAgent[nSets];
  if (setFirstAgent[0] != 0 || nAgents < 0) return MRP_LL_E_INVALID;
  for (int32_t s = 0; s < nSets; ++s)
    if (setFirstAgent[s + 1] < setFirstAgent[s] || setFirstAgent[s + 1] - setFirstAgent[s] > 65535) return MRP_LL_E_INVALID;
  const int64_t nStates = nAgents ? pathFirstState[nAgents] : 0;
  if (nAgents && (pathFirstState[0] != 0 || !statesXY)) return MRP_LL_E_INVALID;
  for (int64_t a = 0; a < nAgents; ++a)
    if (pathFirstState[a + 1] <= pathFirstState[a]) {  // getState asserts a non-empty path (ecbs.cpp:491)
      ctx->err = "mrp_ll_conflict_scan: every path needs at least one state";
      return MRP_LL_E_INVALID;
    }
  ctx->scanStates.resize(static_cast<size_t>(nStates));
  for (int64_t k = 0; k < nStates; ++k) {
    const int32_t x = statesXY[2 * k], y = statesXY[2 * k + 1];
    if (x < 0 || x > 255 || y < 0 || y > 255) {
      ctx->err = "mrp_ll_conflict_scan: coordinates must be 0..255";
      return MRP_LL_E_INVALID;
    }
    ctx->scanStates[k] = static_cast<uint16_t>(x | (y << 8));
  }
  auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
  const size_t oSet = 0, oPath = al((nSets + 1) * 4), oStates = oPath + al((nAgents + 1) * 4),
               oOut = oStates + al(static_cast<size_t>(nStates) * 2), total = oOut + al(sizeof(mrp_ll_conflict) * nSets);
  int rc = reserveScanDev(ctx, total);
  if (rc != MRP_LL_SUCCESS) return rc;
  // A stream of its own (non-blocking): during a session tickets[0].stream is held by the resident kernel until
  // mrp_ll_session_end, and a scan queued behind it would never start (while its caller, blocked here, stops moving the
  // session's heartbeat).  The scan kernel runs beside the resident wavefronts: they leave wave slots and registers free.
  hipStream_t st = nullptr;
  if (auxStream(ctx, &st) != MRP_LL_SUCCESS) return MRP_LL_E_DEVICE;
  HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev + oSet, setFirstAgent, (nSets + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev + oPath, pathFirstState, (nAgents + 1) * 4, hipMemcpyHostToDevice, st));
  if (nStates)
    HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev + oStates, ctx->scanStates.data(), static_cast<size_t>(nStates) * 2,
                               hipMemcpyHostToDevice, st));
  mrp::ConflictParams P;
  P.setFirstAgent = reinterpret_cast<const uint32_t*>(ctx->scanDev + oSet);
  P.pathFirstState = reinterpret_cast<const uint32_t*>(ctx->scanDev + oPath);
  P.states = reinterpret_cast<const uint16_t*>(ctx->scanDev + oStates);
  P.out = reinterpret_cast<mrp::ConflictOut*>(ctx->scanDev + oOut);
  P.nSets = static_cast<uint32_t>(nSets);
  HIPCHK(ctx, mrp_ll_launch_conflict(&P, st));
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->scanDev + oOut, sizeof(mrp_ll_conflict) * nSets, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return MRP_LL_SUCCESS;
}

}  // extern "C"
