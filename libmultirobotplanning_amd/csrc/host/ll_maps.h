// The maps buffer: obstacle bitmaps (and the heuristic tables, ll_heur_host.h) on the host and their copy on the device.
#pragma once
#include "ll_ctx.h"

namespace {

// Room for `need` words in the device maps buffer.  When it has to grow, the words that live on the device only (the
// first mapsBase) move device to device: nothing on the host could restore a computed table.
int reserveMapsDev(mrp_ll_ctx* ctx, size_t need) {
  need = std::max<size_t>(need, 1);
  if (need <= ctx->mapsDevCap) return MRP_LL_SUCCESS;
  // all tickets must be idle before the maps buffer may move
  for (auto& t : ctx->tickets)
    if (t.inFlight) HIPCHK(ctx, hipEventSynchronize(t.evK1));
  const size_t ncap = std::max<size_t>(need * 2, 1u << 20);  // >= 4 MB: room for in-session uploads
  uint32_t* nd = nullptr;
  HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&nd), ncap * sizeof(uint32_t)));
  if (ctx->mapsDev && ctx->mapsBase) {
    // on the first ticket's stream, idle here (no session, every ticket waited for): a stream of its own would be one more
    // for the hardware queues the resident kernels of a later session are spread over
    hipStream_t st = ctx->tickets[0].stream;
    hipError_t e = hipMemcpyAsync(nd, ctx->mapsDev, ctx->mapsBase * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      (void)hipFree(nd);  // the old buffer stays in place
      ctx->err = std::string("maps buffer growth: ") + hipGetErrorString(e);
      return MRP_LL_E_DEVICE;
    }
  }
  if (ctx->mapsDev) HIPCHK(ctx, hipFree(ctx->mapsDev));
  ctx->mapsDev = nd;
  ctx->mapsDevCap = ncap;
  return MRP_LL_SUCCESS;
}

// Copies what has been uploaded since the last call — and only that — behind what the device already holds.
int syncMaps(mrp_ll_ctx* ctx) {
  if (ctx->mapWords.empty()) return MRP_LL_SUCCESS;
  int rc = reserveMapsDev(ctx, ctx->mapsBase + ctx->mapWords.size());
  if (rc != MRP_LL_SUCCESS) return rc;
  HIPCHK(ctx, hipMemcpy(ctx->mapsDev + ctx->mapsBase, ctx->mapWords.data(), ctx->mapWords.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
  ctx->mapsBase += ctx->mapWords.size();
  ctx->mapWords.clear();
  return MRP_LL_SUCCESS;
}

}  // namespace

extern "C" {

int mrp_ll_upload_map(mrp_ll_ctx* ctx, int32_t dimx, int32_t dimy, int32_t nObst, const int32_t* obstXY,
                      int32_t* mapId) {
  if (!ctx || !mapId || dimx <= 0 || dimy <= 0 || dimx > 255 || dimy > 255 || nObst < 0 || (nObst > 0 && !obstXY)) {
    if (ctx) ctx->err = "mrp_ll_upload_map: invalid argument (dimensions must be 1..255)";
    return MRP_LL_E_INVALID;
  }
  if (dimx * dimy > ctx->opt.max_cells) {
    ctx->err = "mrp_ll_upload_map: dimx*dimy exceeds mrp_ll_options.max_cells";
    return MRP_LL_E_INVALID;
  }
  MapRec m;
  m.dimx = dimx;
  m.dimy = dimy;
  m.wpr = (static_cast<uint32_t>(dimx * dimy) + 31u) / 32u;
  // Every bitmap starts on its own 128-byte line: a map uploaded while a resident kernel runs (below) must not share a
  // cache line with an older one — the kernels read obstacle words with plain cached loads, and an XCD's L2 may still
  // hold the line's previous contents (nothing invalidates it between jobs, ll_kernel.hip residentLoop).
  const size_t pending0 = ctx->mapWords.size();
  if (ctx->mapsBase + pending0 + 31u + m.wpr > UINT32_MAX) {
    ctx->err = "mrp_ll_upload_map: the maps buffer is full (2^32 words)";
    return MRP_LL_E_NOMEM;
  }
  while ((ctx->mapsBase + ctx->mapWords.size()) & 31u) ctx->mapWords.push_back(0);
  m.wordOff = static_cast<uint32_t>(ctx->mapsBase + ctx->mapWords.size());
  ctx->mapWords.resize(ctx->mapWords.size() + m.wpr, 0u);
  uint32_t* w = ctx->mapWords.data() + (m.wordOff - ctx->mapsBase);
  // cells past dimx*dimy in the last word are never addressed
  for (int i = 0; i < nObst; ++i) {
    int x = obstXY[2 * i], y = obstXY[2 * i + 1];
    if (x < 0 || x >= dimx || y < 0 || y >= dimy) continue;  // unreachable anyway (stateValid bounds, ecbs.cpp:500)
    uint32_t cell = static_cast<uint32_t>(y * dimx + x);
    w[cell >> 5] |= 1u << (cell & 31);
  }
  ctx->env.maps.push_back(m);
  ctx->maxWpr = std::max(ctx->maxWpr, m.wpr);
  if (ctx->env.session.active) {
    // a resident kernel is reading the maps buffer: it may be appended to, but neither moved nor re-laid-out
    // (a map wider than the session's LDS rows is served from the HBM tier until the next session)
    if (ctx->mapsBase + ctx->mapWords.size() > ctx->mapsDevCap) {
      ctx->env.maps.pop_back();
      ctx->mapWords.resize(pending0);
      ctx->err = "mrp_ll_upload_map: no room in the device map buffer during a session (upload maps before "
                 "mrp_ll_session_begin, or end the session first)";
      return MRP_LL_E_BUSY;
    }
    int rc = syncMaps(ctx);  // (no growth: checked above)
    if (rc != MRP_LL_SUCCESS) return rc;
  }
  *mapId = static_cast<int32_t>(ctx->env.maps.size()) - 1;
  return MRP_LL_SUCCESS;
}

int mrp_ll_sync_maps(mrp_ll_ctx* ctx) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (ctx->env.session.active) return MRP_LL_SUCCESS;  // in-session uploads are copied immediately
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return syncMaps(ctx);
}

int mrp_ll_release_maps(mrp_ll_ctx* ctx) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (engineBusy(ctx)) return MRP_LL_E_BUSY;
  ctx->env.maps.clear();
  ctx->env.heurs.clear();
  ctx->mapWords.clear();
  ctx->mapsBase = 0;  // nothing to copy; the device buffer (and its capacity) is kept for the next uploads
  ctx->env.consSets.assign(ctx->env.consSets.size(), ConsSetRec());  // every constraint set belonged to one of those maps
  return MRP_LL_SUCCESS;
}

}  // extern "C"
