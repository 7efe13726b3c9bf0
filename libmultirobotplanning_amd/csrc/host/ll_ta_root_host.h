// mrp_ll_ta_root_batch: the roots of CBS-TA conflict trees, one workgroup each, in ONE launch of mrp_ll_ta_root_kernel
// (ll_ta_root.h).  The packer of ta_root_pack.h, the first ticket's staging buffers and stream (the engine is idle), the
// launch parameters of an ordinary MRP_LL_ASTAR_TA batch, unpackResult on the way back; the scan of a root whose table did
// not fit its arena slot is completed with mrp_ll_conflict_scan.
// mrp_ll_ta_root_batch_w: the same with roots of up to 256 agents and mrp_ll_ta_root_wide_kernel (ll_ta_root_wide.h).
#pragma once
#include "ll_batch.h"
#include "ll_ctx.h"
#include "ll_heur_host.h"
#include "ll_maps.h"
#include "ta_root_pack.h"

namespace {

int taRootLaunch(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts, bool wide) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = syncMaps(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = reserveMapsDev(ctx, 1);
  if (rc != MRP_LL_SUCCESS) return rc;
  Ticket& t = ctx->tickets[0];  // idle: no session, no batch in flight
  auto packT0 = std::chrono::steady_clock::now();
  mrp::host::TaRootStaging st;
  mrp::host::packTaRoots(ctx->env, n, roots, 0, st, wide ? mrp::kTaRootWideMaxAgents : mrp::kTaRootMaxAgents);
  const uint32_t outStride = static_cast<uint32_t>(ctx->env.maxHorizon) + mrp::kScanOutHalfs;
  const uint32_t nDev = static_cast<uint32_t>(st.recs.size());
  std::vector<int32_t> needScan;
  if (nDev == 0) {
    mrp::host::unpackTaRoots(ctx->stats, st, n, roots, nullptr, nullptr, outStride, planned, conflicts, needScan);
    return MRP_LL_SUCCESS;
  }
  t.jobs.clear();
  t.cons.clear();
  t.paths.clear();
  HIPCHK(ctx, t.jobs.resize(nDev));
  HIPCHK(ctx, t.cons.resize(std::max<size_t>(st.words.size(), 16)));
  HIPCHK(ctx, t.paths.reserve(16));
  HIPCHK(ctx, t.results.resize(st.nResults));
  HIPCHK(ctx, t.outPaths.resize(static_cast<size_t>(st.nResults) * outStride));
  std::memcpy(t.jobs.host, st.recs.data(), nDev * sizeof(DevJob));
  std::memcpy(t.cons.host, st.words.data(), st.words.size() * 4);
  mrp::host::blankTaRootAnswers(st, t.outPaths.host, outStride);
  ctx->stats.pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - packT0).count();
  ctx->stats.staged_bytes += static_cast<int64_t>(nDev * sizeof(DevJob) + st.words.size() * 4);

  mrp::LaunchParams P;
  std::memset(&P, 0, sizeof(P));
  P.jobs = t.jobs.dev;
  P.results = t.results.dev;
  P.out_paths = t.outPaths.dev;
  P.cons = t.cons.dev;
  P.paths = t.paths.dev;
  P.queue_base = t.queueBase;  // (the kernel takes no tickets)
  P.n_jobs = nDev;
  uint32_t ldsBytes = 0;
  rc = fillCommonParams(ctx, t, P, ldsBytes, 2);  // the A* kernels' window: what an MRP_LL_ASTAR_TA batch is launched with
  if (rc != MRP_LL_SUCCESS) return rc;
  const uint32_t grid = std::min<uint32_t>(nDev, static_cast<uint32_t>(ctx->opt.slots));
  HIPCHK(ctx, hipEventRecord(t.evK0, t.stream));
  HIPCHK(ctx, mrp_ll_launch_ta_root(&P, grid, ldsBytes, wide ? 1 : 0, t.stream));
  HIPCHK(ctx, hipEventRecord(t.evK1, t.stream));
  HIPCHK(ctx, hipEventSynchronize(t.evK1));
  ctx->stats.launches += 1;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, t.evK0, t.evK1) == hipSuccess) ctx->stats.kernel_ms += ms;

  auto unpackT0 = std::chrono::steady_clock::now();
  mrp::host::unpackTaRoots(ctx->stats, st, n, roots, t.results.host, t.outPaths.host, outStride, planned, conflicts, needScan);
  ctx->stats.unpack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - unpackT0).count();
  if (needScan.empty()) return MRP_LL_SUCCESS;
  // The roots whose table did not fit the slot's path area: one batch scan over the paths as the device returned them.
  std::vector<int32_t> setFirst(1, 0), pathFirst(1, 0), states;
  for (int32_t k : needScan) {
    for (int a = 0; a < roots[k].n_agents; ++a) {
      const uint32_t ri = st.firstResult[k] + static_cast<uint32_t>(a);
      const uint16_t* p = t.outPaths.host + static_cast<size_t>(ri) * outStride;
      const int32_t len = std::min<int32_t>(t.results.host[ri].n_states, ctx->env.maxHorizon);
      for (int32_t q = 0; q < len; ++q) {
        states.push_back(p[q] & 0xFF);
        states.push_back(p[q] >> 8);
      }
      pathFirst.push_back(static_cast<int32_t>(states.size() / 2));
    }
    setFirst.push_back(static_cast<int32_t>(pathFirst.size()) - 1);
  }
  std::vector<mrp_ll_conflict> found(needScan.size());
  rc = mrp_ll_conflict_scan(ctx, static_cast<int32_t>(needScan.size()), setFirst.data(), pathFirst.data(), states.data(), found.data());
  if (rc != MRP_LL_SUCCESS) return rc;
  for (size_t q = 0; q < needScan.size(); ++q) conflicts[needScan[q]] = found[q];
  return MRP_LL_SUCCESS;
}

}  // namespace

namespace {

int taRootBatch(mrp_ll_ctx* ctx, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts, bool wide) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (nRoots < 0 || (nRoots > 0 && (!roots || !planned || !conflicts))) {
    ctx->err = "mrp_ll_ta_root_batch: invalid argument";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_ta_root_batch: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (nRoots == 0) return MRP_LL_SUCCESS;
  const uint32_t maxAgents = wide ? mrp::kTaRootWideMaxAgents : mrp::kTaRootMaxAgents;
  mrp::host::blankTaRootOutputs(ctx->env, nRoots, roots, planned, conflicts, nullptr, maxAgents);
  const int rc = taRootLaunch(ctx, nRoots, roots, planned, conflicts, wide);
  if (rc != MRP_LL_SUCCESS) mrp::host::blankTaRootOutputs(ctx->env, nRoots, roots, planned, conflicts, nullptr, maxAgents);  // nothing half-told
  return rc;
}

}  // namespace

extern "C" {

int mrp_ll_ta_root_batch(mrp_ll_ctx* ctx, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts) {
  return taRootBatch(ctx, nRoots, roots, planned, conflicts, false);
}

int mrp_ll_ta_root_batch_w(mrp_ll_ctx* ctx, int32_t nRoots, const mrp_ll_ta_root* roots, int32_t* planned, mrp_ll_conflict* conflicts) {
  return taRootBatch(ctx, nRoots, roots, planned, conflicts, true);
}

}  // extern "C"
