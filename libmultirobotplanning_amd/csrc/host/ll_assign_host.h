// Min-cost task assignment (mrp_ll_assign_batch) and its next-best series (mrp_ll_assign_series_*): the packer of
// assign_pack.h, ONE launch of the assignment kernel per call, the series logic of assign_series.h with that launch as
// its solver.  Shares the table calls' device staging (ll_heur_host.h).  The wide calls (mrp_ll_assign_batch_w,
// mrp_ll_assign_series_create_w: up to 256 x 256) are the same with the wide packer and the wide kernel; a series step
// launches once for its narrow children and once for its wide ones.
#pragma once
#include "assign_pack.h"
#include "assign_series.h"
#include "ll_ctx.h"
#include "ll_heur_host.h"
#include "ll_maps.h"

namespace {

// One launch over staged problems: the job records and the data words go up, `launch` runs the kernel on the device
// pointers (jobs, data, out), the first outWords words of the result area come back into ctx->assignOut.  The result
// area has `scratchWords` more words behind them.  The caller has checked that the engine is idle.
template <class Launch>
int assignRun(mrp_ll_ctx* ctx, const void* jobs, size_t jobBytes, size_t nJobs, const std::vector<uint32_t>& data, uint32_t outWords,
              uint64_t scratchWords, const Launch& launch) {
  auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
  const size_t dataBytes = data.size() * 4, outBytes = static_cast<size_t>(outWords) * 4;
  if (data.size() > UINT32_MAX || nJobs > INT32_MAX || outWords + scratchWords > UINT32_MAX) {
    ctx->err = "mrp_ll_assign_batch: the batch is too large for one launch (2^32 staged words)";
    return MRP_LL_E_NOMEM;
  }
  const size_t oData = al(jobBytes), oOut = oData + al(dataBytes), total = oOut + al(outBytes + static_cast<size_t>(scratchWords) * 4);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = syncMaps(ctx);  // the gather form reads tables where the searches read them
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = reserveMapsDev(ctx, 1);  // (a batch without any table still hands the kernel a valid pointer)
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = reserveScanDev(ctx, total);
  if (rc != MRP_LL_SUCCESS) return rc;
  rc = heurEvents(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  hipStream_t stream = ctx->tickets[0].stream;  // idle: no session, no batch in flight
  HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev, jobs, jobBytes, hipMemcpyHostToDevice, stream));
  if (dataBytes) HIPCHK(ctx, hipMemcpyAsync(ctx->scanDev + oData, data.data(), dataBytes, hipMemcpyHostToDevice, stream));
  ctx->assignOut.resize(outWords);
  HIPCHK(ctx, hipEventRecord(ctx->heurEv0, stream));
  HIPCHK(ctx, launch(ctx->scanDev, reinterpret_cast<const uint32_t*>(ctx->scanDev + oData), reinterpret_cast<uint32_t*>(ctx->scanDev + oOut),
                     stream));  // ONE launch, one wavefront per problem
  HIPCHK(ctx, hipEventRecord(ctx->heurEv1, stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->assignOut.data(), ctx->scanDev + oOut, outBytes, hipMemcpyDeviceToHost, stream));
  HIPCHK(ctx, hipStreamSynchronize(stream));
  heurKernelDone(ctx);
  ctx->stats.staged_bytes += static_cast<int64_t>(jobBytes + dataBytes);
  return MRP_LL_SUCCESS;
}

// The staged problems of `results` (packAssignBatch) in one launch.  The caller has checked the arguments and that the
// engine is idle.
int assignLaunch(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results) {
  mrp::host::AssignStaging& st = ctx->assignStaging;
  mrp::host::packAssignBatch(ctx->env, n, problems, results, st);
  if (st.jobs.empty()) return MRP_LL_SUCCESS;
  const int rc = assignRun(ctx, st.jobs.data(), st.jobs.size() * sizeof(mrp::as::AssignJob), st.jobs.size(), st.data, st.outWords, 0,
                           [&](const uint8_t* jobs, const uint32_t* data, uint32_t* out, hipStream_t stream) {
                             mrp::AssignParams P;
                             P.maps = ctx->mapsDev;
                             P.jobs = reinterpret_cast<const mrp::as::AssignJob*>(jobs);
                             P.data = data;
                             P.out = out;
                             P.n = static_cast<uint32_t>(st.jobs.size());
                             return mrp_ll_launch_assign(&P, st.ldsBytes, stream);
                           });
  if (rc != MRP_LL_SUCCESS) return rc;
  mrp::host::unpackAssignBatch(st, ctx->assignOut.data(), results);
  return MRP_LL_SUCCESS;
}

// The same for the wide form (packAssignBatchWide, the wide kernel).
int assignLaunchWide(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_result* results) {
  mrp::host::AssignStagingWide& st = ctx->assignStagingWide;
  mrp::host::packAssignBatchWide(ctx->env, n, problems, results, ctx->assignLdsBudget, st);
  if (st.jobs.empty()) return MRP_LL_SUCCESS;
  const int rc = assignRun(ctx, st.jobs.data(), st.jobs.size() * sizeof(mrp::as::AssignJobWide), st.jobs.size(), st.data, st.outWords,
                           st.scratchWords, [&](const uint8_t* jobs, const uint32_t* data, uint32_t* out, hipStream_t stream) {
                             mrp::AssignWideParams P;
                             P.maps = ctx->mapsDev;
                             P.jobs = reinterpret_cast<const mrp::as::AssignJobWide*>(jobs);
                             P.data = data;
                             P.out = out;
                             P.n = static_cast<uint32_t>(st.jobs.size());
                             return mrp_ll_launch_assign_wide(&P, st.ldsBytes, stream);
                           });
  if (rc != MRP_LL_SUCCESS) return rc;
  mrp::host::unpackAssignBatchWide(st, ctx->assignOut.data(), results);
  return MRP_LL_SUCCESS;
}

}  // namespace

extern "C" {

int mrp_ll_assign_batch(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_result* results) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!problems || !results))) {
    ctx->err = "mrp_ll_assign_batch: invalid argument";
    return MRP_LL_E_INVALID;
  }
  for (int32_t k = 0; k < n; ++k)
    if (problems[k].n_agents > 0 && !results[k].task_of) {
      ctx->err = "mrp_ll_assign_batch: a result without a task_of buffer";
      return MRP_LL_E_INVALID;
    }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_assign_batch: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (n == 0) return MRP_LL_SUCCESS;
  return assignLaunch(ctx, n, problems, results);
}

int mrp_ll_assign_batch_w(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_result* results) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!problems || !results))) {
    ctx->err = "mrp_ll_assign_batch_w: invalid argument";
    return MRP_LL_E_INVALID;
  }
  for (int32_t k = 0; k < n; ++k)
    if (problems[k].n_agents > 0 && !results[k].task_of) {
      ctx->err = "mrp_ll_assign_batch_w: a result without a task_of buffer";
      return MRP_LL_E_INVALID;
    }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_assign_batch_w: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (n == 0) return MRP_LL_SUCCESS;
  return assignLaunchWide(ctx, n, problems, results);
}

int mrp_ll_assign_series_create(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem* problems, mrp_ll_assign_series** out) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!problems || !out))) {
    ctx->err = "mrp_ll_assign_series_create: invalid argument";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_assign_series_create: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (n == 0) return MRP_LL_SUCCESS;
  const int rc = mrp::host::assignSeriesCreate(
      ctx, n, problems, out,
      [ctx](int32_t m, const mrp_ll_assign_problem* ps, mrp_ll_assign_result* rs) { return assignLaunch(ctx, m, ps, rs); });
  if (rc == MRP_LL_E_INVALID)
    ctx->err = "mrp_ll_assign_series_create: a problem is constrained (mode, forbidden, min_matching) or not a valid problem";
  return rc;
}

int mrp_ll_assign_series_create_w(mrp_ll_ctx* ctx, int32_t n, const mrp_ll_assign_problem_w* problems, mrp_ll_assign_series** out) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!problems || !out))) {
    ctx->err = "mrp_ll_assign_series_create_w: invalid argument";
    return MRP_LL_E_INVALID;
  }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_assign_series_create_w: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (n == 0) return MRP_LL_SUCCESS;
  const int rc = mrp::host::assignSeriesCreateWide(
      ctx, n, problems, out,
      [ctx](int32_t m, const mrp_ll_assign_problem_w* ps, mrp_ll_assign_result* rs) { return assignLaunchWide(ctx, m, ps, rs); });
  if (rc == MRP_LL_E_INVALID)
    ctx->err = "mrp_ll_assign_series_create_w: a problem is constrained (mode, forbidden, min_matching), has too few mask_words or is not a valid problem";
  return rc;
}

int mrp_ll_assign_series_next(mrp_ll_ctx* ctx, int32_t n, mrp_ll_assign_series* const* series, mrp_ll_assign_result* results) {
  if (!ctx) return MRP_LL_E_INVALID;
  if (n < 0 || (n > 0 && (!series || !results))) {
    ctx->err = "mrp_ll_assign_series_next: invalid argument";
    return MRP_LL_E_INVALID;
  }
  for (int32_t k = 0; k < n; ++k)
    if (!series[k] || series[k]->owner != ctx) {
      ctx->err = "mrp_ll_assign_series_next: a series that is NULL or belongs to another context";
      return MRP_LL_E_INVALID;
    }
  if (engineBusy(ctx)) {
    ctx->err = "mrp_ll_assign_series_next: a session is active or a batch is in flight";
    return MRP_LL_E_BUSY;
  }
  if (n == 0) return MRP_LL_SUCCESS;
  const int rc = mrp::host::assignSeriesNext(
      n, series, results,
      [ctx](int32_t m, const mrp_ll_assign_problem* ps, mrp_ll_assign_result* rs) { return assignLaunch(ctx, m, ps, rs); },
      [ctx](int32_t m, const mrp_ll_assign_problem_w* ps, mrp_ll_assign_result* rs) { return assignLaunchWide(ctx, m, ps, rs); });
  if (rc == MRP_LL_E_INVALID) ctx->err = "mrp_ll_assign_series_next: a series given twice, or a result without a task_of buffer";
  return rc;
}

void mrp_ll_assign_series_destroy(mrp_ll_assign_series* series) { delete series; }

}  // extern "C"
