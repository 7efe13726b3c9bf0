// The submit and wait entry points: each validates its own arguments, then all go through submitJobs to the batch or the
// session packer.
#pragma once
#include "ll_batch.h"
#include "ll_session_jobs.h"

namespace {

// a.tag >= 0: a co-worker's call into a session (mrp_ll_submit_tagged / _scan / _sets / _node), serialised by coMu.
int submitJobs(mrp_ll_ctx* ctx, const SubmitArgs& a, int32_t* ticketOut) {
  if (a.tag < 0) return ctx->env.session.active ? sessionSubmit(ctx, a, ticketOut) : batchSubmit(ctx, a, ticketOut);
  std::lock_guard<std::mutex> lock(ctx->coMu);
  if (!ctx->env.session.active) return MRP_LL_E_INVALID;
  return sessionSubmit(ctx, a, ticketOut);
}

}  // namespace

extern "C" {

int mrp_ll_submit(mrp_ll_ctx* ctx, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results, int32_t* ticketOut) {
  if (!ctx || !ticketOut || nJobs < 0 || (nJobs > 0 && (!jobs || !results))) return MRP_LL_E_INVALID;
  return submitJobs(ctx, SubmitArgs{-1, nJobs, jobs, results, nullptr, nullptr}, ticketOut);
}

int mrp_ll_submit_lane(mrp_ll_ctx* ctx, int32_t lane, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       int32_t* ticketOut) {
  if (!ctx || !ticketOut || nJobs < 0 || (nJobs > 0 && (!jobs || !results)) || lane < 0 || lane > 1) return MRP_LL_E_INVALID;
  // one device queue, first in first out: `lane` is accepted for source compatibility and otherwise ignored — priority is
  // the order in which the caller publishes (see mrp_ll.h); batch mode has one queue anyway
  return submitJobs(ctx, SubmitArgs{-1, nJobs, jobs, results, nullptr, nullptr}, ticketOut);
}

int mrp_ll_submit_tagged(mrp_ll_ctx* ctx, int32_t tag, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                         int32_t* ticketOut) {
  if (!ctx || !ticketOut || tag < 0 || tag >= mrp_ll_ctx::kMaxTags || nJobs < 0 || (nJobs > 0 && (!jobs || !results)))
    return MRP_LL_E_INVALID;
  return submitJobs(ctx, SubmitArgs{tag, nJobs, jobs, results, nullptr, nullptr}, ticketOut);
}

int mrp_ll_submit_scan(mrp_ll_ctx* ctx, int32_t tag, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       mrp_ll_conflict* conflicts, int32_t* ticketOut) {
  if (!ctx || !ticketOut || nJobs < 0 || (nJobs > 0 && (!jobs || !results || !conflicts))) return MRP_LL_E_INVALID;
  if (!ctx->env.session.active) tag = -1;  // batch mode: the tag names nobody
  else if (tag < 0 || tag >= mrp_ll_ctx::kMaxTags) return MRP_LL_E_INVALID;
  return submitJobs(ctx, SubmitArgs{tag, nJobs, jobs, results, conflicts, nullptr}, ticketOut);
}

int mrp_ll_submit_sets(mrp_ll_ctx* ctx, int32_t tag, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       mrp_ll_conflict* conflicts, const mrp_ll_constraint_ref* sets, int32_t* ticketOut) {
  if (!ctx || !ticketOut || nJobs < 0 || (nJobs > 0 && (!jobs || !results))) return MRP_LL_E_INVALID;
  if (!ctx->env.session.active) tag = -1;  // batch mode: the tag names nobody
  else if (tag < 0 || tag >= mrp_ll_ctx::kMaxTags) return MRP_LL_E_INVALID;
  return submitJobs(ctx, SubmitArgs{tag, nJobs, jobs, results, conflicts, sets}, ticketOut);
}

int mrp_ll_submit_node(mrp_ll_ctx* ctx, int32_t tag, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results,
                       mrp_ll_conflict* conflicts, const mrp_ll_constraint_ref* sets, const mrp_ll_scan_base* bases,
                       int32_t* ticketOut) {
  if (!ctx || !ticketOut || nJobs < 0 || (nJobs > 0 && (!jobs || !results))) return MRP_LL_E_INVALID;
  if (!ctx->env.session.active) tag = -1;  // batch mode: the tag names nobody
  else if (tag < 0 || tag >= mrp_ll_ctx::kMaxTags) return MRP_LL_E_INVALID;
  return submitJobs(ctx, SubmitArgs{tag, nJobs, jobs, results, conflicts, sets, bases}, ticketOut);
}

int mrp_ll_poll(mrp_ll_ctx* ctx, int32_t ticket, int32_t* doneOut) {
  if (!ctx || !doneOut) return MRP_LL_E_INVALID;
  if (ctx->env.session.active) return sessionPoll(ctx, ticket, doneOut);
  // batch mode: completion of the launch
  if (ticket < 0 || ticket >= static_cast<int32_t>(ctx->tickets.size()) || !ctx->tickets[ticket].inFlight)
    return MRP_LL_E_INVALID;
  if (ctx->tickets[ticket].nJobs > 0 && hipEventQuery(ctx->tickets[ticket].evK1) == hipErrorNotReady) {
    *doneOut = 0;
    return MRP_LL_SUCCESS;
  }
  *doneOut = 1;
  return batchWait(ctx, ticket);
}

int mrp_ll_wait(mrp_ll_ctx* ctx, int32_t ticket) {
  if (!ctx) return MRP_LL_E_INVALID;
  return ctx->env.session.active ? sessionWait(ctx, ticket) : batchWait(ctx, ticket);
}

int mrp_ll_search_batch(mrp_ll_ctx* ctx, int32_t nJobs, const mrp_ll_job* jobs, mrp_ll_result* results) {
  int32_t ticket = -1;
  int rc = mrp_ll_submit(ctx, nJobs, jobs, results, &ticket);
  if (rc != MRP_LL_SUCCESS) return rc;
  return mrp_ll_wait(ctx, ticket);
}

}  // extern "C"
