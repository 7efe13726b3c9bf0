// Batch mode: one launch per submit, jobs staged in growable pinned buffers of a ticket.
#pragma once
#include "ll_ctx.h"
#include "ll_maps.h"

namespace {

// What one submit call hands over, whichever entry point it came through (ll_submit.h).
struct SubmitArgs {
  int32_t tag;                        // the co-worker the ticket belongs to (-1: none, and no lock is taken)
  int32_t nJobs;
  const mrp_ll_job* jobs;
  mrp_ll_result* results;
  mrp_ll_conflict* conflicts;         // mrp_ll_submit_scan / _sets: one entry per job (what admits flagged jobs), else null
  const mrp_ll_constraint_ref* sets;  // mrp_ll_submit_sets: one entry per job (what admits by-set jobs), else null
  const mrp_ll_scan_base* bases;      // mrp_ll_submit_node: one entry per job (what admits MRP_LL_JOB_SCAN_FROM_PARENT jobs), else null
  PackArgs packArgs(int i) const { return PackArgs{conflicts != nullptr, sets ? sets + i : nullptr, bases ? bases + i : nullptr}; }
};

// Where a packed job's constraint words / path table go in a batch: growable buffers (sessions: the slot sinks of ll_pack.h).
struct ConsSinkBuf {
  PinnedBuf<uint32_t>& b;
  bool failed = false;
  size_t size() const { return b.size; }
  bool fits(size_t) const { return true; }
  void push(uint32_t w) {
    if (b.push(w) != hipSuccess) failed = true;
  }
  uint32_t* grow(size_t n) {  // n consecutive words, written by the caller
    const size_t at = b.size;
    if (b.resize(at + n) != hipSuccess) {
      failed = true;
      return nullptr;
    }
    return b.host + at;
  }
};
struct PathSinkBuf {
  PinnedBuf<uint16_t>& b;
  bool failed = false;
  uint16_t* alloc(size_t n, uint32_t& off) {
    size_t base = (b.size + 7u) & ~size_t(7);  // 16-byte aligned table start
    if (b.resize(base + n) != hipSuccess) {
      failed = true;
      return nullptr;
    }
    off = static_cast<uint32_t>(base);
    return b.host + base;
  }
};

// Fills the launch parameters that do not depend on where the jobs live; returns the dynamic LDS size.
// kind: the kernel family the launch uses (0 mixed, 1 A*-epsilon only, 2 A* only): the A*-epsilon-only kernels keep the
// (time, cell) bitmap of the compact tier in the arena slot and take a smaller LDS window.
int fillCommonParams(mrp_ll_ctx* ctx, Ticket& t, mrp::LaunchParams& P, uint32_t& ldsBytesOut, int kind) {
  const PackEnv& env = ctx->env;
  P.maps = ctx->mapsDev;
  P.queue_head = t.queueHead;
  P.arena = t.arena;
  P.arena_stride = ctx->arenaStride;
  P.arena_scratch_off = ctx->arenaScratchOff;
  P.arena_paths_bytes = env.arenaPathsBytes;
  P.out_stride = static_cast<uint32_t>(env.maxHorizon);
  P.out_host_stride = P.out_stride + mrp::kScanOutHalfs;  // the path, then a flagged job's conflicts (sessions: the ring's stride, sessionBegin)
  P.arena_nodes = static_cast<uint32_t>(env.arenaNodes);
  P.arena_rows = static_cast<uint32_t>(env.maxHorizon);
  P.arena_row_words = ctx->arenaRowWords;
  // LDS of a workgroup: the compact tier's window (fixed size, ll_compact.h) + the focal path table; occupancy is
  // floor(160 KiB / ldsBytes) workgroups per CU
  uint32_t ldsNodes = static_cast<uint32_t>(env.ldsNodes);
  uint32_t rowWords = (ctx->maxWpr + 3u) & ~3u;
  uint32_t rows = 0;
  uint32_t ldsBytes = 0;
  uint32_t ldsPaths = ctx->tierPathBytes;
  if (const char* e = std::getenv("MRP_LL_LDS_PATHS")) ldsPaths = static_cast<uint32_t>(std::max(0, std::atoi(e))) & ~31u;  // tuning knob
  if (ldsNodes) {
    rows = 64;
    ldsBytes = mrp_ll_lds_bytes(kind, ldsNodes, rows, rowWords, ldsPaths);
    if (ldsBytes > 160u * 1024u - 512u) {
      ldsNodes = 0;
      rows = 0;
    }
  }
  if (!ldsNodes) ldsBytes = mrp_ll_lds_bytes(kind, 0, 0, 0, 0);  // the control block alone
  P.path_store = ctx->pathStore;
  P.path_store_stride = ctx->pathStoreStride;
  P.path_store_slots = env.pathStoreSlots;
  P.cons_store = ctx->consStore;
  P.cons_store_stride = env.consStoreStride;
  P.cons_store_slots = env.consStoreSlots;
  P.lds_nodes = ldsNodes;
  // the window is sized for 64 time steps whatever the caller asked for; what mrp_ll_configure_tiers' lds_rows sets is how many
  // of them a search may use before it leaves the tier (ll_jobs.h narrowMaxT, the only reader)
  P.lds_rows = std::min(rows, ctx->tierRows);
  P.lds_row_words = rowWords;
  P.lds_paths_bytes = ldsNodes ? ldsPaths : 0;
  if (kDebug) {
    if (!ctx->debugHost) {
      HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->debugHost), 16 * 4 * 4096,
                                hipHostMallocMapped | hipHostMallocCoherent));
    }
    std::memset(ctx->debugHost, 0, 16 * 4 * 4096);
    void* dptr = nullptr;
    HIPCHK(ctx, hipHostGetDevicePointer(&dptr, ctx->debugHost, 0));
    P.debug = static_cast<volatile uint32_t*>(dptr);
  }
  ldsBytesOut = ldsBytes;
  return MRP_LL_SUCCESS;
}

int batchSubmit(mrp_ll_ctx* ctx, const SubmitArgs& a, int32_t* ticketOut) {
  const int32_t nJobs = a.nJobs;
  const mrp_ll_job* jobs = a.jobs;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int ti = -1;
  for (size_t i = 0; i < ctx->tickets.size(); ++i)
    if (!ctx->tickets[i].inFlight) {
      ti = static_cast<int>(i);
      break;
    }
  if (ti < 0) {
    ctx->err = "mrp_ll_submit: all tickets in flight";
    return MRP_LL_E_BUSY;
  }
  int rc = syncMaps(ctx);
  if (rc != MRP_LL_SUCCESS) return rc;
  Ticket& t = ctx->tickets[ti];
  auto packT0 = std::chrono::steady_clock::now();
  t.nJobs = nJobs;
  t.userResults = a.results;
  t.userConflicts = a.conflicts;
  t.notes.assign(nJobs, JobNote());
  {
    int nSipp = 0;
    for (int i = 0; i < nJobs; ++i) nSipp += jobs[i].algo == MRP_LL_SIPP ? 1 : 0;
    if (nSipp != 0 && nSipp != nJobs) {
      ctx->err = "mrp_ll_submit: a batch holds either MRP_LL_SIPP jobs or A-star jobs, not both";
      return MRP_LL_E_INVALID;
    }
    t.sipp = nSipp != 0;
    int nEps = 0, nEpsTa = 0;
    for (int i = 0; i < nJobs; ++i) nEps += jobs[i].algo == MRP_LL_ASTAR_EPS ? 1 : 0;
    for (int i = 0; i < nJobs; ++i)  // (a table-h job counts as a job of another algorithm)
      nEpsTa += (jobs[i].algo == MRP_LL_ASTAR_EPS_TA ||
                 ((jobs[i].flags & MRP_LL_JOB_TABLE_H) && (jobs[i].algo == MRP_LL_ASTAR || jobs[i].algo == MRP_LL_ASTAR_EPS))) ? 1 : 0;
    // a one-algorithm batch runs the specialised kernel; MRP_LL_ASTAR_EPS_TA and MRP_LL_JOB_TABLE_H live in the mixed kernel only
    t.kind = (t.sipp || nEpsTa != 0) ? 0 : nEps == nJobs ? 1 : nEps == 0 ? 2 : 0;
  }
  t.jobs.clear();
  t.cons.clear();
  t.paths.clear();
  HIPCHK(ctx, t.jobs.resize(std::max(nJobs, 1)));
  bool allocFailed = false;
  for (int i = 0; i < nJobs; ++i) {
    size_t c0 = t.cons.size, p0 = t.paths.size;
    ConsSinkBuf cs{t.cons};
    PathSinkBuf ps{t.paths};
    JobNote& note = t.notes[i];
    PendingSet pending;
    const bool ok = packJob(ctx->env, jobs[i], a.packArgs(i), cs, ps, t.jobs.host[i], pending);
    commitSet(ctx->env, ok && !cs.failed && !ps.failed, pending, note.setSlot, note.setSeq);
    note.scan = (!t.sipp && (jobs[i].flags & MRP_LL_JOB_SCAN_CONFLICTS) && t.userConflicts) ? 1 : 0;
    if (t.sipp) {
      note.dimx = ok ? static_cast<int32_t>(t.jobs.host[i].dimx) : 1;
      if (ok && jobs[i].sipp_table && jobs[i].sipp_commit) {  // batch mode never uses the device-resident copies: the host
        note.table = const_cast<mrp_ll_sipp_table*>(jobs[i].sipp_table);  // adds the stays
        note.sippFlags = 2u;
      }
    }
    note.init = jobInitOf(jobs[i], ok);
    // (a root chain needs a session: the packer has refused it, and its results come back as a refused chain's do)
    note.chain = t.sipp ? 0 : chainResultsOf(jobs[i]);
    if (cs.failed || ps.failed) allocFailed = true;
    if (!ok) {
      // rejected: give the device a trivially capped job and remember the rejection
      t.cons.size = c0;
      t.paths.size = p0;
      note.rejected = 1;
      trivialRejectedJob(ctx->env, t.jobs.host[i]);
    }
  }
  if (allocFailed) {
    for (const JobNote& n : t.notes)  // nothing of this call runs: the sets it would have written do not exist
      if (n.setSlot >= 0 && ctx->env.consSets[n.setSlot].seq == n.setSeq) ctx->env.consSets[n.setSlot] = ConsSetRec();
    ctx->err = "mrp_ll_submit: pinned staging allocation failed";
    return MRP_LL_E_NOMEM;
  }
  *ticketOut = ti;
  t.inFlight = true;
  if (nJobs == 0) return MRP_LL_SUCCESS;
  const uint32_t outStride = static_cast<uint32_t>(ctx->env.maxHorizon) + mrp::kScanOutHalfs;
  HIPCHK(ctx, t.cons.reserve(16));
  HIPCHK(ctx, t.paths.reserve(16));
  HIPCHK(ctx, t.results.resize(nJobs));
  HIPCHK(ctx, t.outPaths.resize(static_cast<size_t>(nJobs) * outStride));
  ctx->stats.pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - packT0).count();

  mrp::LaunchParams P;
  std::memset(&P, 0, sizeof(P));
  P.jobs = t.jobs.dev;
  P.results = t.results.dev;
  P.out_paths = t.outPaths.dev;
  P.cons = t.cons.dev;
  P.paths = t.paths.dev;
  P.queue_base = t.queueBase;
  P.n_jobs = static_cast<uint32_t>(nJobs);
  uint32_t ldsBytes = 0;
  {
    int rcp = fillCommonParams(ctx, t, P, ldsBytes, t.kind);
    if (rcp != MRP_LL_SUCCESS) return rcp;
  }
  uint32_t grid = std::min<uint32_t>(static_cast<uint32_t>(nJobs), static_cast<uint32_t>(ctx->opt.slots));
  t.queueBase += static_cast<uint32_t>(nJobs) + grid;  // every workgroup takes one ticket past the end when it exits
  HIPCHK(ctx, hipEventRecord(t.evK0, t.stream));
  if (t.sipp)
    HIPCHK(ctx, mrp_ll_launch_sipp(&P, grid, t.stream));
  else
    HIPCHK(ctx, mrp_ll_launch(&P, grid, ldsBytes, t.kind, t.stream));
  HIPCHK(ctx, hipEventRecord(t.evK1, t.stream));
  ctx->stats.launches += 1;
  return MRP_LL_SUCCESS;
}

int batchWait(mrp_ll_ctx* ctx, int32_t ticket) {
  if (ticket < 0 || ticket >= static_cast<int32_t>(ctx->tickets.size())) return MRP_LL_E_INVALID;
  Ticket& t = ctx->tickets[ticket];
  if (!t.inFlight) return MRP_LL_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (kDebug && ctx->debugHost) {
    for (int spin = 0; spin < 100 && hipEventQuery(t.evK1) == hipErrorNotReady; ++spin) {
      struct timespec ts = {0, 100000000};
      nanosleep(&ts, nullptr);
    }
    if (hipEventQuery(t.evK1) == hipErrorNotReady) {
      std::fprintf(stderr, "[mrp_ll] kernel did not finish within 10 s; trace of the first workgroups:\n");
      for (int b = 0; b < 4; ++b) {
        std::fprintf(stderr, "  wg %d:", b);
        for (int k = 0; k < 16; ++k) std::fprintf(stderr, " %u", ctx->debugHost[b * 16 + k]);
        std::fprintf(stderr, "\n");
      }
      std::fflush(stderr);
      std::_Exit(3);
    }
  }
  t.inFlight = false;
  if (t.nJobs == 0) return MRP_LL_SUCCESS;
  HIPCHK(ctx, hipEventSynchronize(t.evK1));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, t.evK0, t.evK1) == hipSuccess) ctx->stats.kernel_ms += ms;
  const uint32_t outStride = static_cast<uint32_t>(ctx->env.maxHorizon) + mrp::kScanOutHalfs;
  auto unpackT0 = std::chrono::steady_clock::now();
  for (int i = 0; i < t.nJobs; ++i)
    collectJob(ctx, t.notes[i], t.results.host[i], t.outPaths.host + static_cast<size_t>(i) * outStride, outStride, t.userResults[i],
               t.userConflicts ? t.userConflicts + i : nullptr);
  ctx->stats.unpack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - unpackT0).count();
  return MRP_LL_SUCCESS;
}

}  // namespace
