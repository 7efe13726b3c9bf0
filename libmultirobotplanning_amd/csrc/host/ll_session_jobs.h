// Session mode, the jobs' side: publishing jobs into the ring, collecting their results by ticket or from the completion queue.
#pragma once
#include "ll_batch.h"
#include "ll_ctx.h"
#include "ll_session.h"

namespace {

int sessionSubmit(mrp_ll_ctx* ctx, const SubmitArgs& a, int32_t* ticketOut) {
  Ring& g = ctx->ring;
  const PackEnv::Session& S = ctx->env.session;
  const int32_t nJobs = a.nJobs;
  const mrp_ll_job* jobs = a.jobs;
  // One device queue, first in first out (mrp_ll_submit_lane).  The lane plumbing below — Q[1], head[1], the lane bit of
  // slotGen, headWord + 16 * lane — is kept on purpose: the kernels still take ring_size1 and a second head word
  // (LaunchParams), and device code is not this file's to change.
  const int lane = 0;
  sessionBeat(g);
  const uint32_t nSlotsLane = S.sipp ? Ring::kSippSlots : Ring::kSlots;
  const uint32_t Q = g.Q[lane];
  const uint32_t qBase = lane ? g.Q[0] : 0;
  if (nJobs > static_cast<int32_t>(nSlotsLane)) {
    ctx->err = "mrp_ll_submit (session): batch larger than the ring";
    return MRP_LL_E_INVALID;
  }
  if (g.freeSlots.size() < static_cast<size_t>(nJobs)) return MRP_LL_E_BUSY;  // (the caller consumes finished tickets first)
  for (int i = 0; i < nJobs; ++i) {
    // a ticket entry may be overwritten once the job published there a whole ring ago has been consumed
    const uint32_t qi = qBase + static_cast<uint32_t>((g.head[lane] + i) % Q);
    const uint32_t prev = g.tkSlot[qi];
    if (prev != 0xFFFFFFFFu && g.busy[prev] && g.slotGen[prev] == g.tkSeq[qi]) return MRP_LL_E_BUSY;
  }
  auto packT0 = std::chrono::steady_clock::now();
  int ti = -1;
  if (!ctx->sessFree.empty()) {
    ti = ctx->sessFree.back();
    ctx->sessFree.pop_back();
  } else {
    ctx->sess.emplace_back();
    ti = static_cast<int>(ctx->sess.size()) - 1;
  }
  SessTicket& st = ctx->sess[ti];
  st.used = true;
  st.lane = lane;
  st.tag = a.tag;
  st.n = nJobs;
  st.remaining = nJobs;
  st.res = a.results;
  st.conf = a.conflicts;
  st.state.assign(nJobs, 0);
  st.slots.resize(nJobs);
  st.seq.resize(nJobs);
  for (int i = 0; i < nJobs; ++i) {
    const mrp_ll_job& job = jobs[i];
    const uint64_t tk = g.head[lane] + i;
    const uint32_t qi = qBase + static_cast<uint32_t>(tk % Q);
    const uint32_t gen = (static_cast<uint32_t>(tk / Q) + 1) & 0x1FFFFFu;
    const uint32_t slot = g.freeSlots.back();
    g.freeSlots.pop_back();
    // a SIPP session takes SIPP jobs only (their tables have a buffer of their own), an A* / A*-epsilon session none
    ConsSinkSlot cs = S.sipp ? ConsSinkSlot{g.sippCons + static_cast<size_t>(slot) * g.sippSlotWords, slot * g.sippSlotWords, g.sippSlotWords}
                             : ConsSinkSlot{g.cons + static_cast<size_t>(slot) * Ring::kSlotConsWords, slot * Ring::kSlotConsWords,
                                            Ring::kSlotConsWords};
    PathSinkSlot ps{g.paths + static_cast<size_t>(slot) * Ring::kSlotPathHalfs, slot * Ring::kSlotPathHalfs,
                    Ring::kSlotPathHalfs};
    const bool rightKind = S.sipp ? job.algo == MRP_LL_SIPP
                                  : job.algo != MRP_LL_SIPP &&
                                        (S.kind == 0 || (S.kind == 1 ? job.algo == MRP_LL_ASTAR_EPS
                                                                     : (job.algo == MRP_LL_ASTAR || job.algo == MRP_LL_ASTAR_TA)));
    DevJob d;
    PendingSet pending;
    const bool ok = rightKind && packJob(ctx->env, job, a.packArgs(i), cs, ps, d, pending);
    // (not ok: wrong kind of job for this session, or constraint list / table larger than a ring slot)
    if (!ok) trivialRejectedJob(ctx->env, d);
    JobNote& note = g.notes[slot];
    note = JobNote();
    note.rejected = ok ? 0 : 1;
    if (S.sipp && ok) {
      note.dimx = ctx->env.maps[job.map_id].dimx;
      if (job.sipp_table) {
        note.sippFlags = static_cast<uint8_t>(((d.ctx_flags & mrp::kSippResident) ? 1u : 0u) | (job.sipp_commit ? 2u : 0u));
        if (note.sippFlags) note.table = const_cast<mrp_ll_sipp_table*>(job.sipp_table);
      }
    }
    commitSet(ctx->env, ok && !S.sipp, pending, note.setSlot, note.setSeq);
    note.scan = (!S.sipp && (job.flags & MRP_LL_JOB_SCAN_CONFLICTS) && st.conf) ? 1 : 0;
    note.init = jobInitOf(job, ok);
    note.chain = S.sipp ? 0 : chainResultsOf(job);
    g.jobs[slot] = d;
    ctx->stats.staged_bytes += static_cast<int64_t>(sizeof(DevJob)) + 4 * static_cast<int64_t>(cs.used) +
                               (S.sipp || (d.ctx_flags & mrp::kCtxById) ? 0 : 2 * static_cast<int64_t>(d.t_pad) * d.n_agents_pad);
    g.busy[slot] = 1;
    g.slotTicket[slot] = ti;
    g.slotJob[slot] = i;
    g.slotGen[slot] = ((static_cast<uint32_t>(tk) + 1u) & 0x3FFFFFFFu) | 0x40000000u | (lane ? 0x80000000u : 0u);  // never 0
    __atomic_store_n(g.done + slot, 0u, __ATOMIC_RELAXED);  // the previous occupant's done word must not be mistaken
    g.tkSlot[qi] = slot;
    g.tkSeq[qi] = g.slotGen[slot];
    st.slots[i] = slot;
    st.seq[i] = g.slotGen[slot];
    pushFence(g);  // the job data above leaves before its ticket entry
    __atomic_store_n(g.state + qi, (gen << mrp::kRingSlotBits) | slot, __ATOMIC_RELEASE);  // publish: the job data above is visible first
  }
  pushFence(g);    // ... and the entries before the count that covers them
  g.head[lane] += static_cast<uint64_t>(nJobs);
  g.inFlightJobs += static_cast<uint32_t>(nJobs);
  // after every ticket entry
  __atomic_store_n(g.headWord + 16 * lane, static_cast<uint32_t>(g.head[lane]), __ATOMIC_RELEASE);
  pushFence(g);
  ctx->stats.pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - packT0).count();
  *ticketOut = ti;
  return MRP_LL_SUCCESS;
}

// The slot's occupant has been consumed: the slot is free again, and the resident kernel has shown that it is alive.
inline void releaseSlot(Ring& g, uint32_t slot) {
  g.busy[slot] = 0;
  g.inFlightJobs -= 1;
  g.emptyPolls = 0;
  g.freeSlots.push_back(slot);
}

// The finished job in `slot` -> its caller's result; the slot goes back to the free list.  Returns the job's ticket.
SessTicket& collectSlot(mrp_ll_ctx* ctx, uint32_t slot) {
  Ring& g = ctx->ring;
  const uint32_t outStride = ctx->env.session.outStride;
  SessTicket& st = ctx->sess[g.slotTicket[slot]];
  const int32_t i = g.slotJob[slot];
  collectJob(ctx, g.notes[slot], g.results[slot], g.outPaths + static_cast<size_t>(slot) * outStride, outStride, st.res[i],
             st.conf ? st.conf + i : nullptr);
  st.state[i] = 1;
  st.remaining -= 1;
  releaseSlot(g, slot);
  return st;
}

int sessionPoll(mrp_ll_ctx* ctx, int32_t ticket, int32_t* doneOut) {
  Ring& g = ctx->ring;
  if (ticket < 0 || ticket >= static_cast<int32_t>(ctx->sess.size()) || !ctx->sess[ticket].used) return MRP_LL_E_INVALID;
  SessTicket& st = ctx->sess[ticket];
  sessionBeat(g);
  for (int i = 0; i < st.n && st.remaining > 0; ++i) {
    if (st.state[i] == 1) continue;
    const uint32_t slot = st.slots[i];
    if (__atomic_load_n(g.done + slot, __ATOMIC_ACQUIRE) != st.seq[i]) continue;
    collectSlot(ctx, slot);
  }
  *doneOut = st.remaining == 0 ? 1 : 0;
  if (st.remaining == 0) {
    st.used = false;
    ctx->sessFree.push_back(ticket);
  }
  return MRP_LL_SUCCESS;
}

// Drains the completion queue: every finished job is unpacked into its caller's result; a ticket whose last job this was
// goes to `tickets` (tag < 0: all of them; else: those of this co-worker, the others wait in their owner's stash).
int32_t drainCompletions(mrp_ll_ctx* ctx, int32_t tag, int32_t* tickets, int32_t cap) {
  Ring& g = ctx->ring;
  const uint32_t R = Ring::kSlots;
  int32_t n = 0;
  // entry k holds (k / R + 1) << 11 | slot once the k-th finished job has been published
  while (n < cap) {
    const uint64_t cursor = g.compCursor;
    const uint32_t e = __atomic_load_n(g.compRing + (cursor % R), __ATOMIC_ACQUIRE);
    if ((e >> mrp::kRingSlotBits) != static_cast<uint32_t>(cursor / R) + 1) break;
    __atomic_store_n(&g.compCursor, cursor + 1, __ATOMIC_RELAXED);
    const uint32_t slot = e & mrp::kRingSlotMask;
    if (!g.busy[slot]) continue;  // already consumed through mrp_ll_poll / mrp_ll_wait
    // ... and if the slot has been re-used since, this entry is stale: only the occupant's own done word counts
    if (__atomic_load_n(g.done + slot, __ATOMIC_ACQUIRE) != g.slotGen[slot]) continue;
    const int32_t id = g.slotTicket[slot];
    SessTicket& st = collectSlot(ctx, slot);
    if (st.remaining == 0) {
      if (tag >= 0 && st.tag != tag && st.tag >= 0 && st.tag < mrp_ll_ctx::kMaxTags) {
        ctx->coStash[st.tag].push_back(id);  // its owner collects (and releases) it
        ctx->coStashCount[st.tag].fetch_add(1, std::memory_order_release);
      } else {
        st.used = false;
        ctx->sessFree.push_back(id);
        tickets[n++] = id;
      }
    }
  }
  return n;
}

int sessionWait(mrp_ll_ctx* ctx, int32_t ticket) {
  auto t0 = std::chrono::steady_clock::now();
  for (uint64_t spin = 0;; ++spin) {
    int32_t done = 0;
    int rc = sessionPoll(ctx, ticket, &done);
    if (rc != MRP_LL_SUCCESS) return rc;
    if (done) return MRP_LL_SUCCESS;
    if ((spin & 0xFFF) == 0xFFF) {
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0) {
        ctx->err = "mrp_ll_wait (session): no completion within 120 s";
        return MRP_LL_E_DEVICE;
      }
      if (hipEventQuery(ctx->ring.ev1) != hipErrorNotReady) {
        ctx->err = "mrp_ll_wait (session): the resident kernel has exited (idle limit or fault)";
        return MRP_LL_E_DEVICE;
      }
    }
  }
}

}  // namespace

extern "C" {

int mrp_ll_poll_any(mrp_ll_ctx* ctx, int32_t* tickets, int32_t cap, int32_t* nOut) {
  if (!ctx || !tickets || !nOut || cap <= 0) return MRP_LL_E_INVALID;
  Ring& g = ctx->ring;
  if (!ctx->env.session.active) return MRP_LL_E_INVALID;
  sessionBeat(g);
  const int32_t n = drainCompletions(ctx, -1, tickets, cap);
  *nOut = n;
  if (n != 0) {
    g.emptyPolls = 0;  // (also when only stashed tickets were handed back)
    return MRP_LL_SUCCESS;
  }
  return sessionAlive(ctx);
}

int mrp_ll_poll_any_tagged(mrp_ll_ctx* ctx, int32_t tag, int32_t* tickets, int32_t cap, int32_t* nOut) {
  if (!ctx || !tickets || !nOut || cap <= 0 || tag < 0 || tag >= mrp_ll_ctx::kMaxTags) return MRP_LL_E_INVALID;
  Ring& g = ctx->ring;
  *nOut = 0;
  // a look without the lock: nothing stashed for this co-worker, nothing new in the completion queue
  if (ctx->coStashCount[tag].load(std::memory_order_acquire) == 0) {
    const uint64_t cursor = __atomic_load_n(&g.compCursor, __ATOMIC_RELAXED);
    const uint32_t e = __atomic_load_n(g.compRing + (cursor % Ring::kSlots), __ATOMIC_ACQUIRE);
    const uint64_t tsc = __builtin_ia32_rdtsc();
    const bool beatDue = tsc - __atomic_load_n(&g.lastBeatTsc, __ATOMIC_RELAXED) >= (1ull << 24);
    if ((e >> mrp::kRingSlotBits) != static_cast<uint32_t>(cursor / Ring::kSlots) + 1 && !beatDue) return MRP_LL_SUCCESS;
  }
  std::lock_guard<std::mutex> lock(ctx->coMu);
  if (!ctx->env.session.active) return MRP_LL_E_INVALID;
  sessionBeat(g);
  int32_t n = 0;
  std::vector<int32_t>& mine = ctx->coStash[tag];
  while (n < cap && !mine.empty()) {
    const int32_t id = mine.back();
    mine.pop_back();
    ctx->coStashCount[tag].fetch_sub(1, std::memory_order_relaxed);
    ctx->sess[id].used = false;
    ctx->sessFree.push_back(id);
    tickets[n++] = id;
  }
  n += drainCompletions(ctx, tag, tickets + n, cap - n);
  *nOut = n;
  if (n != 0) {
    g.emptyPolls = 0;  // (also when only stashed tickets were handed back)
    return MRP_LL_SUCCESS;
  }
  return sessionAlive(ctx);
}

}  // extern "C"
