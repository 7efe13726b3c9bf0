// The engine's context: what a mrp_ll_ctx holds, the per-job record both modes keep until a result is collected, and the
// one routine that collects it.  Included by mrp_ll_host.cpp (the one host translation unit) in front of the subject headers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/mrp_ll.h"
#include "../heur_layout.h"
#include "../ll_device.h"
#include "../ll_launch.h"
#include "assign_pack.h"
#include "ll_pack.h"

namespace {

using namespace mrp::host;
using mrp::DevJob;
using mrp::DevResult;

// Growable pinned host buffer that the device accesses in place (zero-copy staging, see ll_device.h).
template <typename T>
struct PinnedBuf {
  T* host = nullptr;
  T* dev = nullptr;   // device-side address of the same memory
  size_t cap = 0, size = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    size_t ncap = std::max<size_t>(n, cap * 2);
    ncap = std::max<size_t>(ncap, 4096);
    T* nh = nullptr;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&nh), ncap * sizeof(T), hipHostMallocMapped);
    if (e != hipSuccess) return e;
    void* nd = nullptr;
    e = hipHostGetDevicePointer(&nd, nh, 0);
    if (e != hipSuccess) return e;
    if (host) {
      if (size) std::memcpy(nh, host, size * sizeof(T));
      (void)hipHostFree(host);
    }
    host = nh;
    dev = static_cast<T*>(nd);
    cap = ncap;
    return hipSuccess;
  }
  hipError_t resize(size_t n) {
    hipError_t e = reserve(n);
    if (e == hipSuccess) size = n;
    return e;
  }
  hipError_t push(const T& v) {
    if (size == cap) {
      hipError_t e = reserve(size + 1);
      if (e != hipSuccess) return e;
    }
    host[size++] = v;
    return hipSuccess;
  }
  void clear() { size = 0; }
  void release() {
    if (host) (void)hipHostFree(host);
    host = dev = nullptr;
    cap = size = 0;
  }
};

// What the host remembers about a published job until its result has been collected (collectJob): one per job of a
// batch ticket, one per job slot of a session.
struct JobNote {
  uint8_t rejected = 0;    // rejected on the host (MRP_LL_BAD_JOB)
  uint8_t scan = 0;        // flagged MRP_LL_JOB_SCAN_CONFLICTS: its entry of the caller's conflicts array is filled in
  uint8_t sippFlags = 0;   // of `table`: bit 0 = the job runs on the device-resident copy, bit 1 = sipp_commit
  int32_t init = 0;        // jobInitOf: initial_cost (A*) / start_time (SIPP) / the goal of a task-assignment job
  int32_t dimx = 0;        // SIPP: grid width (cell -> x, y when unpacking); 0 for every other job
  int32_t chain = 0;       // MRP_LL_JOB_ROOT_CHAIN: results the job fills (n_agents - agent_idx), else 0
  int32_t setSlot = -1;    // the constraint-store slot the job writes (-1: none) and the mirror's sequence number of that
  uint32_t setSeq = 0;     // write (setCollected)
  mrp_ll_sipp_table* table = nullptr;  // SIPP: the table the job has to report back to (else null)
};

struct Ticket {
  hipStream_t stream = nullptr;
  hipEvent_t evK0 = nullptr, evK1 = nullptr;
  PinnedBuf<DevJob> jobs;
  PinnedBuf<uint32_t> cons;
  PinnedBuf<uint16_t> paths;
  PinnedBuf<DevResult> results;
  PinnedBuf<uint16_t> outPaths;
  uint32_t* queueHead = nullptr;   // device, monotonic
  uint32_t queueBase = 0;
  uint8_t* arena = nullptr;
  bool inFlight = false;
  int32_t nJobs = 0;
  mrp_ll_result* userResults = nullptr;
  mrp_ll_conflict* userConflicts = nullptr;  // mrp_ll_submit_scan: the caller's array, one entry per job (else null)
  std::vector<JobNote> notes;     // per job, sized once per submit
  bool sipp = false;              // the batch holds MRP_LL_SIPP jobs (own kernel, own result format)
  int kind = 0;                   // A* batches: 0 = mixed, 1 = all A*-epsilon, 2 = all A*
};

// ---- session mode: job ring in coherent pinned host memory --------------------------------------------------
// Two levels: a TICKET ring per lane, consumed strictly in order by the workgroups (entry = generation << 11 | job
// slot), and a pool of job SLOTS (descriptor, constraint words, path table, result, path) handed out from a free
// list.  A slot is tied up until its result has been consumed, a ticket entry only until a workgroup has started the
// job, so one long search never blocks the publication of the searches behind it.
// (Whether a session is active, its kind and its output stride are in PackEnv::session: the packer reads them.)
struct Ring {
  static constexpr uint32_t kSlots = mrp::kRingSlots;     // job slots, shared by both lanes (the device masks with the same constant)
  static constexpr uint32_t kTickets0 = 1u << 17;         // ticket-ring entries of lane 0 / lane 1
  static constexpr uint32_t kTickets1 = 1u << 14;
  static constexpr uint32_t kTickets = kTickets0 + kTickets1;
  static constexpr uint32_t kSlotConsWords = mrp::host::kSlotConsWords;
  static constexpr uint32_t kSlotPathHalfs = mrp::host::kSlotPathHalfs;
  uint8_t* block = nullptr;        // pinned host memory: what the DEVICE writes and the host reads (done words, completion
                                   // queue, results, output paths) — and, without a large BAR, everything else too
  uint8_t* push = nullptr;         // what the HOST writes and the device reads (ticket entries, head / stop / heartbeat words,
                                   // job descriptors, constraint words, path tables): pinned host memory, or — with a large
                                   // BAR and MRP_LL_RING_IN_DEVICE=1 — UNCACHED DEVICE memory the host stores into directly
                                   // (write-combined, posted PCIe writes), so that the resident workgroups never read host
                                   // memory.  Measured the same within 1 % once the per-job cache fences were gone.
  bool pushInDevice = false;
  size_t pushBytes = 0;
  uint64_t lastBeatTsc = 0;
  uint32_t *state = nullptr, *done = nullptr, *stop = nullptr, *headWord = nullptr, *compRing = nullptr;
  uint32_t* compCountDev = nullptr;  // device counter
  unsigned long long* ticksDev = nullptr;  // device [2]: busy / idle ticks of the session's workgroups
  uint64_t compCursor = 0;           // next completion-queue entry the host expects
  uint32_t heartbeat = 0;            // bumped on every submit / poll: resident workgroups leave only when it stands still
  uint32_t emptyPolls = 0;           // consecutive polls that found nothing (liveness check of the resident kernel)
  uint32_t inFlightJobs = 0;         // published, result not consumed yet
  uint32_t idleLimitS = 20;
  DevJob* jobs = nullptr;
  DevResult* results = nullptr;
  uint16_t* outPaths = nullptr;
  uint32_t* cons = nullptr;
  uint16_t* paths = nullptr;
  uint64_t head[2] = {0, 0};       // per lane: next ticket number to publish
  std::vector<uint8_t> busy;       // slot holds a job whose result the host has not consumed yet
  std::vector<int32_t> slotTicket; // slot -> session ticket id / job index inside it
  std::vector<int32_t> slotJob;
  std::vector<uint32_t> slotGen;   // value the occupant's done word will show: its ticket number + 1 (valid while busy)
  std::vector<JobNote> notes;      // slot -> what collectJob needs of its occupant
  std::vector<uint32_t> freeSlots;     // job slots not in use (stack)
  std::vector<uint32_t> tkSlot, tkSeq; // per ticket-ring entry: the slot / done value of the job last published there
  uint32_t Q[2] = {kTickets0, kTickets1};  // ticket-ring entries in use (MRP_LL_TICKET_RING shrinks them: wrap tests)
  uint32_t grid = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // Optional second resident launch of the same session (MRP_LL_EXTRA_HBM_WGS): workgroups WITHOUT an LDS tier (their
  // searches live in the HBM arena / L2 from the start) on a stream of their own.  They take tickets from the same
  // rings; the LDS tier caps the first launch at floor(160 KiB / tier bytes) workgroups per CU, these fill SIMD issue
  // slots beyond that.
  uint32_t grid2 = 0;
  hipStream_t stream2 = nullptr;
  hipEvent_t ev2 = nullptr;
  // The heavy workgroups of an A*-epsilon session (mrp_ll_session_begin_tiers; ll_device.h heavy_q): the second launch is
  // then the heavy kernel, the first one the front kernel.
  bool heavy = false;
  unsigned long long* heavyQ = nullptr;   // device: kRingSlots entries
  uint32_t* heavyCtr = nullptr;           // device: [0] written, [16] taken
  uint32_t* heavyAlive = nullptr;         // pinned host: one word per heavy workgroup
  // SIPP sessions (mrp_ll_session_begin_sipp): the jobs' safe-interval tables are far larger than a slot's constraint
  // area, so they get their own pinned buffer, and only the first kSippSlots job slots are used
  static constexpr uint32_t kSippSlots = 512;
  uint32_t* sippCons = nullptr;
  uint32_t sippSlotWords = 0;      // capacity per slot the buffer was allocated with
};
// The host's stores into the push block are write-combined when it is device memory: everything written so far leaves
// the core's buffers, in order, before whatever is stored next (x86 SFENCE; a no-op price for pinned host memory).
inline void pushFence(const Ring& g) {
  if (g.pushInDevice) __builtin_ia32_sfence();
}
struct SessTicket {
  bool used = false;
  int32_t lane = 0;
  int32_t tag = -1;                // mrp_ll_submit_tagged: which of the context's co-workers the ticket belongs to (-1: untagged)
  int32_t n = 0, remaining = 0;
  mrp_ll_result* res = nullptr;
  mrp_ll_conflict* conf = nullptr; // mrp_ll_submit_scan: the caller's array, one entry per job (else null)
  std::vector<uint8_t> state;      // per job: 0 pending, 1 consumed
  std::vector<uint32_t> slots;     // per job: its job slot
  std::vector<uint32_t> seq;       // per job: the done value that marks it finished
};

}  // namespace

struct mrp_ll_ctx {
  mrp_ll_options opt;             // device, n_tickets, slots, max_cells (max_horizon / lds_nodes / arena_nodes: see env)
  int device = 0;
  std::string err;
  PackEnv env;                    // what the packer reads (host/ll_pack.h): maps and tables, limits, session, stores
  // The maps buffer (obstacle bitmaps and the heuristic tables of the task-assignment searches) is laid out in words
  // 0 .. mapsBase + mapWords.size(): the first mapsBase words are on the device ONLY (uploads already copied, tables the
  // device computed itself: mrp_ll_compute_heuristics), mapWords holds what has been uploaded since and not copied yet.
  std::vector<uint32_t> mapWords;
  size_t mapsBase = 0;
  uint32_t* mapsDev = nullptr;
  size_t mapsDevCap = 0;
  hipEvent_t heurEv0 = nullptr, heurEv1 = nullptr;  // kernel time of mrp_ll_compute_heuristics / mrp_ll_heuristic_lookup
  uint32_t maxWpr = 1;
  uint32_t extraHbmWgs = 0;       // session mode: additional resident workgroups without an LDS tier (see Ring::grid2)
  uint32_t tierRows = 64, tierPathBytes = 4096;  // LDS tier geometry (mrp_ll_configure_tiers); nodes live in env.ldsNodes
  bool frontTablesInMemory = false;  // mrp_ll_session_front_tables: front workgroups keep every focal table in their arena slot
  uint32_t sessionRowWords = 0;   // LDS bitmap row width the resident kernel was launched with
  uint32_t arenaRowWords = 0;
  uint64_t arenaStride = 0;
  uint32_t arenaScratchOff = 0;
  std::vector<Ticket> tickets;
  mrp_ll_stats stats;
  uint32_t* debugHost = nullptr;  // MRP_LL_DEBUG: host-mapped trace buffer
  Ring ring;
  std::vector<SessTicket> sess;
  std::vector<int32_t> sessFree;   // free session-ticket ids (stack)
  // co-workers (mrp_ll_submit_tagged / mrp_ll_poll_any_tagged): two host threads that share this context's session
  static constexpr int kMaxTags = 4;
  std::mutex coMu;
  std::vector<int32_t> coStash[kMaxTags];        // finished tickets another co-worker's poll has come across (not released yet)
  std::atomic<int32_t> coStashCount[kMaxTags];
  std::vector<int32_t> sippTabFree;  // device-resident SIPP tables (env.sippTabChunks): free pool indices, next unused one
  int32_t sippTabNext = 0;
  uint16_t* pathStore = nullptr;   // device-resident path store (mrp_ll_path_store_reserve; slots: env.pathStoreSlots)
  uint32_t pathStoreStride = 0;
  uint32_t* consStore = nullptr;   // device-resident constraint store (mrp_ll_constraint_store_reserve; geometry and mirror: env)
  uint8_t* scanDev = nullptr;      // mrp_ll_conflict_scan and the heuristic calls: device staging (grown on demand)
  size_t scanDevCap = 0;
  hipStream_t scanStream = nullptr;  // ... and the scan's own stream: a session's resident kernel occupies tickets[0].stream
  std::vector<uint16_t> scanStates;
  mrp::host::AssignStaging assignStaging;  // mrp_ll_assign_batch / _series_*: the packed batch (kept for its capacity)
  std::vector<uint32_t> assignOut;         // ... and its result records
  mrp::host::AssignStagingWide assignStagingWide;         // the same of mrp_ll_assign_batch_w
  uint32_t assignLdsBudget = mrp::as::kLdsBudgetWide;     // LDS rows up to here, memory rows beyond (MRP_LL_ASSIGN_LDS_BYTES)
};

namespace {

const bool kDebug = std::getenv("MRP_LL_DEBUG") != nullptr;
#define HIPCHK(ctx, call)                                                                         \
  do {                                                                                            \
    if (kDebug) { std::fprintf(stderr, "[mrp_ll] %s\n", #call); std::fflush(stderr); }            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                            \
      return MRP_LL_E_DEVICE;                                                                     \
    }                                                                                             \
  } while (0)

// A session is active or a batch is in flight: the maps buffer, the stores and the tier geometry must stay as they are.
bool engineBusy(const mrp_ll_ctx* ctx) {
  if (ctx->env.session.active) return true;
  for (const Ticket& t : ctx->tickets)
    if (t.inFlight) return true;
  return false;
}

// A job's result has come back: the chain's or the search's result, the conflicts of a flagged job, the constraint set it
// wrote, the report to its SIPP table.  outArea / outStride: the job's host output area (halfwords).
void collectJob(mrp_ll_ctx* ctx, JobNote& n, const DevResult& d, const uint16_t* outArea, uint32_t outStride, mrp_ll_result& r,
                mrp_ll_conflict* c) {
  if (n.chain)
    unpackChain(ctx->stats, d, outArea, n.rejected != 0, r, n.chain, outStride / 2u);
  else
    unpackResult(ctx->stats, d, outArea, n.rejected != 0, r, n.dimx != 0, n.dimx, n.init);
  if (n.scan) unpackConflicts(d, outArea, outStride, n.rejected != 0, *c);
  setCollected(ctx->env, n.setSlot, n.setSeq);
  n.setSlot = -1;
  if (n.table) {
    finishSippTableJob(n.table, n.sippFlags, d, outArea);
    n.table = nullptr;
  }
}

}  // namespace
