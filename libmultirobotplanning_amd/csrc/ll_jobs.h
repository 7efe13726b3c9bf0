// From a job descriptor to a search: the LDS window's size, the host / path-store access helpers (hostLoad32, hostStore32,
// storeLoad), job staging shared by all searches (stageConstraints, fillCtx, baseCJob, putCJob / getCRes), the arena slot's
// cut (cutHeaps, cutArena, compactFits), the by-id focal table build (buildIdTableInArena), and the two CBS / ECBS job runners:
// runJob (stageFocalTable, compactAttempt, then arenaAttempt) and runChain (the root chain of an ECBS conflict tree), with what they share with the other job loops
// (publishPath, beginJob / endJob).
// Needs ll_slot.h (slot::), ll_compact.h (ct::), ll_arena_heap.h and ll_arena_search.h.
#ifndef MRP_LL_JOBS_H
#define MRP_LL_JOBS_H

namespace mrp {

// ---- LDS layout ------------------------------------------------------------------------------------------------
// Dynamic LDS of a CBS / ECBS workgroup: the compact tier's window (ll_compact.h: open list, focal list, walk queue,
// (time, cell) bitmap, obstacle row), then the focal path table.  A search that has left the compact tier keeps the
// heaps' top entries in the same window (TierHyb).
// bg: the window of the A*-epsilon-only kernels (ll_compact.h BG: the (time, cell) bitmap lives in the arena slot)
__host__ __device__ inline uint32_t ldsBytes(uint32_t pathBytes, bool bg) { return ct::windowBytes(bg) + pathBytes; }

// A read of the device path store.  The slot was written by another workgroup (another CU, possibly another XCD) of the
// same resident launch before its completion was published; an agent-scope load goes past this CU's L1 to the coherent
// level, so no cache has to be invalidated for it (a per-job acquire fence would drop the whole L1 of the CU under the
// ten other searches that share it).
DEVI uint32_t storeLoad(const uint16_t* p) {
#ifdef MRP_LL_STORE_ACQUIRE_FENCE
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// Words the HOST wrote (job descriptors, constraint words, id lists, shipped tables) and words the host READS (result
// records, paths): system-scope accesses that go past this XCD's L2 in both directions.  The resident loop publishes and
// consumes jobs without cache-wide fences (residentLoop), so nothing else guarantees that a plain load of a recycled job
// slot does not find the previous occupant in L2, or that a plain store has left it when the done word is written.
DEVI uint32_t hostLoad32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
DEVI void hostStore32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// ---- job staging shared by the searches (runJob, runChain, runJobTA, runJobTaEps, runSipp) -----------------------------
// The job's constraint words leave host memory in one coalesced pass into the arena's copy area; a list of more than
// kConsLocalWords words is read where the host put it, with plain loads behind one acquire fence.  The vertex words and
// the edge words are ONE run: the host packer pushes them back to back, ec_off == vc_off + n_vc (host/ll_pack.h packJob).
DEVI void stageConstraints(const uint32_t* consHost, uint32_t vcOff, uint32_t nVc, uint32_t nEc, uint32_t* consLocal,
                           const uint32_t*& vc, const uint32_t*& ec) {
  const uint32_t* src = consHost + vcOff;
  const uint32_t nWords = nVc + nEc;
  if (nWords <= kConsLocalWords) {
    for (uint32_t i = threadIdx.x; i < nWords; i += 64) consLocal[i] = hostLoad32(src + i);
    vc = consLocal;
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    vc = src;
  }
  ec = vc + nVc;
}

// The same for a job that names its set in the device-resident constraint store (DevJob::pad_, mrp_ll_submit_sets): the union
// is put together in the copy area in the order  base vertex words, added vertex words, base edge words, added edge words
// — ec == vc + nVc as above —, base words from the store, added words from host memory, and, with a result slot, written
// out to it before the search starts (a front workgroup and the heavy workgroup it hands the search to both do, with the
// same words).  Store accesses follow the path store's discipline (storeLoad): agent-scope loads and stores, complete
// before the job's completion is published (publishDone waits for vmcnt), no cache-wide fence.
// A word read from the store is checked against the job's map before anybody indexes with it (buildRows / ensureRows use
// the vertex words unguarded): one that does not fit becomes 0xFFFFFFFF, which no tier matches or indexes with.
// A function of its own, called by processJob before anything of the search is live: the resident kernels' register
// allocation is the searches', not this loop's.
// Returns false when the descriptor does not fit the store or the copy area (the host packer refuses such a job).
__device__ __attribute__((noinline)) bool stageConstraintSet(const DevJob* job, const uint32_t* cons, uint32_t* store, uint32_t stride,
                                                             uint32_t slots, uint32_t* consLocal) {
  const uint32_t nVc = rfl(job->n_vc), nEc = rfl(job->n_ec), dimx = rfl(job->dimx), dimy = rfl(job->dimy);
  const uint32_t baseP1 = rfl(job->pad_[0]), baseCounts = rfl(job->pad_[1]), resP1 = rfl(job->pad_[2]);
  const uint32_t* added = cons + rfl(job->vc_off);
  stride = rfl(stride); slots = rfl(slots);
  const uint32_t bVc = baseP1 ? (baseCounts & 0xFFFFu) : 0u, bEc = baseP1 ? (baseCounts >> 16) : 0u;
  const uint32_t nWords = nVc + nEc;
  if (store == nullptr || baseP1 > slots || resP1 > slots || bVc > nVc || bEc > nEc || nVc > kConsLocalWords ||
      nEc > kConsLocalWords || nWords > kConsLocalWords || nWords > stride)
    return false;
  const uint32_t aVc = nVc - bVc;
  const uint32_t cells = dimx * dimy;
  const uint32_t* base = store + (size_t)(baseP1 ? baseP1 - 1u : 0u) * stride;
  uint32_t* out = store + (size_t)(resP1 ? resP1 - 1u : 0u) * stride;
  for (uint32_t i = threadIdx.x; i < nWords; i += 64) {
    uint32_t w;
    if (i < nVc) {
      if (i < bVc) {
        w = __hip_atomic_load(base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // t << 16 | y << 8 | x
        if ((w & 0xFFu) >= dimx || ((w >> 8) & 0xFFu) >= dimy) w = 0xFFFFFFFFu;
      } else {
        w = hostLoad32(added + (i - bVc));
      }
    } else {
      const uint32_t k = i - nVc;
      if (k < bEc) {
        w = __hip_atomic_load(base + bVc + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // t << 19 | cell << 3 | k
        if (((w >> 3) & 0xFFFFu) >= cells) w = 0xFFFFFFFFu;
      } else {
        w = hostLoad32(added + aVc + (k - bEc));
      }
    }
    consLocal[i] = w;
    if (resP1) __hip_atomic_store(out + i, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return true;
}

// What a search's Ctx takes from the job descriptor; vc / ec (stageConstraints) and the path table are the caller's.
// UNI: the descriptor is read through a pointer the compiler cannot prove wave-uniform (runJobTaEps's argument).
template <bool UNI = false>
DEVI void fillCtx(Ctx& c, const DevJob& J, const uint32_t* maps, volatile uint32_t* debug) {
  auto u = [](uint32_t v) { return UNI ? rfl(v) : v; };
  c.dimx = u(J.dimx); c.dimy = u(J.dimy); c.wpr = u(J.words_per_row);
  c.gx = u(J.gx); c.gy = u(J.gy); c.sx = u(J.sx); c.sy = u(J.sy);
  c.lastGoal = (int32_t)u((uint32_t)J.last_goal_constraint);
  c.w = __builtin_bit_cast(float, u(__builtin_bit_cast(uint32_t, J.w)));
  c.nVc = u(J.n_vc); c.nEc = u(J.n_ec);
  c.obst = maps + u(J.map_word_off);
  c.nAgentsPad = u(J.n_agents_pad); c.tPad = u(J.t_pad);
  c.maxExp = UNI ? (int64_t)rfl64((uint64_t)J.max_expansions) : J.max_expansions;
  c.debug = debug;
}

// A compact-tier job goes into its block of the LDS window (every lane stores the same words) and the result comes back
// from there: the ct:: searches are real functions with their own register allocation.
DEVI void putCJob(uint8_t* smem, const ct::CJob& cj) {
  auto w32 = (__attribute__((address_space(3))) uint32_t*)((wv::Lds)smem + ct::oJob);
  const uint32_t* src = (const uint32_t*)&cj;
#pragma unroll
  for (uint32_t q = 0; q < sizeof(ct::CJob) / 4; ++q) w32[q] = src[q];
}
DEVI ct::CRes getCRes(uint8_t* smem) {
  auto r32 = (__attribute__((address_space(3))) const uint32_t*)((wv::Lds)smem + ct::oRes);
  ct::CRes cr;
  cr.status = (int32_t)rfl(r32[0]); cr.cost = (int32_t)rfl(r32[1]); cr.fmin = (int32_t)rfl(r32[2]);
  cr.nStates = (int32_t)rfl(r32[3]); cr.expanded = rfl(r32[4]); cr.nodes = rfl(r32[5]);
  return cr;
}
// The narrow geometry as mrp_ll_configure_tiers sized it: lds_nodes / 2 = open-list entries, lds_rows = time steps a
// search may use inside the tier; and the expansion budget in the tier's 32 bits (all ones: unlimited).
DEVI uint32_t narrowOpenCap(const LaunchParams& P) { return P.lds_nodes / 2u < ct::kCap ? P.lds_nodes / 2u : ct::kCap; }
DEVI uint32_t narrowMaxT(const LaunchParams& P) {
  return P.lds_rows >= 3u && P.lds_rows - 2u < ct::kMaxT ? P.lds_rows - 2u : ct::kMaxT;
}
DEVI uint32_t clampMaxExp(int64_t maxExp) {
  return maxExp < 0 ? 0xFFFFFFFFu : (maxExp > 0xFFFFFFFEll ? 0xFFFFFFFEu : (uint32_t)maxExp);
}

// Three heap arrays (open, focal, walk queue) of `cap` 64-bit entries each from `p` on, every one with the bias slot in
// front of it; returns the first byte behind them.
DEVI uint8_t* cutHeaps(Mem<TierHbm>& g, uint8_t* p, uint32_t cap) {
  g.open = (Mem<TierHbm>::PE)(p + 8);          p += (size_t)cap * 8 + 16;
  g.focal = (Mem<TierHbm>::PE)(p + 8);         p += (size_t)cap * 8 + 16;
  g.aux = (Mem<TierHbm>::PE)(p + 8);           p += (size_t)cap * 8 + 16;
  g.capNodes = cap; g.capHeap = cap;
  return p;
}
// The arena slot as most searches use it: arena_nodes node records, the three heaps, the (time, cell) bitmap.
DEVI Mem<TierHbm> cutArena(const LaunchParams& P, uint8_t* arenaSlot) {
  Mem<TierHbm> g = {};
  g.nodes = (Mem<TierHbm>::PN32)arenaSlot;
  g.bits = (Mem<TierHbm>::P32)cutHeaps(g, arenaSlot + slot::nodeBytes(P.arena_nodes), P.arena_nodes);
  g.capRows = P.arena_rows; g.rowWords = P.arena_row_words;
  return g;
}
// The compact tiers' claim on the slot's node area, free while a search is in them: the cameFrom table of geometry Geo for
// `rows` time steps (the narrow geometry: always its own kRows) at offset 0 and, BG, the (time, cell) bitmap behind it.
template <class Geo>
DEVI bool compactFits(uint32_t arenaNodes, uint32_t rows, bool bg) {
  return slot::nodeBytes(arenaNodes) >= Geo::parentBytes(rows) + (bg ? Geo::bitsBytes(rows) : 0u);
}
// What every compact-tier job takes from the descriptor and the launch: map, budget, narrow limits, the slot's areas as
// above.  The caller adds start, goal, constraints and focal table, and replaces what differs.
template <class Geo = ct::Narrow>
DEVI ct::CJob baseCJob(const LaunchParams& P, const DevJob& J, uint8_t* arenaSlot, uint16_t* outPath, uint32_t rows = 0) {
  ct::CJob cj;
  cj.dimx = J.dimx; cj.dimy = J.dimy; cj.w = J.w; cj.obstWords = J.words_per_row;
  cj.obst = (uint64_t)(P.maps + J.map_word_off);
  cj.maxExp = clampMaxExp(J.max_expansions);
  cj.openCap = narrowOpenCap(P); cj.maxT = narrowMaxT(P); cj.taNoGoal = 0; cj.rows = 0;
  cj.parentTab = (uint64_t)arenaSlot; cj.bitsG = (uint64_t)(arenaSlot + Geo::parentBytes(rows)); cj.outPath = (uint64_t)outPath;
  return cj;
}

// Which tiers a kernel carries:
//   kTiersAll   — compact (narrow) tier, then the arena tier: batch kernels, CBS / mixed sessions, A*-epsilon sessions
//                 without heavy workgroups;
//   kTiersFront — the compact (narrow) tier only: a search it cannot hold is handed to the heavy workgroups (runJob returns
//                 true, nothing of the job has been reported); no arena-tier code in the kernel;
//   kTiersHeavy — the compact tier in its WIDE geometry (3071 open entries, long horizons, ll_compact.h), then the arena tier.
enum : int { kTiersAll = 0, kTiersFront = 1, kTiersHeavy = 2 };

// Where runJob builds the focal table of a job that names its paths by path-store ids: behind the LDS window when it fits
// there (never behind the wide window), else in the arena slot's path area.  (Also asked by processJob's conflict scan.)
template <int TIERS>
DEVI bool idTableInLds(const LaunchParams& P, uint32_t pathBytes) {
  return TIERS != kTiersHeavy && P.lds_nodes != 0 && pathBytes <= P.lds_paths_bytes;
}

// A front workgroup hands these searches over without looking at them (runJob's first test, kTiersFront).
DEVI bool frontHandsOver(const LaunchParams& P, const DevJob& J) {
  return (J.ctx_flags & kCtxHeavy) != 0 || P.lds_nodes == 0 || J.dimx > 32u || J.dimy > 32u || J.n_agents_pad > 128u || J.n_ec > 64u;
}

// ---- a focal table built from the path store (kCtxById): what stageFocalTable and runJobTaEps (ll_ta.h) share -----------
// The table starts as kEmptyCell everywhere; the barrier stands between the fill and the columns' stores.
// The slots named by a job were written by OTHER workgroups of this same resident launch (possibly on another XCD,
// whose L2 is not coherent with ours), each before its job's completion was published (processJob writes them in
// front of residentLoop's system-scope release), and slots are recycled.  Every read of the store is therefore a storeLoad:
// an agent-scope load that goes past this CU's L1 to the coherent level.  (MRP_LL_STORE_ACQUIRE_FENCE, the A/B build: one
// agent-scope acquire drops whatever stale copies this CU's L1 / this XCD's L2 may hold from an earlier use of a recycled
// slot; after it plain, cached, coalesced loads are correct — MI355X_MICROARCH.md "Valid forms": poll -> ONE acquire ->
// s_waitcnt -> barrier -> plain loads.)
DEVI void clearIdTable(uint16_t* dst, uint32_t pathBytes) {
  uint32_t* d32 = (uint32_t*)dst;
  for (uint32_t i = threadIdx.x; i < pathBytes / 4; i += 64) d32[i] = 0xFFFFFFFFu;  // kEmptyCell everywhere
#ifdef MRP_LL_STORE_ACQUIRE_FENCE  // A/B: one fence + plain loads instead of agent-scope loads
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  __syncthreads();
}
// Agents a0 .. a0 + 63 of the id list, one per lane: the slot and its length word (one gather for all lengths).  An id
// outside the store — kNoStoreSlot: an empty path, the searching agent itself — has length 0.
DEVI void loadIdChunk(const uint32_t* ids, uint32_t a0, uint32_t nCtx, const uint16_t* store, uint32_t stride, uint32_t slots,
                      uint32_t& idL, uint32_t& lenL) {
  const uint32_t lane = threadIdx.x;
  idL = kNoStoreSlot; lenL = 0;
  if (a0 + lane < nCtx) idL = hostLoad32(ids + a0 + lane);
  if (idL < slots) lenL = storeLoad(store + (size_t)idL * stride);
  if (lenL > stride - 1) lenL = stride - 1;
}
// The table [tPad][nAgentsPad] in the arena (global memory) at dst: one lane per AGENT, agents in chunks of 64, so that a
// row of the table is one coalesced store (a lane per time step would scatter 2-byte stores 2 * n_agents_pad bytes apart
// — measured on agents100: the longest conflict-tree chain of a batch a third slower).  The reads gather one cell per slot
// and stay in L2 from row to row; eight rows are in flight at a time.  A path shorter than tPad is held at its last cell; an
// id outside the store or a zero length word leaves the column empty.  The caller has made sure that the table fits at dst
// and that nCtx <= nAgentsPad, and puts a barrier between this and the first read of the table.
DEVI void buildIdTableInArena(uint16_t* dst, const uint32_t* ids, uint32_t nCtx, uint32_t tPad, uint32_t nAgentsPad,
                              const uint16_t* store, uint32_t stride, uint32_t slots) {
  const uint32_t lane = threadIdx.x;
  clearIdTable(dst, tPad * nAgentsPad * 2);
  for (uint32_t a0 = 0; a0 < nCtx; a0 += 64) {
    uint32_t idL, lenA;
    loadIdChunk(ids, a0, nCtx, store, stride, slots, idL, lenA);
    const uint16_t* slotA = store + (size_t)(idL < slots ? idL : 0) * stride + 1;
    const bool hasA = idL < slots && lenA != 0;
    for (uint32_t t0 = 0; t0 < tPad; t0 += 8) {
      uint32_t v[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t t = t0 + u;
        v[u] = kEmptyCell;
        if (hasA && t < tPad) v[u] = storeLoad(slotA + (t < lenA ? t : lenA - 1));
      }
#pragma unroll
      for (uint32_t u = 0; u < 8; ++u)
        if (hasA && t0 + u < tPad) dst[(t0 + u) * nAgentsPad + a0 + lane] = (uint16_t)v[u];
    }
  }
}

// runJob's first phase: the job's focal path table leaves host memory, or is built from the path store, in one coalesced
// pass — into `ldsPaths` (behind the LDS window) when it fits there, else into `pathsArena` (the slot's path-table copy).
// Leaves where the table is in c.paths / c.pathsLds; false: a table named by ids fits nowhere (nothing was written).
template <int TIERS>
DEVI bool stageFocalTable(const LaunchParams& P, const DevJob& J, uint8_t* ldsPaths, uint8_t* pathsArena, Ctx& c) {
  constexpr bool kTableMayBeInLds = TIERS != kTiersHeavy;  // the wide window holds no path table
  const uint32_t lane = threadIdx.x;
  const uint32_t pathBytes = c.tPad * c.nAgentsPad * 2;  // multiple of 32
  const uint32_t* psrc = (const uint32_t*)(P.paths + J.path_off);
  c.pathsLds = nullptr;
  if (pathBytes != 0 && (J.ctx_flags & kCtxById)) {
    // f2: the CT node's paths are named by their slots in the device-resident path store (each was written there by
    // the search that produced it); the time-major table [t][agent] is built here, on the device, instead of being
    // packed by the host and read over PCIe.
    const bool inLds = idTableInLds<TIERS>(P, pathBytes);
    if (!inLds && pathBytes > P.arena_paths_bytes) return false;  // (the host packer refuses such a job; never write past the slot)
    uint16_t* dst = inLds ? (uint16_t*)ldsPaths : (uint16_t*)pathsArena;
    const uint32_t* ids = P.cons + J.path_off;
    const uint32_t nCtx = J.n_ctx;
    if (!inLds) {
      buildIdTableInArena(dst, ids, nCtx, c.tPad, c.nAgentsPad, P.path_store, P.path_store_stride, P.path_store_slots);
    } else {
      // table in LDS: a lane per time step (one coalesced read per agent); eight agents' loads are in flight before
      // the first store
      clearIdTable(dst, pathBytes);
      for (uint32_t a0 = 0; a0 < nCtx; a0 += 64) {
        uint32_t idL, lenL;
        loadIdChunk(ids, a0, nCtx, P.path_store, P.path_store_stride, P.path_store_slots, idL, lenL);
        const uint32_t nHere = nCtx - a0 < 64 ? nCtx - a0 : 64;
        for (uint32_t t0 = 0; t0 < c.tPad; t0 += 64) {
          const uint32_t t = t0 + lane;
          for (uint32_t q0 = 0; q0 < nHere; q0 += 8) {
            uint32_t v[8];
            bool has[8];
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) {
              uint32_t id = kNoStoreSlot, len = 0;
              if (q0 + u < nHere) {
                id = __builtin_amdgcn_readlane(idL, q0 + u);
                len = __builtin_amdgcn_readlane(lenL, q0 + u);
              }
              has[u] = id < P.path_store_slots && len != 0 && t < c.tPad;  // not: empty path / the searching agent itself
              v[u] = kEmptyCell;
              if (has[u]) v[u] = storeLoad(P.path_store + (size_t)id * P.path_store_stride + 1 + (t < len ? t : len - 1));
            }
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u)
              if (has[u]) dst[t * c.nAgentsPad + a0 + q0 + u] = (uint16_t)v[u];
          }
        }
      }
    }
    c.paths = dst;
    if (inLds) c.pathsLds = (__attribute__((address_space(3))) const uint16_t*)ldsPaths;
  } else if (pathBytes == 0) {
    c.paths = nullptr;
  } else if (kTableMayBeInLds && P.lds_nodes != 0 && pathBytes <= P.lds_paths_bytes) {
    uint32_t* dst = (uint32_t*)ldsPaths;
    for (uint32_t i = lane; i < pathBytes / 4; i += 64) dst[i] = hostLoad32(psrc + i);
    c.paths = (const uint16_t*)ldsPaths;
    c.pathsLds = (__attribute__((address_space(3))) const uint16_t*)ldsPaths;
  } else if (pathBytes <= P.arena_paths_bytes) {
    uint32_t* dst = (uint32_t*)pathsArena;
    for (uint32_t i = lane; i < pathBytes / 4; i += 64) dst[i] = hostLoad32(psrc + i);
    c.paths = (const uint16_t*)pathsArena;
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    c.paths = P.paths + J.path_off;
  }
  return true;
}

// runJob's second phase, the compact tier (ll_compact.h): the whole search in LDS, a state = its 32-bit heap entry.  Maps up
// to 32 x 32 and up to 128 agents in the focal context; a search that outgrows the tier (open list, time steps, focalH
// field) comes back as C_OVERFLOW with nothing of it observable, and is run again from the start by the next tier.
// Returns true when the search ended here: its answer is in rc, res and s.
// TH (runJobTableH): the table form of the narrow tier (ll_compact.h): h from the 2 KiB table `heur`, which the search copies
// into the window's path area behind a focal table that stands there.
template <bool EPS, bool BG, int TIERS, bool TH = false>
DEVI bool compactAttempt(const LaunchParams& P, const DevJob& J, uint8_t* smem, uint8_t* arenaSlot, const Ctx& c, DevResult& res,
                         uint16_t* outPath, SState& s, int& rc, const uint16_t* heur = nullptr) {
  static_assert(!TH || (!BG && TIERS == kTiersAll), "the table form exists for the mixed kernels' narrow tier");
  typedef typename std::conditional<TIERS == kTiersHeavy, ct::Wide, ct::Narrow>::type Geo;
  // the wide geometry: as many time steps as the arena slot's node area has room for (cameFrom table + bitmap), in
  // chunks of 64, up to the job's horizon
  uint32_t geoRows = Geo::kRows;
  if (TIERS == kTiersHeavy) {
    const uint64_t room = slot::nodeBytes(P.arena_nodes) / (1024u + ct::kRowBytes);
    geoRows = (uint32_t)(room < P.arena_rows ? room : P.arena_rows) & ~63u;
  }
  const bool compactOk = !(TIERS == kTiersAll && (J.ctx_flags & kCtxHeavy) != 0) && P.lds_nodes != 0 && c.dimx <= 32u &&
                         c.dimy <= 32u && c.nAgentsPad <= 128u && c.nEc <= 64u && geoRows >= 64u &&
                         compactFits<Geo>(P.arena_nodes, geoRows, BG) &&
                         (!TH || P.lds_paths_bytes >= 2048u + (EPS && c.pathsLds != nullptr ? c.tPad * c.nAgentsPad * 2u : 0u));
  bool done = false;
  if (compactOk) {
    ct::CJob cj = baseCJob<Geo>(P, J, arenaSlot, outPath, geoRows);
    cj.obstWords = c.wpr;  // (the Ctx's copy, live for the arena tier anyway: the descriptor's, read again, costs the all-tier kernels a VGPR)
    cj.sx = c.sx; cj.sy = c.sy; cj.gx = c.gx; cj.gy = c.gy;
    cj.lastGoal = c.lastGoal;
    cj.nVc = c.nVc; cj.nEc = c.nEc;
    cj.nAgentsPad = EPS ? c.nAgentsPad : 0u; cj.tPad = c.tPad;
    cj.rows = geoRows;
    if (TIERS == kTiersHeavy) {  // the wide geometry at its full size
      cj.openCap = Geo::kCap;
      cj.maxT = Geo::kMaxT < geoRows - 2u ? Geo::kMaxT : geoRows - 2u;
    }
    cj.vc = (uint64_t)c.vc; cj.ec = (uint64_t)c.ec;
    cj.pathsG = (uint64_t)c.paths;
    if constexpr (TH) cj.bitsG = (uint64_t)heur;  // (free in a BG = false job)
    putCJob(smem, cj);
    const bool tableInLds = !EPS || c.nAgentsPad == 0u || c.pathsLds != nullptr;
#ifndef MRP_LL_TRACE  // (the trace build uses prof[] for its phase counters)
    const uint64_t tl0 = __builtin_amdgcn_s_memrealtime();
#endif
    int32_t crc;
    if constexpr (TH && !EPS)
      crc = ct::compactSearch<false, true, false, ct::Narrow, true>((wv::Lds)smem);
    else if constexpr (TH)
      crc = tableInLds ? ct::compactSearch<true, true, false, ct::Narrow, true>((wv::Lds)smem)
                       : ct::compactSearch<true, false, false, ct::Narrow, true>((wv::Lds)smem);
    else if constexpr (TIERS == kTiersHeavy)
      crc = ct::compactSearch<EPS, false, BG, ct::Wide>((wv::Lds)smem);
    else
      crc = tableInLds ? ct::compactSearch<EPS, true, BG>((wv::Lds)smem) : ct::compactSearch<EPS, false, BG>((wv::Lds)smem);
    const ct::CRes cr = getCRes(smem);
#ifndef MRP_LL_TRACE
    // 100 MHz ticks / expansions in the compact tier (of a search that was handed over: until then); the wide geometry
    // reports into the arena tier's pair — "the searches that outgrew the narrow tier"
    res.prof[TIERS == kTiersHeavy ? 2 : 0] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);
    res.prof[TIERS == kTiersHeavy ? 3 : 1] = cr.expanded;
#endif
#ifdef MRP_CT_PROF  // diagnostic build: the compact tier's own phase counters instead of the tier statistics
    {
      auto r32 = (__attribute__((address_space(3))) const uint32_t*)((wv::Lds)smem + ct::oRes + 32u);
      for (uint32_t q = 0; q < 8; ++q) res.prof[q] = rfl(r32[q]);
    }
#endif
    if (crc != ct::C_OVERFLOW) {
      rc = crc;  // C_OK / C_NO_SOLUTION / C_CAP_EXP == ST_OK / ST_NO_SOLUTION / ST_CAP_EXP
      res.cost = cr.cost; res.fmin = cr.fmin; res.n_states = cr.nStates;
      s.expansions = cr.expanded; s.nNodes = cr.nodes;
      done = true;
      if (TIERS == kTiersHeavy) res.tier = 2;
    } else {
#ifndef MRP_LL_TRACE
      res.prof[6] = cr.expanded;  // expansions thrown away with the attempt
      res.prof[7] = 1;
#endif
    }
  }
  return done;
}

// runJob's third phase, the arena tier: the search from the start with its state in the arena slot (cutArena) and the heaps'
// top levels in the LDS window.  Returns runSearch's code.
// TH (runJobTableH): the searches read h from the shortest-path table `heur` (ll_arena_search.h).
template <bool EPS, bool BG, int TIERS, bool TH = false>
DEVI int arenaAttempt(const LaunchParams& P, uint8_t* smem, uint8_t* arenaSlot, const Ctx& c, DevResult& res, uint16_t* outPath,
                      SState& s, const uint16_t* heur = nullptr, uint32_t heurStride = 0) {
  typedef typename std::conditional<TIERS == kTiersHeavy, ct::Wide, ct::Narrow>::type Geo;
  int rc;
  // HBM tier view of this workgroup's arena slot
  const Mem<TierHbm> g = cutArena(P, arenaSlot);
  // ... and the view the arena tier actually runs on: the same arrays, the heaps' first nTop entries in this
  // workgroup's LDS (the compact tier's area, free once a search has left it)
  Mem<TierHyb> gh = viewAs<TierHyb>(g);
  {
    const uint32_t area = Geo::windowBytes(BG) - ct::oOpen;  // (the window's control blocks in front of it stay as they are)
    // the open list gets half of the area, the focal list five sixteenths, the walk queue the rest (MRP_LL_TOPS_EQUAL:
    // thirds, as before the A*-epsilon kernels' window shrank)
#ifdef MRP_LL_TOPS_EQUAL
    const uint32_t perO = (area / 3u) & ~15u, perF = perO, perA = perO;
#else
    const uint32_t perO = (area / 2u) & ~15u, perF = (area * 5u / 16u) & ~15u, perA = (area - perO - perF) & ~15u;
#endif
    auto tops = [&](uint32_t per) {
      uint32_t n = per >= 32u ? ((per - 8u) / 8u) : 0u;
      if (n > 4095u) n = 4095u;
      n = n ? ((n - 1u) | 1u) : 0u;  // odd (or 0: no LDS tier configured)
      return P.lds_nodes == 0 ? 0u : n;
    };
    auto l8 = (__attribute__((address_space(3))) uint8_t*)smem + ct::oOpen;
    gh.open = HybPtr{(__attribute__((address_space(3))) uint64_t*)(l8 + 8), (uint64_t*)g.open, tops(perO)};
    gh.focal = HybPtr{(__attribute__((address_space(3))) uint64_t*)(l8 + perO + 8), (uint64_t*)g.focal, tops(perF)};
    gh.aux = HybPtr{(__attribute__((address_space(3))) uint64_t*)(l8 + perO + perF + 8), (uint64_t*)g.aux, tops(perA)};
  }
  const bool xyEntries = P.arena_nodes <= 65536u;  // TierHybXy: 16-bit node ids leave room for the cell in the entry
  Mem<TierHybXy> ghx = viewAs<TierHybXy>(gh);
  res.tier = 1;
  __syncthreads();  // previous job's / the compact attempt's LDS accesses are done
  if constexpr (TH) {
    if (xyEntries)
      initSearch<TierHybXy, EPS, true>(ghx, s, c, heur, heurStride);
    else
      initSearch<TierHyb, EPS, true>(gh, s, c, heur, heurStride);
  } else if (xyEntries)
    initSearch<TierHybXy, EPS>(ghx, s, c);
  else
    initSearch<TierHyb, EPS>(gh, s, c);
  __syncthreads();
#ifndef MRP_LL_TRACE
  const uint64_t th0 = __builtin_amdgcn_s_memrealtime();
#endif
  if constexpr (TH) {
    if (xyEntries)
      rc = runSearch<TierHybXy, EPS, true>(ghx, s, c, res, outPath, heur, heurStride);
    else
      rc = runSearch<TierHyb, EPS, true>(gh, s, c, res, outPath, heur, heurStride);
  } else if (xyEntries)
    rc = runSearch<TierHybXy, EPS>(ghx, s, c, res, outPath);
  else
    rc = runSearch<TierHyb, EPS>(gh, s, c, res, outPath);
#ifndef MRP_LL_TRACE
  if (TIERS != kTiersHeavy) {
    res.prof[2] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - th0);
    res.prof[3] = (uint32_t)s.expansions;
  }
#endif
  return rc;
}

// One CBS / ECBS job: its constraint words and focal table into place, then the compact tier, then the arena tier.
// Returns true when the job has to be handed to the heavy workgroups (kTiersFront only).
template <bool EPS, bool BG, int TIERS>
DEVI bool runJob(const LaunchParams& P, const DevJob& J, uint8_t* smem, uint8_t* arenaSlot, DevResult& res,
                 uint16_t* outPath) {
  typedef typename std::conditional<TIERS == kTiersHeavy, ct::Wide, ct::Narrow>::type Geo;
  // not a search of the narrow tier (the caller says so, or the job's shape does): nothing to set up here
  if (TIERS == kTiersFront && frontHandsOver(P, J)) return true;
  Ctx c;
  fillCtx(c, J, P.maps, P.debug);
  uint32_t* consLocal = slot::consCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  if ((J.pad_[0] | J.pad_[2]) != 0u) {  // the union is in the copy area already (processJob, stageConstraintSet)
    c.vc = consLocal;
    c.ec = consLocal + c.nVc;
  } else {
    stageConstraints(P.cons, J.vc_off, c.nVc, c.nEc, consLocal, c.vc, c.ec);
  }
  if (!stageFocalTable<TIERS>(P, J, smem + Geo::windowBytes(BG), slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride), c)) {
    res.status = ST_BAD; res.expanded = 0; res.nodes_created = 0;
    return false;
  }
  __syncthreads();
  SState s;
  int rc = ST_BAD;
  res.tier = 0;
  if (!compactAttempt<EPS, BG, TIERS>(P, J, smem, arenaSlot, c, res, outPath, s, rc)) {
    if constexpr (TIERS == kTiersFront)
      return true;  // the heavy workgroups run it from the start
    else
      rc = arenaAttempt<EPS, BG, TIERS>(P, smem, arenaSlot, c, res, outPath, s);
  }
  if (rc == RUN_MIGRATE_NODES) rc = ST_CAP_NODES;
  if (rc == RUN_MIGRATE_ROWS) rc = ST_CAP_HORIZON;
  res.status = rc;
  res.expanded = s.expansions;
  res.nodes_created = s.nNodes;
  return false;
}

// One CBS / ECBS job with MRP_LL_JOB_TABLE_H (ll_device.h kCtxTableH): runJob's staging, then the arena tier with h read from
// the goal's shortest-path table in the maps buffer — rows of 32 halfwords on maps up to 32 x 32, of dimx beyond
// (host/ll_pack.h heurStride).  The table belongs to the job's map (the packer checked), so every cell of the map has a
// halfword in it; what the halfwords SAY is the caller's: a value that does not fit f's field ends the job
// ST_CAP_HORIZON.  A start the table calls unreachable is answered at once: ST_NO_SOLUTION, nothing expanded.
// A real function with plain values for arguments (as runJobTaEps is, ll_ta.h): its own register allocation, and the mixed
// kernels keep theirs.  The job is read where the kernel staged it; status, cost, fmin, n_states, expanded, nodes_created and
// tier go to `out`.  The arguments arrive in vector registers and are made wave-uniform here.
template <bool EPS>
__device__ __attribute__((noinline)) void runJobTableH(const DevJob* Jp, DevResult* out, uint8_t* smem, uint8_t* arenaSlot,
                                                       const uint32_t* maps, const uint32_t* consHost, const uint16_t* pathsHost,
                                                       uint32_t scratchOff, uint32_t outStride, uint32_t arenaNodes,
                                                       uint32_t arenaRows, uint32_t arenaRowWords, uint32_t arenaPathsBytes,
                                                       uint32_t ldsNodes, uint32_t ldsPathsBytes) {
  LaunchParams P = {};  // what the staging and the arena tier read of the launch
  P.maps = (const uint32_t*)rfl64((uint64_t)maps);
  P.cons = (const uint32_t*)rfl64((uint64_t)consHost);
  P.paths = (const uint16_t*)rfl64((uint64_t)pathsHost);
  P.arena_scratch_off = rfl(scratchOff); P.out_stride = rfl(outStride);
  P.arena_nodes = rfl(arenaNodes); P.arena_rows = rfl(arenaRows); P.arena_row_words = rfl(arenaRowWords);
  P.arena_paths_bytes = rfl(arenaPathsBytes);
  P.lds_nodes = rfl(ldsNodes); P.lds_paths_bytes = rfl(ldsPathsBytes);
  smem = (uint8_t*)rfl64((uint64_t)smem);
  arenaSlot = (uint8_t*)rfl64((uint64_t)arenaSlot);
  DevJob J;  // a wave-uniform copy of the staged descriptor's words
  for (uint32_t q = 0; q < sizeof(DevJob) / 4; ++q) ((uint32_t*)&J)[q] = rfl(((const uint32_t*)Jp)[q]);
  J.ctx_flags &= ~kCtxById;  // (the packer refuses path_ids with this flag; the path store is not passed in)
  DevResult res = {};
  Ctx c;
  fillCtx(c, J, P.maps, nullptr);
  if (!EPS) { c.nAgentsPad = 0; c.tPad = 0; }
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  stageConstraints(P.cons, J.vc_off, c.nVc, c.nEc, slot::consCopy(arenaSlot, P.arena_scratch_off, P.out_stride), c.vc, c.ec);
  {  // the focal table goes behind the window only where the 2 KiB heuristic table still fits behind it
    LaunchParams Pst = P;
    Pst.lds_paths_bytes = P.lds_paths_bytes >= 2048u ? P.lds_paths_bytes - 2048u : 0u;
    stageFocalTable<kTiersAll>(Pst, J, smem + ct::Narrow::windowBytes(false), slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride), c);
  }
  __syncthreads();
  const uint16_t* heur = (const uint16_t*)(P.maps + J.heur_off);
  const uint32_t heurStride = (c.dimx <= 32u && c.dimy <= 32u) ? 32u : c.dimx;
  const bool startInMap = c.sx < c.dimx && c.sy < c.dimy;
  const uint32_t h0 = startInMap ? rfl(heur[c.sy * heurStride + c.sx]) : 0u;
  int rc = ST_BAD;
  res.tier = 1;
  if (!startInMap) {
    rc = ST_BAD;  // (the host packer refuses such a job)
  } else if (h0 == 0xFFFFu) {
    rc = ST_NO_SOLUTION;  // the start cannot reach the goal at all: nothing to expand
  } else if (h0 > kFMax - 2u) {
    rc = ST_CAP_HORIZON;
  } else {
    SState s;
    res.tier = 0;
    // the narrow LDS tier first (maps up to 32 x 32, room for the table in the window's path area); a search that outgrows
    // it — open list, time steps, focalH, and here also h(start) or a successor's f beyond 124 — is run again by the arena tier
    if (!compactAttempt<EPS, false, kTiersAll, true>(P, J, smem, arenaSlot, c, res, outPath, s, rc, heur))
      rc = arenaAttempt<EPS, false, kTiersAll, true>(P, smem, arenaSlot, c, res, outPath, s, heur, heurStride);
    if (rc == RUN_MIGRATE_NODES) rc = ST_CAP_NODES;
    if (rc == RUN_MIGRATE_ROWS) rc = ST_CAP_HORIZON;
    res.expanded = s.expansions;
    res.nodes_created = s.nNodes;
  }
  out->status = rc; out->cost = res.cost; out->fmin = res.fmin; out->n_states = res.n_states;
  out->expanded = res.expanded; out->nodes_created = res.nodes_created; out->tier = res.tier;
  for (int q = 0; q < 8; ++q) out->prof[q] = res.prof[q];
}

// A search's path, `len` states at outPath, becomes visible: to the host at hostDst, then (f2) as cells in the device path
// store, where the jobs of the conflict-tree nodes that contain it will read it; visible to them because they are published
// after this job's completion was seen.  sidOf() names the slot and is asked between the two.  Agent-scope stores: through
// this XCD's L2 to memory, where the readers' agent-scope loads find them — no write-back of the whole L2 (residentLoop).
// A path that does not fit its slot (len >= path_store_stride; the packer cannot know the length beforehand) is NOT stored:
// the slot keeps its previous content, which a by-id reader would take for the path — callers keep their paths below
// max_horizon and treat a returned n_states >= max_horizon as not stored (mrp_ll.h).
template <class SidFn>
DEVI void publishPath(const LaunchParams& P, const uint16_t* outPath, uint32_t len, uint32_t* hostDst, SidFn sidOf) {
  const uint32_t lane = threadIdx.x;
  const uint32_t* src = (const uint32_t*)outPath;
  for (uint32_t i = lane; i < (len + 1u) / 2u; i += 64) hostStore32(hostDst + i, src[i]);
  const uint32_t sid = sidOf();
  if (sid < P.path_store_slots && len < P.path_store_stride) {
    uint16_t* slot = P.path_store + (size_t)sid * P.path_store_stride;
    for (uint32_t i = lane; i < len; i += 64) __hip_atomic_store(slot + 1 + i, outPath[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // x | y << 8
    __hip_atomic_store(slot, (uint16_t)len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the length word last
  }
}

// One job's bracket, shared by processJob and processSippJob: the descriptor out of host memory into the staging record in
// one coalesced read — HOSTLOADS: with system-scope loads; else with plain loads behind the resident loop's acquire fence —,
// the blank result, and at the end the result record back to host memory with lane-parallel stores.
template <bool HOSTLOADS>
DEVI void beginJob(const DevJob* jobSrc, DevJob& jobS, DevResult& res, uint32_t tier) {
  const uint32_t lane = threadIdx.x;
  const uint32_t* src = (const uint32_t*)jobSrc;
  __syncthreads();
  if (lane < sizeof(DevJob) / 4) ((uint32_t*)&jobS)[lane] = HOSTLOADS ? hostLoad32(src + lane) : src[lane];
  __syncthreads();
  res.status = ST_BAD; res.cost = 0; res.fmin = 0; res.n_states = 0; res.expanded = 0; res.nodes_created = 0;
  res.tier = tier;
  for (int q = 0; q < 8; ++q) res.prof[q] = 0;
}
DEVI void endJob(const DevResult& res, DevResult& resS, DevResult* resDst) {
  __syncthreads();
  resS = res;
  __syncthreads();
  if (threadIdx.x < sizeof(DevResult) / 4) hostStore32((uint32_t*)resDst + threadIdx.x, ((const uint32_t*)&resS)[threadIdx.x]);
}

// The root chain of one ECBS conflict tree (ecbs.hpp:118-136; ll_device.h kCtxChain): agent a is planned against the
// paths of the agents in front of it, the focal table [kChainRows][n_agents_pad] stays in the window between the
// searches and gains one column per path.  Everything runs in the compact tier; a search that outgrows it ends the chain
// in front of it.  Written for the A*-epsilon-only kernels (BG window).
// A launch whose window holds no table (lds_paths_bytes == 0: the front workgroups of mrp_ll_session_front_tables) keeps the
// chain's table in the path area of its arena slot instead, and the searches read it there (PLDS = false, CJob::pathsG).
// The rule that rests on is the one the compact tier's (time, cell) bitmap rests on (ll_compact.h, the successor probes): the
// table is written by THIS wave alone — the fill, the columns of the paths that exist, the column appended after each
// search, all plain stores — and read by this wave alone, with plain loads; a wave's vector-memory operations reach its
// CU's L1 in program order and that cache writes through, so a wave's later load of an address sees its own earlier store
// with no fence and no cache-wide action (the LLVM AMDGPU memory model asks for nothing between a store and a load of one
// thread in program order).  No other workgroup ever looks at the area, so no scope wider than the wave is involved; the one
// wait is the compiler's own, in front of the first use of a loaded value.
DEVI void runChain(const LaunchParams& P, const DevJob& J, uint8_t* smem, uint8_t* arenaSlot, DevResult& res,
                   uint16_t* outPath, uint16_t* hostOut) {
  constexpr bool BG = true;
  const uint32_t lane = threadIdx.x;
  const uint32_t n = J.n_ctx, first = J.t_pad, npad = J.n_agents_pad;
  const uint32_t end = J.reserved > first && J.reserved < n ? J.reserved : n;  // one past the last agent of this job
  res.tier = 0; res.n_states = 0; res.expanded = 0;
  if (P.lds_nodes == 0 || J.dimx > 32u || J.dimy > 32u || n > kChainMaxAgents || first >= n || npad < n || npad > 128u ||
      (npad & 1u) || kChainRows * npad * 2u > (P.lds_paths_bytes != 0u ? P.lds_paths_bytes : P.arena_paths_bytes) ||
      !compactFits<ct::Narrow>(P.arena_nodes, 0, BG) ||
      (uint64_t)n * kChainEntryWords * 2u + (uint64_t)n * 64u > (uint64_t)P.out_host_stride) {
    res.status = ST_BAD;  // (the host packer refuses such a job)
    return;
  }
  const uint32_t* who = P.cons + J.vc_off;   // starts / goals
  const uint32_t* ids = who + n;             // path-store slots
  const bool tabInLds = P.lds_paths_bytes != 0u;
  uint16_t* table = (uint16_t*)(tabInLds ? smem + ldsBytes(0, BG) : slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride));
  for (uint32_t i = lane; i < kChainRows * npad / 2u; i += 64) ((uint32_t*)table)[i] = 0xFFFFFFFFu;  // nobody anywhere
  __syncthreads();
  for (uint32_t a = 0; a < first; ++a) {  // the paths that exist already: lane = time step
    const uint32_t id = rfl(hostLoad32(ids + a));
    if (id >= P.path_store_slots) continue;
    const uint16_t* slot = P.path_store + (size_t)id * P.path_store_stride;
    uint32_t len = rfl(storeLoad(slot));
    if (len > P.path_store_stride - 1) len = P.path_store_stride - 1;
    if (len == 0) continue;
    table[lane * npad + a] = (uint16_t)storeLoad(slot + 1 + (lane < len ? lane : len - 1));
  }
  __syncthreads();
  int64_t budget = J.max_expansions;  // < 0: unlimited
  uint32_t* hostW = (uint32_t*)hostOut;
  uint32_t pathOff = n * kChainEntryWords;  // words
  uint32_t done = 0, maxLen = 0;
  bool allOk = true;
  int64_t total = 0;
  for (uint32_t a = first; a < end; ++a) {
    // (The bases of what a search's results are written through, made opaque once per search: the per-lane addresses behind
    // them are then built where they are used — two instructions — instead of being kept, which under the front kernel's
    // 128 VGPRs means spilled and reloaded, across the search.)
    asm volatile("" : "+s"(hostW), "+s"(outPath));
    const uint32_t sg = rfl(hostLoad32(who + a));
    ct::CJob cj = baseCJob(P, J, arenaSlot, outPath);
    cj.sx = sg & 0xFFu; cj.sy = (sg >> 8) & 0xFFu; cj.gx = (sg >> 16) & 0xFFu; cj.gy = sg >> 24;
    cj.lastGoal = -1;
    cj.nVc = 0; cj.nEc = 0;
    cj.nAgentsPad = npad; cj.tPad = kChainRows;
    cj.maxExp = clampMaxExp(budget);
    cj.vc = 0; cj.ec = 0;
    cj.pathsG = tabInLds ? 0ull : (uint64_t)table;
    __syncthreads();
    putCJob(smem, cj);
#ifndef MRP_LL_TRACE
    const uint64_t tl0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int32_t crc = tabInLds ? ct::compactSearch<true, true, BG>((wv::Lds)smem) : ct::compactSearch<true, false, BG>((wv::Lds)smem);
    const ct::CRes cr = getCRes(smem);
    const int32_t cost = cr.cost, fmin = cr.fmin, nStates = cr.nStates;
    const uint32_t expanded = cr.expanded;
#ifndef MRP_LL_TRACE
    res.prof[0] += (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);
    res.prof[1] += expanded;
#endif
    if (crc == ct::C_OVERFLOW) {
#ifndef MRP_LL_TRACE
      res.prof[6] += expanded;
      res.prof[7] += 1;
#endif
      allOk = false;
      break;  // not a search of this tier: the caller runs it as an ordinary job
    }
    {  // the agent's entry
      uint32_t v = 0;
      v = lane == 0 ? (uint32_t)crc : lane == 1 ? (uint32_t)cost : lane == 2 ? (uint32_t)fmin
          : lane == 3 ? (crc == ct::C_OK ? (uint32_t)nStates : 0u) : lane == 4 ? expanded : lane == 5 ? pathOff : 0u;
      if (lane < kChainEntryWords) hostStore32(hostW + (size_t)done * kChainEntryWords + lane, v);
    }
    done += 1;
    total += expanded;
    if (crc != ct::C_OK) {  // no path / expansion budget: the conflict tree ends with this answer
      allOk = false;
      break;
    }
    const uint32_t len = (uint32_t)nStates;
    maxLen = len > maxLen ? len : maxLen;
    {  // the path: to the host, to its path-store slot, into the table
      publishPath(P, outPath, len, hostW + pathOff, [&] { return rfl(hostLoad32(ids + a)); });
      pathOff += (len + 1u) / 2u;
      uint32_t rowLen = npad;  // (opaque likewise: lane * npad is computed here, not kept across the search)
      asm volatile("" : "+s"(rowLen));
      table[lane * rowLen + a] = outPath[lane < len ? lane : len - 1];
    }
    if (budget >= 0) budget = budget > (int64_t)expanded ? budget - (int64_t)expanded : 0;  // Instance::remainingLL()
  }
  __syncthreads();
  res.status = ST_OK;
  res.n_states = (int32_t)done;
  res.expanded = total;
  res.cost = -1;
  res.fmin = -1;
  // ---- the root node's conflicts (SURVEY.md §8 f1 on the drivers' path): when the chain has planned EVERY agent of the
  // instance, the table in the window is the root's whole solution, and this workgroup says at once whether the conflict
  // tree has anything to do — getFirstConflict (ecbs.cpp:401-452) and focalHeuristic (ecbs.cpp:315-350) over t = 0 ..
  // max_t - 1 (the final time step is never checked) and all pairs i < j:
  //   vertex conflict at t: state_i(t) == state_j(t);  edge conflict: state_i(t) == state_j(t+1) && state_i(t+1) == state_j(t)
  // Lane = time step (every path of this tier has at most 63 states); the first conflict is the smallest
  // (t, vertex before edge, i, j).  Seven instances in ten of the ten-agent workload end here: HL 1, no conflict.
  if (first == 0 && end == n && done == n && allOk && maxLen >= 1u && maxLen <= kChainRows) {
    const uint32_t T = maxLen - 1u;  // <= 62
    uint32_t cnt = 0, key = 0x7FFFFFFFu;  // this lane's conflicts, and its first one: t << 24 | edge << 16 | i << 8 | j
    // the pairs of time step t, whose row and the next one are tab[rowC ..] and tab[rowN ..] (inT: this lane has a time step)
    auto pairsOf = [&](const uint16_t* tab, uint32_t rowC, uint32_t rowN, uint32_t t, bool inT) {
      uint32_t bestV = 0xFFFFu, bestE = 0xFFFFu;  // the time step's first vertex / edge pair: i << 8 | j
      for (uint32_t i = 0; i + 1u < n; ++i) {
        const uint32_t ci = tab[rowC + i], ni = tab[rowN + i];
        for (uint32_t j = i + 1u; j < n; ++j) {
          const uint32_t cj = tab[rowC + j], nj = tab[rowN + j];
          const bool v = inT && ci == cj, e = inT && ci == nj && ni == cj;
          cnt += (v ? 1u : 0u) + (e ? 1u : 0u);
          if (v && bestV == 0xFFFFu) bestV = (i << 8) | j;
          if (e && bestE == 0xFFFFu) bestE = (i << 8) | j;
        }
      }
      const uint32_t k = bestV != 0xFFFFu ? (t << 24) | bestV : bestE != 0xFFFFu ? (t << 24) | (1u << 16) | bestE : 0x7FFFFFFFu;
      key = k < key ? k : key;
    };
    if (tabInLds) {
      pairsOf(table, lane * npad, (lane + 1u < kChainRows ? lane + 1u : kChainRows - 1u) * npad, lane, lane < T);
    } else {
      // The table is in device memory: its rows come into the window's open and focal areas — free after the last search,
      // 8 KB — with coalesced 4-byte loads, as many rows as fit, and a pass looks at the time steps whose row and next row it
      // holds: ONE pass up to 64 agents (64 rows of 128 bytes), two at 128 (rows 0 .. 31, then 31 .. 62).  A time step belongs
      // to one lane of one pass, so the count and the smallest key are what the single pass over a table in the window gives.
      uint16_t* stage = (uint16_t*)(smem + ct::oOpen);
      static_assert(2u * ct::kHeapBytes >= 32u * kChainMaxAgents * 2u, "room for 32 rows of the widest table");
      const uint32_t rowsFit = 2u * ct::kHeapBytes / (npad * 2u) < kChainRows ? 2u * ct::kHeapBytes / (npad * 2u) : kChainRows;  // >= 32
      for (uint32_t r0 = 0; r0 < T; r0 += rowsFit - 1u) {
        const uint32_t nRows = kChainRows - r0 < rowsFit ? kChainRows - r0 : rowsFit;  // rows r0 .. r0 + nRows - 1 (r0 < T <= 62: >= 2)
        __syncthreads();
        for (uint32_t i = lane; i < nRows * npad / 2u; i += 64) ((uint32_t*)stage)[i] = ((const uint32_t*)table)[r0 * npad / 2u + i];
        __syncthreads();
        const bool inT = lane + 1u < nRows && r0 + lane < T;
        const uint32_t row = inT ? lane : 0u;
        pairsOf(stage, row * npad, (row + 1u) * npad, r0 + lane, inT);
      }
    }
#pragma unroll
    for (uint32_t off = 32; off >= 1; off >>= 1) {
      cnt += (uint32_t)__shfl_xor((int)cnt, (int)off, 64);
      const uint32_t other = (uint32_t)__shfl_xor((int)key, (int)off, 64);
      key = other < key ? other : key;
    }
    res.cost = (int32_t)rfl(cnt);
    res.fmin = rfl(key) == 0x7FFFFFFFu ? -1 : (int32_t)rfl(key);
  }
}

}  // namespace mrp

#endif  // MRP_LL_JOBS_H
