// The CBS / ECBS search of the arena tier: AStar::search / AStarEpsilon::search over (time, cell) states with the whole
// state in the arena slot — ensureRows (the lazy (time, cell) bitmap), initSearch, runSearch.  Instantiated for TierHyb and
// TierHybXy by runJob (ll_jobs.h); ensureRows also serves the task-assignment searches (ll_ta.h).
// Needs ll_arena_heap.h.
#ifndef MRP_LL_ARENA_SEARCH_H
#define MRP_LL_ARENA_SEARCH_H

namespace mrp {

// ---- lazy bitmap rows: row t = obstacles | vertex constraints at time t | states already discovered --------
template <class T>
DEVI void ensureRows(Mem<T>& m, SState& s, const Ctx& c, uint32_t t1) {
  if (t1 < s.rowsReady) return;
  const uint32_t lane = threadIdx.x;
  uint32_t r0 = s.rowsReady;
  uint32_t r1 = t1 + 4;
  if (r1 > m.capRows) r1 = m.capRows;
  for (uint32_t r = r0; r < r1; ++r)
    for (uint32_t wd = lane; wd < c.wpr; wd += 64)
      m.bits[r * m.rowWords + wd] = c.obst[wd];
  __syncthreads();
  for (uint32_t j = lane; j < c.nVc; j += 64) {
    uint32_t v = c.vc[j];  // t << 16 | y << 8 | x
    uint32_t tt = v >> 16, cell = ((v >> 8) & 0xFFu) * c.dimx + (v & 0xFFu);
    if (tt >= r0 && tt < r1)
      __hip_atomic_fetch_or(m.bits + tt * m.rowWords + (cell >> 5), 1u << (cell & 31), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  s.rowsReady = r1;
}

// ---- one search in one tier ------------------------------------------------------------------------------------
// TH (MRP_LL_JOB_TABLE_H): admissibleHeuristic is a halfword of the shortest-path table `heur` (rows of heurStride halfwords)
// instead of the Manhattan distance; the caller has made sure that the start's value fits the entry's f field.
template <class T, bool EPS, bool TH = false>
DEVI void initSearch(Mem<T>& m, SState& s, const Ctx& c, const uint16_t* heur = nullptr, uint32_t heurStride = 0) {
  static_assert(T::AS == 1 && T::kWideNodes, "the arena tier: heaps, bitmap and four-word node records in global memory");
  uint32_t h0 = (c.sx > c.gx ? c.sx - c.gx : c.gx - c.sx) + (c.sy > c.gy ? c.sy - c.gy : c.gy - c.sy);
  if constexpr (TH) h0 = rfl(heur[c.sy * heurStride + c.sx]);
  s.nNodes = 1;
  s.nOpen = 1;
  s.nFocal = EPS ? 1 : 0;
  s.rowsReady = 0;
  s.bestF = (int32_t)h0;
  s.expansions = 0;
  u32x4 n0;
  n0.x = c.sx | (c.sy << 8) | (0u << 16) | (7u << 27);
  n0.y = kNoParent;
  n0.z = 0;
  n0.w = 0;
  ((typename Mem<T>::PNode4)m.nodes)[0] = n0;
  typename T::E e0 = T::pack(0, h0, 0, 0);
  if constexpr (T::kEntryXy) e0 = T::withXy(e0, c.sx | (c.sy << 8));
  m.open[0] = e0;
  if (EPS) m.focal[0] = e0;
}

// Returns a status (>= 0) when the search ended, or RUN_MIGRATE_NODES / _ROWS when the arena slot has no room for the next
// expansion's nodes / time step: runJob reports those as ST_CAP_NODES / ST_CAP_HORIZON.  (Nothing migrates any more; the
// two codes stay out of band because returning the statuses directly makes the compiler allocate registers differently in
// every kernel that hosts this search — a change for a pull request that measures it.)
// TH: a successor whose f = g + h does not fit the entry's field ends the search ST_CAP_HORIZON (the Manhattan h is bounded
// by the map and needs no test), as the task-assignment searches do (ll_ta.h TaEnv::fits).
enum : int { RUN_MIGRATE_NODES = -1, RUN_MIGRATE_ROWS = -2 };
template <class T, bool EPS, bool TH = false>
DEVI int runSearch(Mem<T>& m, SState& s, const Ctx& c, DevResult& res, uint16_t* outPath, const uint16_t* heur = nullptr,
                   uint32_t heurStride = 0) {
  static_assert(T::AS == 1 && T::kWideNodes, "the arena tier: heaps, bitmap and four-word node records in global memory");
  typedef typename T::E E;
  const uint32_t lane = threadIdx.x;
  uint32_t dbgIter = 0;
  // edge-constraint keys, one per lane (lists longer than a wave keep their tail in memory)
  const uint32_t ecReg = lane < c.nEc ? c.ec[lane] : 0xFFFFFFFFu;
  // successor of this lane in the reference's order Wait, Left, Right, Up, Down (ecbs.cpp:365-398) on lanes 0..4
  const int32_t dx = (lane == 2) - (lane == 1);
  const int32_t dy = (lane == 3) - (lane == 4);
  for (;;) {
    DBG(c, 5, ++dbgIter);
    PROF_MARK(profTop);
    if (s.nOpen == 0) return ST_NO_SOLUTION;
    const E topE = ldU<T>(m.open, 0);
    E curE = topE;
    if (EPS) {
      const int32_t oldBest = s.bestF;
      s.bestF = (int32_t)T::f(topE);
      if (s.bestF > oldBest) {
        PROF_T0();
        orderedWalk<T>(m, s, c, oldBest, res);
        PROF_ADD(res, 0);
        PROF_INC(res, 6, 1);
      }
      curE = ldU<T>(m.focal, 0);
    }
    // f, g (== time: every action costs 1) and focalH of the popped node are in its entry
    const uint32_t curId = T::id(curE);
    const uint32_t t = T::g(curE);
    const uint32_t curFh = T::fh(curE);
    uint32_t xy, curPos = 0;
    uint32_t curPosV = 0;  // kEntryXy: the open position as loaded (waited for only where popFocalEraseOpen needs it)
    if constexpr (T::kEntryXy) {
      xy = T::xyOf(curE);
      if (EPS) curPosV = m.nodes[curId * 4 + 3];
    } else {
      nodeXyPos<T>(m, curId, xy, curPos);
    }
    const uint32_t x = xy & 0xFF, y = xy >> 8;
    const bool isGoal = (x == c.gx) && (y == c.gy) && ((int32_t)t > c.lastGoal);
    DBG(c, 6, xy | (t << 16));
    DBG(c, 7, isGoal ? 1 : 2);
    if (!isGoal) {
      if (s.nNodes + 5 > m.capNodes || s.nOpen + 5 > m.capHeap) return RUN_MIGRATE_NODES;
      if (t + 1 >= m.capRows) return RUN_MIGRATE_ROWS;
    }
    // other agents' positions at t and t+1 (issued early; consumed after the heap pops)
    uint32_t a0 = kEmptyCell, b0 = kEmptyCell, a1 = kEmptyCell, b1 = kEmptyCell;
    const uint16_t* rowA = nullptr;
    const uint16_t* rowB = nullptr;
    if (EPS && c.nAgentsPad && !isGoal) {
      const uint32_t ra = t < c.tPad ? t : c.tPad - 1;
      const uint32_t rb = (t + 1) < c.tPad ? (t + 1) : c.tPad - 1;
      rowA = c.paths + (size_t)ra * c.nAgentsPad;
      rowB = c.paths + (size_t)rb * c.nAgentsPad;
      if (c.pathsLds) {  // the usual case: LDS reads proper, not flat loads through the LDS aperture
        if (lane < c.nAgentsPad) {  // rows are n_agents_pad (multiple of 16) entries long
          a0 = c.pathsLds[ra * c.nAgentsPad + lane];
          b0 = c.pathsLds[rb * c.nAgentsPad + lane];
        }
        if (64 + lane < c.nAgentsPad) {
          a1 = c.pathsLds[ra * c.nAgentsPad + 64 + lane];
          b1 = c.pathsLds[rb * c.nAgentsPad + 64 + lane];
        }
      } else {
        if (lane < c.nAgentsPad) {
          a0 = rowA[lane];
          b0 = rowB[lane];
        }
        if (64 + lane < c.nAgentsPad) {
          a1 = rowA[64 + lane];
          b1 = rowB[64 + lane];
        }
      }
    }

    s.expansions += 1;  // onExpandNode (a_star_epsilon.hpp:193 / a_star.hpp:87) — counts the goal pop too
    if (c.maxExp >= 0 && s.expansions > c.maxExp) return ST_CAP_EXP;

    if (isGoal) {
      res.cost = (int32_t)t;
      res.fmin = (int32_t)(EPS ? T::f(topE) : T::f(curE));
      res.n_states = (int32_t)t + 1;
      uint32_t nid = curId;
      for (int32_t k = (int32_t)t; k >= 0; --k) {  // follow cameFrom (a_star_epsilon.hpp:198-208)
        uint32_t pxy, par;
        nodeXyParent<T>(m, nid, pxy, par);
        outPath[k] = (uint16_t)pxy;  // all lanes, same address, same value
        nid = par;
      }
      DBG(c, 8, 77);
      return ST_OK;
    }

    const uint32_t t1 = t + 1;
    ensureRows<T>(m, s, c, t1);
    PROF_SINCE(res, 4, profTop);  // loop top -> pops, minus the ordered walk (slot 0)
    // the five successor probes: bounds, then ONE bit of the (time, cell) bitmap = obstacle | vertex constraint |
    // already discovered; the words are requested before the pops below so that their latency hides behind them
    const uint32_t nx = x + (uint32_t)dx, ny = y + (uint32_t)dy;
    const bool inb = (lane < 5) && (nx < c.dimx) && (ny < c.dimy);
    const uint32_t ncell = inb ? ny * c.dimx + nx : 0;
    const uint32_t curCell = y * c.dimx + x;
    const uint32_t bitIdx = t1 * m.rowWords + (ncell >> 5);
    const uint32_t word = m.bits[bitIdx];

    {
      PROF_T0();
      if (EPS) {
        if constexpr (T::kEntryXy) curPos = rfl(curPosV);
        popFocalEraseOpen<T>(m, s.nFocal, s.nOpen, curPos);
      } else {
        heapPop<T, 0, true>(m, m.open, s.nOpen);
      }
      PROF_ADD(res, 1);
    }
    const bool ok = inb && !((word >> (ncell & 31)) & 1u);
    uint32_t mask = (uint32_t)(ballot64(ok) & 0x1Full);
    if (c.nEc) {  // transitionValid (ecbs.cpp:505-510): lane j holds edge-constraint key j = t << 19 | cell << 3 | action
      const uint32_t base = (t << 19) | (curCell << 3);
      const uint32_t d = ecReg - base;
      if (ballot64(d < 5u)) {  // rare: some constraint names a move out of this very state
        uint32_t blocked = 0;
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) blocked |= ballot64(d == k) ? (1u << k) : 0u;
        mask &= ~blocked;
      }
      if (c.nEc > 64) {
        uint32_t blocked = 0;
        for (uint32_t j = 64; j < c.nEc; ++j) {  // lists longer than a wave: the rest one by one
          const uint32_t dd = rfl(c.ec[j]) - base;
          if (dd < 5) blocked |= 1u << dd;
        }
        mask &= ~blocked;
      }
    }
    if (mask == 0) continue;
    PROF_MARK(profEnt);

    // ---- the successors' entries, one per lane 0..4 (order-independent part: heuristics, node records, discovered marks)
    const bool mine = (lane < 5) && ((mask >> lane) & 1u);
    const uint32_t nBase = s.nNodes;
    const uint32_t nid = nBase + (uint32_t)__builtin_popcount(mask & ((1u << lane) - 1u));
    uint32_t h = (nx > c.gx ? nx - c.gx : c.gx - nx) + (ny > c.gy ? ny - c.gy : c.gy - ny);
    if constexpr (TH) h = mine ? heur[ny * heurStride + nx] : 0u;  // (a lane without a successor has no cell to look up)
    const uint32_t f = t1 + h;
    if constexpr (TH) {
      if (ballot64(mine && f > kFMax - 2u)) return ST_CAP_HORIZON;
    }
    uint32_t fh = curFh;
    if (EPS && c.nAgentsPad) {
      // focalStateHeuristic (ecbs.cpp:282-295) + focalTransitionHeuristic (ecbs.cpp:298-312): lanes hold the other
      // agents' cells at t (a) and t+1 (b); an agent counts once if it stands on the successor's cell at t+1 and once
      // more if it swaps places with this agent
      // (the path table holds the other agents' cells as x | y << 8)
      const uint32_t nxyL = nx | (ny << 8);
      const uint64_t swap0 = ballot64(b0 == xy);
      const uint64_t swap1 = c.nAgentsPad > 64 ? ballot64(b1 == xy) : 0ull;
      for (uint32_t mm = mask; mm; mm &= mm - 1) {
        const uint32_t k = (uint32_t)__builtin_ctz(mm);
        const uint32_t cc = __builtin_amdgcn_readlane(nxyL, k);
        uint32_t cnt = (uint32_t)__popcll(ballot64(b0 == cc)) + (uint32_t)__popcll(ballot64(a0 == cc) & swap0);
        if (c.nAgentsPad > 64) {
          cnt += (uint32_t)__popcll(ballot64(b1 == cc)) + (uint32_t)__popcll(ballot64(a1 == cc) & swap1);
          for (uint32_t base = 128; base < c.nAgentsPad; base += 64) {
            uint32_t av = kEmptyCell, bv = kEmptyCell;
            if (base + lane < c.nAgentsPad) {
              av = rowA[base + lane];
              bv = rowB[base + lane];
            }
            cnt += (uint32_t)__popcll(ballot64(bv == cc)) + (uint32_t)__popcll(ballot64(av == cc && bv == xy));
          }
        }
        fh = lane == k ? curFh + cnt : fh;
      }
      if (ballot64(mine && fh > T::kFhCap)) return ST_CAP_FOCAL;
    }
    E eMine = T::pack(fh, f, t1, nid);
    if constexpr (T::kEntryXy) eMine = T::withXy(eMine, nx | (ny << 8));
    const float bound = __fmul_rn((float)s.bestF, c.w);  // a_star_epsilon.hpp:240, binary32
    const uint32_t maskF = EPS ? (uint32_t)(ballot64(mine && (float)(int32_t)f <= bound) & 0x1Full) : 0u;
    if (mine) {
      u32x4 nn;
      nn.x = nx | (ny << 8) | (t1 << 16) | (lane << 27);
      nn.y = curId;
      nn.z = fh;
      nn.w = 0;
      ((typename Mem<T>::PNode4)m.nodes)[nid] = nn;
    }
    {
      // mark (t1, cell) discovered: stands for stateToHeap / closedSet membership (a_star_epsilon.hpp:224-227); the
      // successors of one expansion are distinct cells, so marking them together changes nothing.  A plain store of the
      // merged word instead of a memory-side atomic per successor (successors that share a bitmap word all store the same
      // merged word)
      const uint32_t myBit = mine ? 1u << (ncell & 31) : 0u;
      uint32_t merged = word;
#pragma unroll
      for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t oi = __builtin_amdgcn_readlane(bitIdx, k);
        const uint32_t ob = __builtin_amdgcn_readlane(myBit, k);
        merged |= oi == bitIdx ? ob : 0u;
      }
      if (mine) m.bits[bitIdx] = merged;
    }
    s.nNodes = nBase + (uint32_t)__builtin_popcount(mask);
    E e[5];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) e[k] = T::fromLane(eMine, k);
    PROF_SINCE(res, 3, profEnt);  // successors' entries: heuristics, node records, discovered marks
    // ---- pushes: openSet.push for every successor, focalSet.push for those within the bound, in successor order
    {
      PROF_T0();
      PushChains<T> po, pf;
      po.load(m.open, s.nOpen, mask);
      if (EPS) pf.load(m.focal, s.nFocal, maskF);
      po.template resolve<0, true>(m, m.open, s.nOpen, mask, e);
      s.nOpen += (uint32_t)__builtin_popcount(mask);
      if (EPS) {
        pf.template resolve<1, false>(m, m.focal, s.nFocal, maskF, e);
        s.nFocal += (uint32_t)__builtin_popcount(maskF);
      }
      PROF_ADD(res, 2);
    }
  }
}

}  // namespace mrp

#endif  // MRP_LL_ARENA_SEARCH_H
