// The task-assignment low levels: TaEnv (the Environment of cbs_ta / ecbs_ta on the arena's records), runTaArena and
// runJobTA (MRP_LL_ASTAR_TA: compact tier, then arena), orderedWalkTaEps and runJobTaEps (MRP_LL_ASTAR_EPS_TA) and, in front
// of it for a job that asks (MRP_LL_JOB_TRY_LDS), runTaEpsLds.
// Needs ll_arena_heap.h (heaps, Mem), ll_arena_search.h (ensureRows), ll_jobs.h (staging, cutArena, cutHeaps) and
// ll_compact_ta_eps.h.
#ifndef MRP_LL_TA_H
#define MRP_LL_TA_H

namespace mrp {

// ---- the Environment of the task-assignment searches (example/cbs_ta.cpp:283-372 == example/ecbs_ta.cpp:283-445) -----
// What runTaArena (AStar) and runJobTaEps (AStarEpsilon) share: optional task, shortest-path heuristic from the uploaded
// table, a Wait at the goal is free, so a state can be reached again with a smaller g.  On the arena's records:
//   node   {x | y << 8 | t << 16 | action << 27, parent, g, position of its entry in the open array}
//   status one word per (t, cell): 0 unseen, node + 1 in the open list, bit 31 closed (stateToHeap + closedSet,
//          a_star.hpp:116-117); rows are zeroed as the search reaches them
//   bits   (time, cell) bitmap: obstacles | vertex constraints (stateValid, cbs_ta.cpp:483-489), rows made on demand
// Wave-uniform but for ecReg, dx, dy (one value per lane).
struct TaProbe {  // lanes 0..4: the successor by Wait, Left, Right, Up, Down
  uint32_t nxy, ncell, h, st;  // x | y << 8, cell index, heuristic, status word
};
struct TaEnv {
  typedef TierHbm T;
  uint32_t dimx, dimy, cells, gx, gy;
  bool noGoal;
  const uint16_t* heur;  // the task's shortest-path table, rows of heurStride halfwords
  uint32_t heurStride;
  uint32_t* status;
  uint32_t rows, statusReady;  // time steps the table has room for / that have been zeroed
  const uint32_t* ec;
  uint32_t nEc, ecReg;  // ecReg: this lane's word of the first 64 edge constraints
  int32_t dx, dy;

  DEVI void init(const Ctx& c, bool noGoal_, const uint16_t* heur_, uint32_t heurStride_, uint32_t* status_, uint32_t rows_) {
    const uint32_t lane = threadIdx.x;
    dimx = c.dimx; dimy = c.dimy; cells = c.dimx * c.dimy; gx = c.gx; gy = c.gy;
    noGoal = noGoal_; heur = heur_; heurStride = heurStride_;
    status = status_; rows = rows_; statusReady = 0;
    ec = c.ec; nEc = c.nEc;
    ecReg = lane < nEc ? ec[lane] : 0xFFFFFFFFu;
    dx = (lane == 2) - (lane == 1);
    dy = (lane == 3) - (lane == 4);
  }
  // false: the task cannot be reached from the start (the reference's table says INT_MAX), or not within f's field
  DEVI bool startH(uint32_t sx, uint32_t sy, uint32_t& h0) const {
    h0 = noGoal ? 0u : heur[sy * heurStride + sx];
    return h0 <= kFMax - 2u;
  }
  DEVI bool atGoal(uint32_t x, uint32_t y) const { return noGoal || (x == gx && y == gy); }
  DEVI void zeroRows(uint32_t t1) {  // the status rows up to time step t1: nothing seen
    while (statusReady <= t1) {
      for (uint32_t i = threadIdx.x; i < cells; i += 64) status[statusReady * cells + i] = 0;
      statusReady += 1;
    }
  }
  DEVI void close(uint32_t x, uint32_t y, uint32_t t) { status[t * cells + y * dimx + x] = 0x80000000u; }
  // getNeighbors (cbs_ta.cpp:321-367, ecbs_ta.cpp:392-438): Wait, Left, Right, Up, Down on lanes 0..4 — bounds, obstacle |
  // vertex constraint (one bit of the bitmap), edge constraints by key (transitionValid, cbs_ta.cpp:491-496).  Returns the
  // 5-bit mask of the valid successors of (x, y, t).
  DEVI uint32_t probe(const Mem<T>& g, uint32_t x, uint32_t y, uint32_t t, TaProbe& p) const {
    const uint32_t lane = threadIdx.x;
    const uint32_t t1 = t + 1u;
    const uint32_t nx = x + (uint32_t)dx, ny = y + (uint32_t)dy;
    const bool inb = (lane < 5) && (nx < dimx) && (ny < dimy);
    p.ncell = inb ? ny * dimx + nx : 0;
    const uint32_t word = g.bits[t1 * g.rowWords + (p.ncell >> 5)];
    p.h = (noGoal || !inb) ? 0u : heur[ny * heurStride + nx];
    p.st = inb ? status[t1 * cells + p.ncell] : 0u;
    p.nxy = nx | (ny << 8);
    uint32_t mask = (uint32_t)(ballot64(inb && !((word >> (p.ncell & 31)) & 1u)) & 0x1Full);
    if (nEc) {
      const uint32_t base = (t << 19) | ((y * dimx + x) << 3);
      uint32_t blocked = 0;
      for (uint32_t j0 = 0; j0 < nEc; j0 += 64) {
        const uint32_t d = (j0 == 0 ? ecReg : (j0 + lane < nEc ? ec[j0 + lane] : 0xFFFFFFFFu)) - base;
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) blocked |= ballot64(d == k) ? (1u << k) : 0u;
      }
      mask &= ~blocked;
    }
    return mask;
  }
  // a new node's h, f = g + h and g fit the heap entry's fields
  DEVI static bool fits(uint32_t h, uint32_t g2) { return !(h > kFMax || g2 + h > kFMax - 2u || g2 > kGMask); }
  DEVI void newNode(Mem<T>& g, uint32_t nid, uint32_t xy, uint32_t t, uint32_t action, uint32_t parent, uint32_t g2,
                    uint32_t cell) {
    u32x4 nn;
    nn.x = xy | (t << 16) | (action << 27);
    nn.y = parent;
    nn.z = g2;
    nn.w = 0;
    ((Mem<T>::PNode4)g.nodes)[nid] = nn;
    status[t * cells + cell] = nid + 1u;
  }
  // A node that is still in the open list, reached again by `action` from `parent` with g2 (a_star.hpp:130-152,
  // a_star_epsilon.hpp:248-279).  False: not an improvement.  Otherwise cameFrom and g are replaced and the caller gets
  // what it needs to re-key the open entry: its position, its f so far and fNew = f - (gOld - g2).
  DEVI static bool rekey(Mem<T>& g, uint32_t nid, uint32_t action, uint32_t parent, uint32_t g2, uint32_t& gOld,
                         uint32_t& posOld, uint32_t& fOld, uint32_t& fNew) {
    const u32x4 on = ((Mem<T>::PNode4)g.nodes)[nid];
    gOld = rfl(on.z);
    posOld = rfl(on.w);
    if (g2 >= gOld) return false;
    fOld = T::f(ldU<T>(g.open, posOld));
    fNew = fOld - (gOld - g2);
    g.nodes[nid * 4 + 0] = (rfl(on.x) & 0x07FFFFFFu) | (action << 27);
    g.nodes[nid * 4 + 1] = parent;
    g.nodes[nid * 4 + 2] = g2;
    return true;
  }
  // the solution's states, goal first, along the parents (all lanes, same address, same value)
  DEVI static void walkPath(Mem<T>& g, uint32_t nid, uint32_t t, uint16_t* outPath) {
    for (int32_t k = (int32_t)t; k >= 0; --k) {
      const u32x4 pn = ((Mem<T>::PNode4)g.nodes)[nid];
      outPath[k] = (uint16_t)(rfl(pn.x) & 0xFFFFu);
      nid = rfl(pn.y);
    }
  }
};

// MRP_LL_ASTAR_TA in the arena tier: AStar::search (a_star.hpp:63-161) over TaEnv for the searches the compact tier cannot
// hold (more than 1023 open nodes, t > 61, f > 254, more than 64 + 64 constraints, maps beyond 32 x 32).  Same rules as
// ct::compactSearchTA; `openSet.increase(handle)` (a_star.hpp:139-145) is live.
//   entry  TierHbm: key = (f asc, g desc), low word = node id
//   status in the (unused) focal + walk-queue areas of the slot
// Time steps: as many as the status table has room for (and the job's horizon); beyond: MRP_LL_CAP_HORIZON.
DEVI void runTaArena(const LaunchParams& P, const DevJob& J, uint8_t* arenaSlot, DevResult& res, uint16_t* outPath,
                     const uint32_t* vc, const uint32_t* ec, const uint16_t* heur, uint32_t heurStride) {
  typedef TierHbm T;
  Mem<T> g = cutArena(P, arenaSlot);
  uint32_t* status = (uint32_t*)((uint8_t*)g.focal - 8);  // (the status table lives from here on)
  g.aux = g.focal;
  const uint64_t statusWords = slot::heapBytes(P.arena_nodes) * 2 / 4;
  Ctx c;
  fillCtx(c, J, P.maps, P.debug);
  c.w = 1.0f;
  c.vc = vc; c.ec = ec;
  c.paths = nullptr; c.pathsLds = nullptr;
  c.nAgentsPad = 0; c.tPad = 0;
  const uint32_t cells = c.dimx * c.dimy;
  const uint32_t rows = (uint32_t)(statusWords / cells < P.arena_rows ? statusWords / cells : P.arena_rows);
  res.tier = 1;
  res.status = ST_NO_SOLUTION;
  if (rows < 2u) {
    res.status = ST_CAP_HORIZON;
    return;
  }
  TaEnv env;
  env.init(c, (J.ctx_flags & kTaNoGoal) != 0, heur, heurStride, status, rows);
  SState s;
  s.nNodes = 1; s.nOpen = 1; s.nFocal = 0; s.rowsReady = 0; s.bestF = 0; s.expansions = 0;
  {
    uint32_t h0;
    if (!env.startH(c.sx, c.sy, h0)) {
      res.status = ST_CAP_HORIZON;
      return;
    }
    g.open[0] = T::pack(0, h0, 0, 0);
    env.zeroRows(0);
    __syncthreads();
    env.newNode(g, 0, c.sx | (c.sy << 8), 0, 7u, kNoParent, 0, c.sy * c.dimx + c.sx);  // node 0, in the open list
  }
  for (;;) {
    if (s.nOpen == 0) {
      res.status = ST_NO_SOLUTION;
      break;
    }
    const T::E curE = ldU<T>(g.open, 0);
    const uint32_t curId = T::id(curE), gcur = T::g(curE), fcur = T::f(curE);
    const u32x4 nd = ((Mem<T>::PNode4)g.nodes)[curId];
    const uint32_t xyt = rfl(nd.x);
    const uint32_t x = xyt & 0xFFu, y = (xyt >> 8) & 0xFFu, t = (xyt >> 16) & 0x7FFu;
    const bool atGoal = env.atGoal(x, y);
    s.expansions += 1;  // onExpandNode (a_star.hpp:87)
    if (c.maxExp >= 0 && s.expansions > c.maxExp) {
      res.status = ST_CAP_EXP;
      break;
    }
    if (atGoal && (int32_t)t > c.lastGoal) {  // isSolution (cbs_ta.cpp:313-319) -> a_star.hpp:89-106
      if (t + 1u > P.out_stride) {
        res.status = ST_CAP_HORIZON;
        break;
      }
      TaEnv::walkPath(g, curId, t, outPath);
      res.status = ST_OK;
      res.cost = (int32_t)gcur;
      res.fmin = (int32_t)fcur;
      res.n_states = (int32_t)t + 1;
      break;
    }
    const uint32_t t1 = t + 1u;
    if (t1 >= env.rows || t1 >= g.capRows) {
      res.status = ST_CAP_HORIZON;
      break;
    }
    if (s.nNodes + 5u > g.capNodes || s.nOpen + 5u > g.capHeap) {
      res.status = ST_CAP_NODES;
      break;
    }
    heapPop<T, 0, true>(g, g.open, s.nOpen);  // openSet.pop() (a_star.hpp:109)
    env.close(x, y, t);                       // closedSet.insert (a_star.hpp:110)
    ensureRows<T>(g, s, c, t1);
    env.zeroRows(t1);
    __syncthreads();
    TaProbe pr;
    const uint32_t mask = env.probe(g, x, y, t, pr);
    bool fail = false;
    for (uint32_t mm = mask; mm && !fail; mm &= mm - 1) {  // the new / rediscovered / closed cases of a_star.hpp:116-153, in order
      const uint32_t k = (uint32_t)__builtin_ctz(mm);
      const uint32_t st = __builtin_amdgcn_readlane(pr.st, k);
      if (st & 0x80000000u) continue;  // closed
      const uint32_t g2 = gcur + ((k == 0 && atGoal) ? 0u : 1u);  // tentative_gScore (a_star.hpp:118)
      if (st == 0) {  // not in the open list, not closed: a new node (a_star.hpp:120-129)
        const uint32_t h = __builtin_amdgcn_readlane(pr.h, k);
        if (!TaEnv::fits(h, g2)) {
          res.status = ST_CAP_HORIZON;
          fail = true;
          break;
        }
        const uint32_t nid = s.nNodes++;
        env.newNode(g, nid, __builtin_amdgcn_readlane(pr.nxy, k), t1, k, curId, g2, __builtin_amdgcn_readlane(pr.ncell, k));
        siftUp<T, 0, true>(g, g.open, s.nOpen, T::pack(0, g2 + h, g2, nid));
        s.nOpen += 1;
      } else {        // still in the open list (a_star.hpp:130-146)
        const uint32_t nid = st - 1u;
        uint32_t gOld, posOld, fOld, fNew;
        if (!TaEnv::rekey(g, nid, k, curId, g2, gOld, posOld, fOld, fNew)) continue;  // (a_star.hpp:135-137)
        siftUp<T, 0, true>(g, g.open, posOld, T::pack(0, fNew, g2, nid));  // increase(handle)
      }
    }
    if (fail) break;
  }
  res.expanded = s.expansions;
  res.nodes_created = s.nNodes;
}

// MRP_LL_ASTAR_TA: the low level of the task-assignment callers: the compact tier (ll_compact.h
// compactSearchTA) when the job fits it — a map up to 32 x 32, at most 64 vertex and 64 edge constraints — and the arena
// tier above when it does not, or when the search outgrows the compact tier on the way (its capacity statuses are then
// not an answer).  The goal's shortest-path table sits in the maps buffer (mrp_ll_upload_heuristic): [32][32] halfwords
// for maps up to 32 x 32, [dimy][dimx] beyond.
DEVI void runJobTA(const LaunchParams& P, const DevJob& J, uint8_t* smem, uint8_t* arenaSlot, DevResult& res, uint16_t* outPath) {
  res.tier = 0;
  const uint32_t* vc;
  const uint32_t* ec;
  stageConstraints(P.cons, J.vc_off, J.n_vc, J.n_ec, slot::consCopy(arenaSlot, P.arena_scratch_off, P.out_stride), vc, ec);
  __syncthreads();
  const bool small = J.dimx <= 32u && J.dimy <= 32u;
  const uint16_t* heur = (const uint16_t*)(P.maps + J.path_off);
  const bool compactOk = P.lds_nodes != 0 && P.lds_paths_bytes >= 2048u && small && J.n_vc <= 64u && J.n_ec <= 64u &&
                         compactFits<ct::Narrow>(P.arena_nodes, 0, false);
  if (compactOk) {
    ct::CJob cj = baseCJob(P, J, arenaSlot, outPath);
    cj.sx = J.sx; cj.sy = J.sy; cj.gx = J.gx; cj.gy = J.gy;
    cj.lastGoal = J.last_goal_constraint;
    cj.w = 1.0f;
    cj.nVc = J.n_vc; cj.nEc = J.n_ec;
    cj.nAgentsPad = 0; cj.tPad = 0;
    cj.taNoGoal = (J.ctx_flags & kTaNoGoal) ? 1u : 0u;
    cj.vc = (uint64_t)vc; cj.ec = (uint64_t)ec;
    cj.pathsG = (uint64_t)heur;
    putCJob(smem, cj);
    const uint64_t tl0 = __builtin_amdgcn_s_memrealtime();
    const int32_t crc = ct::compactSearchTA((wv::Lds)smem);
    const ct::CRes cr = getCRes(smem);
    res.prof[0] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);
    res.prof[1] = cr.expanded;
    if (crc != ct::C_CAP_NODES && crc != ct::C_CAP_HORIZON) {  // an answer (C_OK / C_NO_SOLUTION / C_CAP_EXP == the ST_ codes)
      res.status = crc; res.cost = cr.cost; res.fmin = cr.fmin; res.n_states = cr.nStates;
      res.expanded = cr.expanded; res.nodes_created = cr.nodes;
      return;
    }
    res.prof[6] = cr.expanded;  // expansions thrown away with the attempt
    res.prof[7] = 1;
    __syncthreads();
  }
  const uint64_t th0 = __builtin_amdgcn_s_memrealtime();
  runTaArena(P, J, arenaSlot, res, outPath, vc, ec, heur, small ? 32u : J.dimx);
  res.prof[2] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - th0);
  res.prof[3] = (uint32_t)res.expanded;
}

// ---- MRP_LL_ASTAR_EPS_TA: the low level of ECBS with task assignment ---------------------------------------------------
// AStarEpsilon::search (a_star_epsilon.hpp:86-285) over the Environment of example/ecbs_ta.cpp:283-445 — what
// ecbs_ta.hpp:498-499 instantiates.  The Environment is TaEnv, shared with runTaArena (optional task, shortest-path
// heuristic from the uploaded table, a Wait at the goal is free), the focal heuristics are example/ecbs.cpp's, taken at the successor's TIME
// (ecbs_ta.cpp:314-344).  Because g != time a state can be discovered again with a smaller g, and this is the one search of
// the reference in which a_star_epsilon.hpp:249-269 is live: g and f drop, `openSet.increase(handle)` sifts the open entry
// up, focalH keeps its value, and a node that already sits in the focal list is NOT moved there — the reference's focal
// heap compares through handles, so the entry simply reads the new f and g where it lies.  Replayed verbatim: the focal
// entry's key is rewritten at its position (TierFocalPos keeps handle -> focal position) and nothing is sifted; every later
// focal operation then sees the same (possibly out-of-order) array the reference's heap sees.
//
// The arena slot's node + heap area (ll_slot.h areaBytes: arena_nodes * 40 + 48 bytes; the (time, cell) bitmap behind it stays
// where it is) is cut differently from the other searches, because this one needs the status table AND both heaps:
//   status   one word per (t, cell): 0 unseen, node + 1 in the open list, bit 31 closed; rows = min(arena_rows,
//            area / 8 / cells) time steps (at most half of the area)
//   then, for capN = (area - status - 64) / 48 nodes:
//   node A   {x | y << 8 | t << 16 | action << 27, parent, g, position in the open array}
//   node B   {focalH, position in the focal array (kNoPos: not there)}
//   open, focal, walk queue: capN 64-bit entries each (TierHbm keys)
// Beyond those: MRP_LL_CAP_HORIZON / MRP_LL_CAP_NODES; focalH beyond its key field: MRP_LL_CAP_FOCAL.
template <class T>
DEVI void eraseOpen(Mem<T>& m, uint32_t& nOpen, uint32_t curPos) {  // boost erase: bubble to the root, then pop
  typedef typename T::E E;
  const uint32_t lane = threadIdx.x;
  const uint32_t nOld = nOpen;
  nOpen -= 1;
  E lastOv = 0;
  if (nOpen > 0) lastOv = m.open[nOld - 1];
  const uint32_t depth = 31u - (uint32_t)__builtin_clz(curPos + 1);
  const bool act = lane < depth;
  const uint32_t anc = act ? ((curPos + 1) >> (lane + 1)) - 1 : 0;
  E ae = 0;
  if (depth != 0) ae = m.open[anc];
  if (act) {  // every ancestor of curPos moves down one level
    const uint32_t dest = ((curPos + 1) >> lane) - 1;
    m.open[dest] = ae;
    setPos<T>(m, T::id(ae), dest);
  }
  // the element pop() moves to the root: the last one — which the shift has just overwritten if the erased node WAS the
  // last one (then it is the erased node's parent)
  E lastO = T::first(lastOv);
  if (curPos == nOld - 1 && depth != 0) lastO = T::fromLane(ae, 0);
  if (nOpen > 0) descend<T, 0, true, false>(m, m.open, nOpen, 0, lastO);
}

// orderedWalk (above) with the focal pushes recorded in the nodes' B records.  Returns false if the focal array is full
// (cannot happen while every open node sits in it at most once; checked because the array must never be overrun).
DEVI bool orderedWalkTaEps(Mem<TierHbm>& m, Mem<TierFocalPos>& mf, SState& s, float w, int32_t oldBest) {
  typedef TierHbm T;
  typedef T::E E;
  const float lo = __fmul_rn((float)oldBest, w);  // a_star_epsilon.hpp:145,149: int * float in binary32
  const float hi = __fmul_rn((float)s.bestF, w);
  uint32_t npq = 0;
  E curA = T::aux(T::keyOpen(ldU<T>(m.open, 0)), 0);
  for (;;) {
    const uint32_t cur = T::auxIdx(curA);
    const uint32_t first = 2 * cur + 1;
    if (first < s.nOpen) {
      E e1, e2;
      ldPair<T>(m.open, first, e1, e2);
      E ee[5];
      ee[0] = T::aux(T::keyOpen(e1), first);
      ee[1] = T::aux(T::keyOpen(e2), first + 1);
      ee[2] = ee[3] = ee[4] = 0;
      const uint32_t pm = first + 1 < s.nOpen ? 3u : 1u;
      PushChains<T> pc;
      pc.load(m.aux, npq, pm);
      pc.template resolve<2, false>(m, m.aux, npq, pm, ee);
      npq += pm == 3u ? 2u : 1u;
    }
    const float fv = (float)(int32_t)T::f(curA);
    if (fv > lo && fv <= hi) {
      if (s.nFocal + 1u >= mf.capHeap) return false;
      const E e = ldU<T>(m.open, cur);
      siftUp<TierFocalPos, 1, true>(mf, mf.focal, s.nFocal, e);
      s.nFocal += 1;
    }
    if (fv > hi) break;
    if (npq == 0) break;
    curA = auxPop<T>(m, npq);
  }
  return true;
}

// A real function (its own register allocation): the kernels that host it keep theirs.  The job is read where the kernel
// staged it, the result goes to `out` (status, cost, fmin, n_states, expanded, nodes_created, tier).
// IN_PLACE (ll_ta_root.h, ECBS-TA): the focal table [t_pad][n_agents_pad] already lies in the slot's path area — where the
// ordinary job copies its shipped one — and is taken as it is; nothing is copied, path_off is not looked at.  The ordinary
// job is the IN_PLACE = false instance, which knows two more sources: a table shipped by the host (paths[path_off]), or —
// kCtxById — the conflict-tree node's paths named by their path-store slots (n_ctx ids at cons[path_off]): the workgroup
// builds the table in the slot's path area with ll_jobs.h buildIdTableInArena, the build runJob uses for a table in the
// arena.  A by-id table that does not fit the path area, or names more agents than its rows are wide, is ST_BAD with nothing
// written (the host packer refuses such a job).  pathStore / storeStride / storeSlots: LaunchParams' path store.
template <bool IN_PLACE>
__device__ __attribute__((noinline)) void runJobTaEps(const DevJob* Jp, DevResult* out, uint8_t* arenaSlot, const uint32_t* maps,
                                                      const uint32_t* consHost, const uint16_t* pathsHost,
                                                      uint32_t scratchOff, uint32_t outStride, uint32_t arenaNodes,
                                                      uint32_t arenaRows, uint32_t arenaRowWords, uint32_t arenaPathsBytes,
                                                      const uint16_t* pathStore, uint32_t storeStride, uint32_t storeSlots) {
  typedef TierHbm T;
  typedef TierFocalPos TF;
  typedef T::E E;
  const uint32_t lane = threadIdx.x;
  // (arguments arrive in vector registers: with these two wave-uniform, so are rows, capN and `run` below, and TaEnv's
  // row counter stays scalar)
  arenaNodes = rfl(arenaNodes); arenaRows = rfl(arenaRows);
  Ctx c;
  fillCtx<true>(c, *Jp, maps, nullptr);
  c.pathsLds = nullptr;
  const uint32_t dimx = c.dimx, cells = dimx * c.dimy, tPad = c.tPad;
  const float w = c.w;
  const bool small = dimx <= 32u && c.dimy <= 32u;

  int32_t status = ST_NO_SOLUTION, cost = 0, fmin = 0, nStates = 0;
  SState s;
  s.nNodes = 0; s.nOpen = 0; s.nFocal = 0; s.rowsReady = 0; s.bestF = 0; s.expansions = 0;

  // ---- the job's constraint words and focal path table leave host memory in one pass
  uint16_t* outPath = slot::outPath(arenaSlot, scratchOff, outStride);
  uint32_t* consLocal = slot::consCopy(arenaSlot, scratchOff, outStride);
  uint8_t* pathsArena = slot::pathsCopy(arenaSlot, scratchOff, outStride);
  stageConstraints(consHost, rfl(Jp->vc_off), c.nVc, c.nEc, consLocal, c.vc, c.ec);
  bool tableOk = true;
  {
    const uint32_t pathOff = rfl(Jp->path_off);
    const uint32_t pathBytes = tPad * c.nAgentsPad * 2;  // multiple of 32
    if (pathBytes == 0) {
      c.paths = nullptr;
      c.nAgentsPad = 0;
    } else if constexpr (IN_PLACE) {
      c.paths = (const uint16_t*)pathsArena;  // (its writer made sure that it fits)
    } else if (rfl(Jp->ctx_flags) & kCtxById) {
      // (the store's arguments arrive in vector registers too: wave-uniform, so are the build's loop bounds and slot bases)
      const uint32_t nCtx = rfl(Jp->n_ctx);
      if (pathBytes > rfl(arenaPathsBytes) || nCtx > c.nAgentsPad) {  // never write past the path area
        tableOk = false;
        c.paths = nullptr;
        c.nAgentsPad = 0;
      } else {
        buildIdTableInArena((uint16_t*)pathsArena, consHost + pathOff, nCtx, tPad, c.nAgentsPad,
                            (const uint16_t*)rfl64((uint64_t)pathStore), rfl(storeStride), rfl(storeSlots));
        c.paths = (const uint16_t*)pathsArena;
      }
    } else if (pathBytes <= arenaPathsBytes) {
      const uint32_t* psrc = (const uint32_t*)(pathsHost + pathOff);
      uint32_t* dst = (uint32_t*)pathsArena;
      for (uint32_t i = lane; i < pathBytes / 4; i += 64) dst[i] = hostLoad32(psrc + i);
      c.paths = (const uint16_t*)pathsArena;
    } else {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      c.paths = pathsHost + pathOff;
    }
  }
  __syncthreads();

  // ---- this search's cut of the slot
  const uint64_t area = slot::areaBytes(arenaNodes);
  const uint64_t rows64 = area / 8 / cells;
  const uint32_t rows = (uint32_t)(rows64 < arenaRows ? rows64 : arenaRows);
  const uint64_t statusBytes = ((uint64_t)rows * cells * 4 + 15) & ~15ull;
  uint64_t capN64 = area > statusBytes + 64 ? (area - statusBytes - 64) / 48 : 0;
  if (capN64 > kMaxArenaNodes) capN64 = kMaxArenaNodes;
  const uint32_t capN = (uint32_t)capN64 & ~1u;
  Mem<T> g = {};
  uint8_t* const recA = arenaSlot + statusBytes;
  uint8_t* const recB = recA + (size_t)capN * 16;
  g.nodes = (Mem<T>::PN32)recA;
  cutHeaps(g, recB + (size_t)capN * 8, capN);
  g.bits = (Mem<T>::P32)(arenaSlot + area);
  g.capRows = arenaRows; g.rowWords = arenaRowWords;
  Mem<TF> gf = viewAs<TF>(g);  // the same heaps; its node records are the B records
  gf.nodes = (Mem<TF>::PN32)recB;
  typedef __attribute__((address_space(1))) u32x2* PNodeB;
  const PNodeB nodesB = (PNodeB)gf.nodes;
  TaEnv env;
  env.init(c, (rfl(Jp->ctx_flags) & kTaNoGoal) != 0, (const uint16_t*)(maps + rfl(Jp->heur_off)), small ? 32u : dimx,
           (uint32_t*)arenaSlot, rows);

  bool run = true;
  uint32_t h0 = 0;
  if (!tableOk) {
    status = ST_BAD;
    run = false;
  } else if (rows < 2u || !env.startH(c.sx, c.sy, h0)) {  // no room for a second time step / the task is out of reach
    status = ST_CAP_HORIZON;
    run = false;
  } else if (capN < 16u) {
    status = ST_CAP_NODES;
    run = false;
  }
  if (run) {
    u32x2 b0;
    b0.x = 0;
    b0.y = 0;  // focal position 0
    nodesB[0] = b0;
    const E e0 = T::pack(0, h0, 0, 0);
    g.open[0] = e0;
    g.focal[0] = e0;
    env.zeroRows(0);
    __syncthreads();
    env.newNode(g, 0, c.sx | (c.sy << 8), 0, 7u, kNoParent, 0, c.sy * dimx + c.sx);  // node 0, in the open list
    s.nNodes = 1; s.nOpen = 1; s.nFocal = 1;
    s.bestF = (int32_t)h0;
  }
  while (run) {
    if (s.nOpen == 0) {
      status = ST_NO_SOLUTION;
      break;
    }
    const E topE = ldU<T>(g.open, 0);
    {  // a_star_epsilon.hpp:134-154: bestFScore follows open.top() (also down); the ordered walk only when it rose
      const int32_t oldBest = s.bestF;
      s.bestF = (int32_t)T::f(topE);
      if (s.bestF > oldBest && !orderedWalkTaEps(g, gf, s, w, oldBest)) {
        status = ST_CAP_NODES;
        break;
      }
    }
    if (s.nFocal == 0) {  // (w < 1: the reference reads the top of an empty heap here)
      status = ST_BAD;
      break;
    }
    const E curE = ldU<T>(g.focal, 0);  // focalSet.top(): g, f, focalH as they are NOW (re-keyed in place)
    const uint32_t curId = T::id(curE), gcur = T::g(curE), curFh = T::fh(curE);
    const u32x4 nd = ((Mem<T>::PNode4)g.nodes)[curId];
    const uint32_t xyt = rfl(nd.x), curPos = rfl(nd.w);
    const uint32_t x = xyt & 0xFFu, y = (xyt >> 8) & 0xFFu, t = (xyt >> 16) & 0x7FFu;
    const uint32_t xy = xyt & 0xFFFFu;
    const bool atGoal = env.atGoal(x, y);
    s.expansions += 1;  // onExpandNode (a_star_epsilon.hpp:193) — counts the goal pop too
    if (c.maxExp >= 0 && s.expansions > c.maxExp) {
      status = ST_CAP_EXP;
      break;
    }
    if (atGoal && (int32_t)t > c.lastGoal) {  // isSolution (ecbs_ta.cpp:384-390) -> a_star_epsilon.hpp:195-213
      if (t + 1u > outStride) {
        status = ST_CAP_HORIZON;
        break;
      }
      TaEnv::walkPath(g, curId, t, outPath);
      status = ST_OK;
      cost = (int32_t)gcur;
      fmin = (int32_t)T::f(topE);  // openSet.top().fScore (a_star_epsilon.hpp:210)
      nStates = (int32_t)t + 1;
      break;
    }
    const uint32_t t1 = t + 1u;
    if (t1 >= env.rows || t1 >= g.capRows) {
      status = ST_CAP_HORIZON;
      break;
    }
    if (s.nNodes + 5u > capN || s.nOpen + 5u > capN || s.nFocal + 5u > capN) {
      status = ST_CAP_NODES;
      break;
    }
    // other agents' cells at t and t + 1 (x | y << 8), 64 agents per lane load; rows beyond the table repeat its last one
    uint32_t a0 = kEmptyCell, b0 = kEmptyCell, a1 = kEmptyCell, b1 = kEmptyCell;
    const uint16_t* rowA = nullptr;
    const uint16_t* rowB = nullptr;
    if (c.nAgentsPad) {
      const uint32_t ra = t < tPad ? t : tPad - 1;
      const uint32_t rb = t1 < tPad ? t1 : tPad - 1;
      rowA = c.paths + (size_t)ra * c.nAgentsPad;
      rowB = c.paths + (size_t)rb * c.nAgentsPad;
      if (lane < c.nAgentsPad) {
        a0 = rowA[lane];
        b0 = rowB[lane];
      }
      if (64 + lane < c.nAgentsPad) {
        a1 = rowA[64 + lane];
        b1 = rowB[64 + lane];
      }
    }
    heapPop<TF, 1, true>(gf, gf.focal, s.nFocal);  // focalSet.pop()          (a_star_epsilon.hpp:215)
    eraseOpen<T>(g, s.nOpen, curPos);              // openSet.erase(handle)   (:216)
    env.close(x, y, t);                            // stateToHeap.erase, closedSet.insert (:217-218)
    ensureRows<T>(g, s, c, t1);
    env.zeroRows(t1);
    __syncthreads();
    TaProbe pr;
    const uint32_t mask = env.probe(g, x, y, t, pr);
    const float bound = __fmul_rn((float)s.bestF, w);  // bestFScore * m_w (a_star_epsilon.hpp:240,265), binary32
    const uint64_t swap0 = ballot64(b0 == xy);
    const uint64_t swap1 = ballot64(b1 == xy);
    bool fail = false;
    for (uint32_t mm = mask; mm; mm &= mm - 1) {  // a_star_epsilon.hpp:223-281, neighbour by neighbour
      const uint32_t k = (uint32_t)__builtin_ctz(mm);
      const uint32_t st = __builtin_amdgcn_readlane(pr.st, k);
      if (st & 0x80000000u) continue;  // closed (:224)
      const uint32_t g2 = gcur + ((k == 0 && atGoal) ? 0u : 1u);  // tentative_gScore (:225)
      if (st == 0) {  // a new node (:227-247)
        const uint32_t h = __builtin_amdgcn_readlane(pr.h, k);
        const uint32_t cc = __builtin_amdgcn_readlane(pr.nxy, k);
        if (!TaEnv::fits(h, g2)) {
          status = ST_CAP_HORIZON;
          fail = true;
          break;
        }
        // focalStateHeuristic + focalTransitionHeuristic (ecbs_ta.cpp:314-344): an agent counts once if it stands on the
        // successor's cell at time t + 1 and once more if it is there at t and on this node's cell at t + 1 (a Wait too)
        uint32_t cnt = 0;
        if (c.nAgentsPad) {
          cnt = (uint32_t)__popcll(ballot64(b0 == cc)) + (uint32_t)__popcll(ballot64(a0 == cc) & swap0) +
                (uint32_t)__popcll(ballot64(b1 == cc)) + (uint32_t)__popcll(ballot64(a1 == cc) & swap1);
          for (uint32_t base = 128; base < c.nAgentsPad; base += 64) {
            uint32_t av = kEmptyCell, bv = kEmptyCell;
            if (base + lane < c.nAgentsPad) {
              av = rowA[base + lane];
              bv = rowB[base + lane];
            }
            cnt += (uint32_t)__popcll(ballot64(bv == cc)) + (uint32_t)__popcll(ballot64(av == cc && bv == xy));
          }
        }
        const uint32_t fh = curFh + cnt;
        if (fh > kFhMax) {
          status = ST_CAP_FOCAL;
          fail = true;
          break;
        }
        const uint32_t f2 = g2 + h;
        const uint32_t nid = s.nNodes++;
        env.newNode(g, nid, cc, t1, k, curId, g2, __builtin_amdgcn_readlane(pr.ncell, k));
        u32x2 nb;
        nb.x = fh;
        nb.y = kNoPos;
        nodesB[nid] = nb;
        const E e = T::pack(fh, f2, g2, nid);
        siftUp<T, 0, true>(g, g.open, s.nOpen, e);  // openSet.push (:237)
        s.nOpen += 1;
        if ((float)(int32_t)f2 <= bound) {          // focalSet.push (:240-243)
          siftUp<TF, 1, true>(gf, gf.focal, s.nFocal, e);
          s.nFocal += 1;
        }
      } else {  // still in the open list (:248-270)
        const uint32_t nid = st - 1u;
        uint32_t gOld, posOld, fOld, fNew;
        if (!TaEnv::rekey(g, nid, k, curId, g2, gOld, posOld, fOld, fNew)) continue;  // (:251-253)
        const u32x2 ob = nodesB[nid];
        const uint32_t fhOld = rfl(ob.x), fpos = rfl(ob.y);
        const E e = T::pack(fhOld, fNew, g2, nid);  // focalH keeps its value
        siftUp<T, 0, true>(g, g.open, posOld, e);   // openSet.increase(handle) (:262)
        if (fpos != kNoPos) {
          // already in the focal list: its entry reads the new f and g where it lies; the heap is not repaired
          if (fpos < s.nFocal) g.focal[fpos] = e;
        } else if ((float)(int32_t)fNew <= bound && (float)(int32_t)fOld > bound) {  // crossed the bound (:265-269)
          siftUp<TF, 1, true>(gf, gf.focal, s.nFocal, e);
          s.nFocal += 1;
        }
      }
    }
    if (fail) break;
  }
  out->status = status;
  out->cost = cost;
  out->fmin = fmin;
  out->n_states = nStates;
  out->expanded = s.expansions;
  out->nodes_created = s.nNodes;
  out->tier = 1;
}

// MRP_LL_ASTAR_EPS_TA with MRP_LL_JOB_TRY_LDS (kCtxTryLds): the search in its LDS tier (ll_compact_ta_eps.h
// ct::compactSearchTaEps), called by processJob in front of runJobTaEps.  True: the tier gave the answer (res.tier = 0).
// False: the job or the launch does not fit the tier — a map beyond 32 x 32, more than 64 vertex or 64 edge constraints,
// more than 128 context agents, the tier off or its path area below ct::kTePathBytes, a focal table that does not fit the
// slot's path area or is refused — or the search outgrew it (prof[6] / prof[7]: the expansions thrown away, as runJobTA);
// runJobTaEps<false> then runs the job from the start and stages everything again, unchanged.
// Constraint words and focal table go where runJobTaEps puts them: the slot's copy areas.  The cameFrom table takes the
// slot's node area, as for every compact tier.
DEVI bool runTaEpsLds(const LaunchParams& P, const DevJob& J, uint8_t* smem, uint8_t* arenaSlot, DevResult& res, uint16_t* outPath) {
  const uint32_t lane = threadIdx.x;
  const uint32_t pathBytes = J.t_pad * J.n_agents_pad * 2;  // multiple of 32
  const bool byId = (J.ctx_flags & kCtxById) != 0;
  if (P.lds_nodes == 0 || P.lds_paths_bytes < ct::kTePathBytes || !ct::taEpsJobFits(J.dimx, J.dimy, J.n_vc, J.n_ec, J.n_agents_pad) ||
      !compactFits<ct::Narrow>(P.arena_nodes, 0, false) || pathBytes > P.arena_paths_bytes || (byId && J.n_ctx > J.n_agents_pad))
    return false;
  const uint32_t* vc;
  const uint32_t* ec;
  stageConstraints(P.cons, J.vc_off, J.n_vc, J.n_ec, slot::consCopy(arenaSlot, P.arena_scratch_off, P.out_stride), vc, ec);
  uint8_t* pathsArena = slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  if (pathBytes != 0) {
    if (byId) {
      buildIdTableInArena((uint16_t*)pathsArena, P.cons + J.path_off, J.n_ctx, J.t_pad, J.n_agents_pad, P.path_store,
                          P.path_store_stride, P.path_store_slots);
    } else {
      const uint32_t* psrc = (const uint32_t*)(P.paths + J.path_off);
      uint32_t* dst = (uint32_t*)pathsArena;
      for (uint32_t i = lane; i < pathBytes / 4; i += 64) dst[i] = hostLoad32(psrc + i);
    }
  }
  __syncthreads();
  ct::CJob cj = baseCJob(P, J, arenaSlot, outPath);
  cj.sx = J.sx; cj.sy = J.sy; cj.gx = J.gx; cj.gy = J.gy;
  cj.lastGoal = J.last_goal_constraint;
  cj.nVc = J.n_vc; cj.nEc = J.n_ec;
  cj.nAgentsPad = pathBytes ? J.n_agents_pad : 0u; cj.tPad = pathBytes ? J.t_pad : 0u;
  cj.taNoGoal = (J.ctx_flags & kTaNoGoal) ? 1u : 0u;
  cj.rows = ct::kTeNodeCap;
  cj.vc = (uint64_t)vc; cj.ec = (uint64_t)ec;
  cj.pathsG = (uint64_t)pathsArena;
  cj.bitsG = (uint64_t)(P.maps + J.heur_off);  // the task's shortest-path table, [32][32] halfwords
  putCJob(smem, cj);
  const uint64_t tl0 = __builtin_amdgcn_s_memrealtime();
  const int32_t crc = ct::compactSearchTaEps((wv::Lds)smem);
  const ct::CRes cr = getCRes(smem);
  res.prof[0] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);
  res.prof[1] = cr.expanded;
  if (crc != ct::C_CAP_NODES && crc != ct::C_CAP_HORIZON && crc != ct::C_OVERFLOW) {  // an answer (the ST_ codes, ST_BAD included)
    res.status = crc; res.cost = cr.cost; res.fmin = cr.fmin; res.n_states = cr.nStates;
    res.expanded = cr.expanded; res.nodes_created = cr.nodes;
    res.tier = 0;
    return true;
  }
  res.prof[6] = cr.expanded;  // expansions thrown away with the attempt
  res.prof[7] = 1;
  __syncthreads();
  return false;
}

}  // namespace mrp

#endif  // MRP_LL_TA_H
