// SIPP (MRP_LL_SIPP, config 5): A* over (cell, safe interval) states.
// Reference: SIPP::search sipp.hpp:91-134 -> AStar::search a_star.hpp:63-161 over SIPPState with
// SIPPEnvironment::getNeighbors sipp.hpp:191-223 (motions Up, Down, Left, Right of mapf_prioritized_sipp.cpp:99-121;
// isCommandValid :129-142: arrival t = max(si.start, g + 1), cost t - g; swaps are not checked) and isSolution
// sipp.hpp:185-189 (goal cell AND the interval ends at INT_MAX).  Edge costs vary, so the decrease-key branch
// a_star.hpp:139-145 (`openSet.increase(handle)` == sift-up from the handle's position) is live here.
// Job tables (packed by the host, copied into the arena slot): cellIdx[cells] (halfwords; 0 = single default interval
// [0, INT_MAX], k+1 = special cell k), specFirst[K+1], ivals[total][2].  State id = cell for default cells,
// cells + specFirst[k] + i for interval i of special cell k.  Such a job runs in the arena tier only.
// Holds the packed x word, the three tiers (TierLdsSipp: nodes and open list in LDS; TierMix: open list in LDS, nodes in
// the arena; TierHbmX / TierHbm: everything in the arena), SippView (a job's own table or a device-resident one), the node
// accessors, sippLoop, sippCommitPath, runSipp and processSippJob.
// Needs ll_arena_heap.h (TierHbm, Mem, heap primitives) and ll_jobs.h (cutArena, hostStore32).
#ifndef MRP_LL_SIPP_H
#define MRP_LL_SIPP_H

namespace mrp {

// SIPP node "x" word as the search loop sees it: cell | interval << 16 | (interval ends at INT_MAX) << 31.  Packed forms
// (LDS node records, TierXT heap entries) squeeze it to kSippXBits = 16 + kSippIvBits + 1 bits.
constexpr uint32_t kSippIvBits = 4;  // kSippCap = 15 intervals per cell
static_assert((1u << kSippIvBits) > kSippCap, "interval index width");
constexpr uint32_t kSippXBits = 16 + kSippIvBits + 1;                       // 21
constexpr uint32_t kSippXLow = (1u << (16 + kSippIvBits)) - 1u;             // cell and interval
DEVI uint32_t sippPackX(uint32_t x) { return (x & kSippXLow) | (x >> 31) << (16 + kSippIvBits); }
DEVI uint32_t sippUnpackX(uint32_t v) { return (v & kSippXLow) | ((v >> (16 + kSippIvBits)) & 1u) << 31; }

// SIPP fast tier: nodes and open list in LDS.  32-bit entries [31:21] 2047 - f, [20:11] g (arrival time, <= kGMask),
// [10:0] node — the whole open key of TierHbm; one word per node, its g and its open position a halfword each.
struct TierLdsSipp {
  static constexpr int AS = 3;
  static constexpr int NAS = 3;
  static constexpr bool kWideNodes = false;  // one word per node + a halfword position array
  static constexpr bool kPosPair = false;
  static constexpr bool kEntryHasX = false;
  static constexpr bool kEntryXy = false;
  static constexpr bool kHybrid = false;
  typedef uint32_t E;
  typedef u32x2 Pair;
  static constexpr uint32_t kIdBits = 11, kMaxNodes = 1u << kIdBits;
  DEVI static E pack(uint32_t, uint32_t f, uint32_t g, uint32_t id) {  // (no focalH in this tier)
    return ((kFMax - f) << (kIdBits + kGBits)) | (g << kIdBits) | id;
  }
  DEVI static uint32_t keyFocal(E e) { return e >> kIdBits; }
  DEVI static uint32_t keyOpen(E e) { return (e >> kIdBits) & ((1u << (kGBits + kFBits)) - 1u); }
  DEVI static uint32_t id(E e) { return e & (kMaxNodes - 1u); }
  DEVI static uint32_t f(E e) { return kFMax - ((e >> (kIdBits + kGBits)) & kFMax); }
  DEVI static uint32_t g(E e) { return (e >> kIdBits) & kGMask; }
  DEVI static E first(E v) { return rfl(v); }
  DEVI static E fromLane(E v, uint32_t srcLane) { return __builtin_amdgcn_readlane(v, srcLane); }
  DEVI static E shr1(E v) { return waveShr1(v); }
};
// SIPP middle tier, for a search that has outgrown TierLdsSipp's kSippLdsCap - 1 = 767 nodes: the node records go to the
// arena, the open list stays in LDS as 64-bit entries (the whole fast-tier area, (kSippLdsBytes - 16) / 8 = 1152 of them
// with MRP_LL_SIPP_LDS_NODES = 768).  Only the open key of the entry is ever
// compared, so the 21 bits around it carry the node's x word (cell 16, interval 4, ends-at-INT_MAX 1): an expansion
// then needs no node read at all, like in the fast tier.
template <int HEAP_AS>
struct TierXT : TierHbm {
  static constexpr int AS = HEAP_AS;
  static constexpr int NAS = 1;
  static constexpr bool kEntryHasX = true;
  static constexpr uint32_t kIdBitsMix = 22;  // kMaxArenaNodes
  DEVI static uint32_t id(E e) { return (uint32_t)e & ((1u << kIdBitsMix) - 1u); }
  DEVI static E withX(E e, uint32_t x) {  // x = cell | interval << 16 | endsAtInf << 31
    const uint32_t v = sippPackX(x);                                           // 21 bits: 10 below the key word, 11 above the key
    // (pack() leaves 2047 - focalH = all ones in the eleven bits above the open key: they are cleared first)
    return (e & ~((uint64_t)kFhMax << (32 + kGBits + kFBits))) | ((uint64_t)(v & 0x3FFu) << kIdBitsMix) |
           ((uint64_t)(v >> 10) << (32 + kGBits + kFBits));
  }
  DEVI static uint32_t xOf(E e) {
    const uint32_t v = (((uint32_t)e >> kIdBitsMix) & 0x3FFu) | ((uint32_t)(e >> (32 + kGBits + kFBits)) & kFhMax) << 10;
    return sippUnpackX(v);
  }
};
typedef TierXT<3> TierMix;   // open list in LDS
typedef TierXT<1> TierHbmX;  // ... in the arena: the last tier of a search on a resident table (entries keep their x word)

constexpr int32_t kIntMax = 0x7FFFFFFF;

// Where runSipp finds a cell's safe intervals and a state's open/closed status.
//   RES = false: the job's own compact table, copied from the host into the arena (layout above); status words
//                (0 unseen, node + 1 in open, bit 31 closed) in the arena too, zeroed per job.
//   RES = true:  the device-resident table of an mrp_ll_sipp_table (ll_device.h kSippResident): per cell a 64-byte row
//                of bounds words + count (`ivals`) and a 64-byte row of status words, tagged with the job's epoch so
//                nothing is zeroed per job.
template <bool RES>
struct SippView {
  static constexpr uint32_t kClosed = RES ? kSippStClosed : 0x80000000u;
  const uint16_t* cellIdx;
  const uint32_t* specFirst;
  const int32_t* ivals;
  uint32_t* status;
  uint32_t cells, epochBits;
  // nk != 0: the cell has its own interval list, `n` entries from ivals[2 * first]; nk == 0: the default [0, INT_MAX]
  DEVI void lookup(uint32_t cell, uint32_t& nk, uint32_t& first, uint32_t& n) const {
    if constexpr (RES) {
      nk = (uint32_t)ivals[cell * kSippRowWords + 15u];
      first = 0;
      n = nk ? nk - 1 : 1;
    } else {
      nk = cellIdx[cell];
      first = 0;
      n = 1;
      if (nk) {
        first = specFirst[nk - 1];
        n = specFirst[nk] - first;
      }
    }
  }
  DEVI uint32_t sid(uint32_t cell, uint32_t nk, uint32_t first, uint32_t i) const {
    if constexpr (RES) return cell * kSippRowWords + i;
    return nk ? cells + first + i : cell;
  }
  DEVI uint32_t getSt(uint32_t id) const {
    uint32_t v = status[id];
    if constexpr (RES) v = (v >> kSippEpochShift) == (epochBits >> kSippEpochShift) ? (v & ((1u << kSippEpochShift) - 1u)) : 0u;
    return v;
  }
  DEVI void putSt(uint32_t id, uint32_t v) const { status[id] = RES ? (v | epochBits) : v; }
  // a bounds word of the resident table (ll_device.h)
  DEVI static int32_t bStart(uint32_t w) { return (int32_t)(w & 0xFFFFu); }
  DEVI static int32_t bEnd(uint32_t w) { return (w >> 16) == kSippEndInf ? 0x7FFFFFFF : (int32_t)(w >> 16); }
  DEVI static uint32_t bPack(int32_t s, int32_t e) { return (uint32_t)s | (e == 0x7FFFFFFF ? kSippEndInf : (uint32_t)e) << 16; }
};

// SIPP node records.  Arena tier: u32x4 { x = cell | interval << 16 | (RES: interval ends at INT_MAX) << 31, parent, g,
// position of the open entry }.  TierLdsSipp: one word  cell | interval << 16 | endsAtInf << 20 | parent << 21  (interval
// < kSippCap = 16; parent < 2047, 0x7FF = none), g in Mem::gOf, the position in Mem::pos.
constexpr uint32_t kSippNoParentLds = 0x7FFu;
template <class T>
DEVI uint32_t sippNodeX(Mem<T>& m, uint32_t id) {
  if constexpr (T::kWideNodes) {
    return rfl(((typename Mem<T>::PNode4)m.nodes)[id].x);
  } else {
    const uint32_t w = rfl(m.nodes[id]);
    return sippUnpackX(w);
  }
}
template <class T>
DEVI void sippNodeNew(Mem<T>& m, uint32_t id, uint32_t x, uint32_t parent, uint32_t t) {
  if constexpr (T::kWideNodes) {
    u32x4 nn;
    nn.x = x;
    nn.y = parent;
    nn.z = t;
    nn.w = 0;
    ((typename Mem<T>::PNode4)m.nodes)[id] = nn;
  } else {
    m.nodes[id] = sippPackX(x) | (parent & kSippNoParentLds) << kSippXBits;
    m.gOf[id] = (uint16_t)t;
  }
}
// g and open position of a node that is in the open list (decrease-key, a_star.hpp:130-146)
template <class T>
DEVI void sippNodeGPos(Mem<T>& m, uint32_t id, uint32_t& gOld, uint32_t& pos) {
  if constexpr (T::kWideNodes) {
    const u32x4 on = ((typename Mem<T>::PNode4)m.nodes)[id];
    gOld = rfl(on.z);
    pos = rfl(on.w);
  } else {
    gOld = rfl((uint32_t)m.gOf[id]);
    pos = rfl((uint32_t)m.pos[id]);
  }
}
template <class T>
DEVI void sippNodeReparent(Mem<T>& m, uint32_t id, uint32_t parent, uint32_t t) {  // cameFrom update + new g
  if constexpr (T::kWideNodes) {
    m.nodes[id * 4 + 1] = parent;
    m.nodes[id * 4 + 2] = t;
  } else {
    m.nodes[id] = (rfl(m.nodes[id]) & ((1u << kSippXBits) - 1u)) | (parent & kSippNoParentLds) << kSippXBits;
    m.gOf[id] = (uint16_t)t;
  }
}
template <class T>
DEVI void sippNodePath(Mem<T>& m, uint32_t id, uint32_t& cell, uint32_t& gN, uint32_t& parent) {
  if constexpr (T::kWideNodes) {
    const u32x4 pn = ((typename Mem<T>::PNode4)m.nodes)[id];
    cell = rfl(pn.x) & 0xFFFFu;
    gN = rfl(pn.z);
    parent = rfl(pn.y);
  } else {
    const uint32_t w = rfl(m.nodes[id]);
    cell = w & 0xFFFFu;
    gN = rfl((uint32_t)m.gOf[id]);
    parent = (w >> kSippXBits) == kSippNoParentLds ? kNoParent : (w >> kSippXBits);
  }
}

template <class T>
DEVI typename T::E sippEntry(uint32_t f, uint32_t gN, uint32_t id, uint32_t x) {
  typename T::E e = T::pack(0, f, gN, id);
  if constexpr (T::kEntryHasX) e = T::withX(e, x);
  return e;
}

struct SippState {  // wave-uniform
  uint32_t nNodes, nOpen;
  int64_t expansions;
};
constexpr int32_t kSippNextTier = -1;  // sippLoop's answer that is not a status: runSipp continues the search in its next tier

// The search loop over one memory tier.  Returns the job's status, or kSippNextTier when an LDS tier has no room for the
// successors of the next expansion (nothing of that expansion has happened yet: the caller copies nodes and open list
// into the next tier and calls that instance with the same state).
template <class T, bool RES>
DEVI int32_t sippLoop(const LaunchParams& P, const DevJob& J, Mem<T>& g, const SippView<RES>& tv, SippState& s,
                      DevResult& res, uint16_t* outPath) {
  const uint32_t lane = threadIdx.x;
  const uint32_t dimx = J.dimx, dimy = J.dimy;
  const uint32_t gx = J.gx, gy = J.gy;
  const int64_t maxExp = J.max_expansions;
  const uint32_t* obst = P.maps + J.map_word_off;
  const int32_t* ivals = tv.ivals;
  uint32_t& nNodes = s.nNodes;
  uint32_t& nOpen = s.nOpen;
  int64_t& expansions = s.expansions;
  const uint32_t divMagic = rfl(0xFFFFFFFFu / dimx + 1u);
  for (;;) {
    if (nOpen == 0) {
      res.status = ST_NO_SOLUTION;
      break;
    }
    const typename T::E curE = ldU<T>(g.open, 0);
    const uint32_t curId = T::id(curE);
    uint32_t cw;
    if constexpr (T::kEntryHasX)
      cw = T::xOf(curE);
    else
      cw = sippNodeX<T>(g, curId);
    const uint32_t cell = cw & 0xFFFF, iv = RES ? (cw >> 16) & 0x7FFFu : cw >> 16;
    const uint32_t gcur = T::g(curE);  // == the node's g: every entry is packed with it
    // cell / dimx without the ~30-instruction division sequence: one multiply-high by floor(2^32 / dimx) + 1 is exact for
    // cell < 2^16 and dimx <= 2^16 (the product overshoots cell / dimx by less than 2^-16 < 1 / dimx)
    const uint32_t cy = dimx == 1u ? cell : __umulhi(cell, divMagic), cx = cell - cy * dimx;
    // RES: every table word this expansion needs has an address that follows from (cell, iv) alone — the cell's own
    // list length and interval end, and for the four neighbours (lanes 16 * motion + i) the obstacle word, the list
    // length, interval slot i and its status word: two 64-byte sectors per cell.  All of
    // it is requested here, in ONE round trip, and the heap pop below (LDS tier) runs while it is in flight; slots beyond
    // a list's length hold stale words that are loaded and ignored.  "Ends at INT_MAX", which the goal test needs at
    // once, rides in bit 31 of the node's x.
    uint32_t ck = 0, f0 = 0, nCur = 0;
    int32_t endT = kIntMax;
    uint32_t r_nc = 0, r_obstW = 0xFFFFFFFFu, r_nk = 0, r_st = 0, r_ck = 0, r_h = 0;
    uint32_t r_bw = 0, r_endW = 0;  // raw bounds words: decoded where they are used, BEHIND the heap pop (a decode here
                                    // would make the wavefront wait for the table before it pops)
    bool r_inb = false;
    if constexpr (RES) {
      const uint32_t mm = lane >> 4, i = lane & 15u;
      const uint32_t nx = cx + (mm == 3) - (mm == 2), ny = cy + (mm == 0) - (mm == 1);
      r_inb = nx < dimx && ny < dimy;
      r_nc = r_inb ? ny * dimx + nx : 0;
      r_h = (nx > gx ? nx - gx : gx - nx) + (ny > gy ? ny - gy : gy - ny);
      const int32_t* rowN = ivals + r_nc * kSippRowWords;
      r_ck = (uint32_t)ivals[cell * kSippRowWords + 15u];
      r_endW = (uint32_t)ivals[cell * kSippRowWords + iv];
      r_obstW = obst[r_nc >> 5];
      r_nk = (uint32_t)rowN[15];
      if (i < kSippCap) {
        r_bw = (uint32_t)rowN[i];
        r_st = tv.status[r_nc * kSippRowWords + i];
      }
      if (!(cw >> 31)) endT = 0;  // any finite value: the goal test below only asks whether it is INT_MAX
    } else {
      tv.lookup(cell, ck, f0, nCur);
      ck = rfl(ck);
      f0 = rfl(f0);
      if (ck) endT = rfli(ivals[2 * (f0 + iv) + 1]);
    }
    if constexpr (T::AS == 3) {  // LDS tiers: room for every successor of this expansion, or continue in the next tier
      if (nNodes + 4 * kSippCap > g.capNodes || nOpen + 4 * kSippCap > g.capHeap) return kSippNextTier;
    }
    expansions += 1;
    if (maxExp >= 0 && expansions > maxExp) {
      res.status = ST_CAP_EXP;
      break;
    }
    if (cx == gx && cy == gy && endT == kIntMax) {
      // raw A* solution: (cell, g) per state; the host inserts the explicit Wait actions (sipp.hpp:105-128)
      uint32_t len = 0;
      for (uint32_t nid = curId; nid != kNoParent;) {
        uint32_t pc, pg, pp;
        sippNodePath<T>(g, nid, pc, pg, pp);
        nid = pp;
        len += 1;
      }
      if (len * 2 > P.out_stride) {
        res.status = ST_CAP_HORIZON;
        break;
      }
      uint32_t* out32 = (uint32_t*)outPath;
      uint32_t nid = curId;
      for (int32_t k = (int32_t)len - 1; k >= 0; --k) {
        uint32_t pc, pg, pp;
        sippNodePath<T>(g, nid, pc, pg, pp);
        out32[k] = pc | (pg << 16);
        nid = pp;
      }
      res.status = ST_OK;
      res.cost = (int32_t)gcur;
      res.fmin = (int32_t)T::f(curE);
      res.n_states = (int32_t)len;
      break;
    }
    heapPop<T, 0, true>(g, g.open, nOpen);
    if constexpr (RES) {
      ck = rfl(r_ck);
      f0 = 0;
      if (ck) endT = SippView<RES>::bEnd(rfl(r_endW));
      else endT = kIntMax;
    }
    const uint32_t curSid = tv.sid(cell, ck, f0, iv);
    tv.putSt(curSid, SippView<RES>::kClosed);
    const uint32_t startT = gcur + 1;
    if (startT > kGMask) {
      res.status = ST_CAP_HORIZON;
      break;
    }
    bool fail = false;
    // ---- neighbours.  Lanes 0..3 probe the four motions Up, Down, Left, Right at once (bounds, obstacle bit, the
    // cell's safe-interval list); when no list is longer than 16 the intervals of all four cells are then evaluated on
    // lanes 16*m + i together with their open/closed status — three dependent global round trips per expansion
    // instead of three to five per motion.  Candidates are consumed in lane order, which IS the reference's order
    // (motion-major, interval-minor, sipp.hpp:205-222).
    uint32_t c4[4] = {0, 0, 0, 0}, f4[4] = {0, 0, 0, 0}, nc4[4] = {0, 0, 0, 0}, nk4[4] = {0, 0, 0, 0}, h4[4] = {0, 0, 0, 0};
    if constexpr (!RES) {
      const uint32_t nxL = cx + (lane == 3) - (lane == 2), nyL = cy + (lane == 0) - (lane == 1);
      const bool inbL = lane < 4 && nxL < dimx && nyL < dimy;
      const uint32_t ncL = inbL ? nyL * dimx + nxL : 0;
      uint32_t obstW = 0xFFFFFFFFu, nkL = 0, firstL = 0, cntL = 0;
      if (inbL) {
        obstW = obst[ncL >> 5];
        tv.lookup(ncL, nkL, firstL, cntL);
      }
      const bool validL = inbL && !((obstW >> (ncL & 31)) & 1u);
      if (!validL) cntL = 0;
      const uint32_t hL = (nxL > gx ? nxL - gx : gx - nxL) + (nyL > gy ? nyL - gy : gy - nyL);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        c4[m] = __builtin_amdgcn_readlane(cntL, m);
        f4[m] = __builtin_amdgcn_readlane(firstL, m);
        nc4[m] = __builtin_amdgcn_readlane(ncL, m);
        nk4[m] = __builtin_amdgcn_readlane(nkL, m);
        h4[m] = __builtin_amdgcn_readlane(hL, m);
      }
    }
    const uint32_t cMax = RES ? 0u : max(max(c4[0], c4[1]), max(c4[2], c4[3]));
    if (cMax <= 16) {
      const uint32_t mm = lane >> 4, i = lane & 15;
      uint32_t cntM, firstM, ncM, nkM, hM, sidL, stL = 0;
      int32_t siS = 0, siE = kIntMax;
      bool act;
      if constexpr (RES) {
        const bool valid = r_inb && !((r_obstW >> (r_nc & 31)) & 1u);
        nkM = r_nk;
        ncM = r_nc;
        hM = r_h;
        firstM = 0;
        cntM = valid ? (nkM ? nkM - 1 : 1u) : 0u;
        act = i < cntM;
        sidL = tv.sid(r_nc, 0, 0, i);
        if (act) {
          if (nkM) {
            siS = SippView<RES>::bStart(r_bw);
            siE = SippView<RES>::bEnd(r_bw);
          }
          stL = (r_st >> kSippEpochShift) == (tv.epochBits >> kSippEpochShift) ? (r_st & ((1u << kSippEpochShift) - 1u)) : 0u;
        }
      } else {
        cntM = mm == 0 ? c4[0] : mm == 1 ? c4[1] : mm == 2 ? c4[2] : c4[3];
        firstM = mm == 0 ? f4[0] : mm == 1 ? f4[1] : mm == 2 ? f4[2] : f4[3];
        ncM = mm == 0 ? nc4[0] : mm == 1 ? nc4[1] : mm == 2 ? nc4[2] : nc4[3];
        nkM = mm == 0 ? nk4[0] : mm == 1 ? nk4[1] : mm == 2 ? nk4[2] : nk4[3];
        hM = mm == 0 ? h4[0] : mm == 1 ? h4[1] : mm == 2 ? h4[2] : h4[3];
        act = i < cntM;
        sidL = tv.sid(ncM, nkM, firstM, i);
        if (act) {
          if (nkM) {
            siS = ivals[2 * (firstM + i)];
            siE = ivals[2 * (firstM + i) + 1];
          }
          stL = tv.getSt(sidL);
        }
      }
      // sipp.hpp:209: skip if si.start - m_time > end_t || si.end < start_t
      const bool cand = act && !((int64_t)siS - 1 > (int64_t)endT || siE < (int32_t)startT);
      const uint32_t tArr = (uint32_t)(siS > (int32_t)startT ? siS : (int32_t)startT);
      const uint64_t candMask = ballot64(cand);
      const uint64_t lateMask = ballot64(cand && tArr > kGMask);
      const uint64_t openMask = ballot64(cand && stL != 0 && !(stL & SippView<RES>::kClosed));   // already in the open list
      const uint64_t newMask = ballot64(cand && stL == 0);
      const uint32_t nNew = (uint32_t)__popcll(newMask);
      if (lateMask) {
        res.status = ST_CAP_HORIZON;
        fail = true;
      } else if (openMask == 0 && nNew <= 5) {
        // the usual case — nothing to re-key: all pushes of the expansion in one round trip (PushChains)
        if (nNodes + nNew > g.capNodes) {
          res.status = ST_CAP_NODES;
          fail = true;
        } else if (nNew) {
          typename T::E e[5];
          uint64_t mk = newMask;
#pragma unroll
          for (uint32_t k = 0; k < 5; ++k) {
            e[k] = 0;
            if (k < nNew) {
              const uint32_t l = (uint32_t)__builtin_ctzll(mk);
              mk &= mk - 1;
              const uint32_t t = __builtin_amdgcn_readlane(tArr, l);
              const uint32_t sid = __builtin_amdgcn_readlane(sidL, l);
              const uint32_t nc = __builtin_amdgcn_readlane(ncM, l);
              const uint32_t hN = __builtin_amdgcn_readlane(hM, l);
              const uint32_t nid = nNodes + k;
              const uint32_t xN = nc | ((l & 15u) << 16) | (RES ? __builtin_amdgcn_readlane(siE == kIntMax ? 1u : 0u, l) << 31 : 0u);
              sippNodeNew<T>(g, nid, xN, curId, t);
              tv.putSt(sid, nid + 1);
              e[k] = sippEntry<T>(t + hN, t, nid, xN);
            }
          }
          const uint32_t pm = (1u << nNew) - 1u;
          PushChains<T> pc;
          pc.load(g.open, nOpen, pm);
          pc.template resolve<0, true>(g, g.open, nOpen, pm, e);
          nNodes += nNew;
          nOpen += nNew;
        }
      } else {
        uint64_t mask = candMask;
        while (mask && !fail) {
          const uint32_t l = (uint32_t)__builtin_ctzll(mask);
          mask &= mask - 1;
          const uint32_t t = __builtin_amdgcn_readlane(tArr, l);
          const uint32_t sid = __builtin_amdgcn_readlane(sidL, l);
          const uint32_t nc = __builtin_amdgcn_readlane(ncM, l);
          const uint32_t hN = __builtin_amdgcn_readlane(hM, l);
          const uint32_t st = __builtin_amdgcn_readlane(stL, l);
          if (st & SippView<RES>::kClosed) continue;                   // closedSet.find (a_star.hpp:117)
          const uint32_t xN = nc | ((l & 15u) << 16) | (RES ? __builtin_amdgcn_readlane(siE == kIntMax ? 1u : 0u, l) << 31 : 0u);
          if (st == 0) {                                   // new state (a_star.hpp:120-129)
            if (nNodes >= g.capNodes) {
              res.status = ST_CAP_NODES;
              fail = true;
              break;
            }
            const uint32_t nid = nNodes++;
            sippNodeNew<T>(g, nid, xN, curId, t);
            tv.putSt(sid, nid + 1);
            siftUp<T, 0, true>(g, g.open, nOpen, sippEntry<T>(t + hN, t, nid, xN));
            nOpen += 1;
          } else {                                         // already in open (a_star.hpp:130-146)
            const uint32_t nid = st - 1;
            uint32_t gOld, posOld;
            sippNodeGPos<T>(g, nid, gOld, posOld);
            if (t >= gOld) continue;
            sippNodeReparent<T>(g, nid, curId, t);
            siftUp<T, 0, true>(g, g.open, posOld, sippEntry<T>(t + hN, t, nid, xN));  // increase(handle)
          }
        }
      }
    } else {
      // a cell with more than 16 safe intervals: one motion at a time, 64 intervals per pass
      for (uint32_t m = 0; m < 4 && !fail; ++m) {  // Up, Down, Left, Right
        const uint32_t nx = cx + (m == 3) - (m == 2), ny = cy + (m == 0) - (m == 1);
        if (nx >= dimx || ny >= dimy) continue;
        const uint32_t nc = ny * dimx + nx;
        if ((rfl(obst[nc >> 5]) >> (nc & 31)) & 1u) continue;
        uint32_t nk, first, cnt;
        tv.lookup(nc, nk, first, cnt);
        nk = rfl(nk);
        first = rfl(first);
        cnt = rfl(cnt);
        const uint32_t hN = (nx > gx ? nx - gx : gx - nx) + (ny > gy ? ny - gy : gy - ny);
        for (uint32_t base = 0; base < cnt && !fail; base += 64) {
          const uint32_t i = base + lane;
          int32_t siS = 0, siE = kIntMax;
          if (nk && i < cnt) {
            siS = ivals[2 * (first + i)];
            siE = ivals[2 * (first + i) + 1];
          }
          // sipp.hpp:209: skip if si.start - m_time > end_t || si.end < start_t
          const bool cand = (i < cnt) && !((int64_t)siS - 1 > (int64_t)endT || siE < (int32_t)startT);
          const uint32_t tArr = (uint32_t)(siS > (int32_t)startT ? siS : (int32_t)startT);
          uint64_t mask = ballot64(cand);
          while (mask) {
            const uint32_t l = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1;
            const uint32_t ii = base + l;
            const uint32_t t = __builtin_amdgcn_readlane(tArr, l);
            if (t > kGMask) {
              res.status = ST_CAP_HORIZON;
              fail = true;
              break;
            }
            const uint32_t sid = tv.sid(nc, nk, first, ii);
            const uint32_t st = rfl(tv.getSt(sid));
            if (st & SippView<RES>::kClosed) continue;                   // closedSet.find (a_star.hpp:117)
            if (st == 0) {                                   // new state (a_star.hpp:120-129)
              if (nNodes >= g.capNodes) {
                res.status = ST_CAP_NODES;
                fail = true;
                break;
              }
              const uint32_t nid = nNodes++;
              sippNodeNew<T>(g, nid, nc | (ii << 16), curId, t);
              tv.putSt(sid, nid + 1);
              siftUp<T, 0, true>(g, g.open, nOpen, T::pack(0, t + hN, t, nid));
              nOpen += 1;
            } else {                                         // already in open (a_star.hpp:130-146)
              const uint32_t nid = st - 1;
              uint32_t gOld, posOld;
              sippNodeGPos<T>(g, nid, gOld, posOld);
              if (t >= gOld) continue;
              sippNodeReparent<T>(g, nid, curId, t);
              siftUp<T, 0, true>(g, g.open, posOld, T::pack(0, t + hN, t, nid));  // increase(handle)
            }
          }
        }
      }
    }
    if (fail) return res.status;
  }
  return res.status;
}

// sipp_commit (mrp_ll.h): the stays of the path just found — state k = (cell, arrival t_k) occupies its cell during
// [t_k, t_{k+1} - 1], the last one during [t_last, INT_MAX] — become collision intervals of the resident table, i.e. each
// splits the safe interval that contains it (what SIPP::setCollisionIntervals, sipp.hpp:245-284, yields for the longer
// collision list; the stay lies inside ONE safe interval because the search kept the agent there).  One lane per state,
// 64 states per pass; lanes whose states share a cell take turns.  Returns false if a cell would need more than kSippCap
// intervals or a stay is not inside a safe interval: the table is then left half-updated and the host redoes it.
DEVI bool sippCommitPath(const SippView<true>& tv, const uint32_t* path, uint32_t len) {
  const uint32_t lane = threadIdx.x;
  bool bad = false;
  for (uint32_t base = 0; base < len; base += 64) {
    const uint32_t k = base + lane;
    const bool act = k < len;
    const uint32_t w = act ? path[k] : 0xFFFFFFFFu;
    const uint32_t wn = (k + 1 < len) ? path[k + 1] : 0;
    const uint32_t cell = w & 0xFFFFu;
    const int32_t s0 = (int32_t)(w >> 16);
    const int32_t e0 = (k + 1 < len) ? (int32_t)(wn >> 16) - 1 : kIntMax;
    // how many earlier states of this pass sit on the same cell (a path may come back to a cell)
    uint32_t rank = 0;
    const uint32_t nAct = min(len - base, 64u);
    for (uint32_t j = 0; j + 1 < nAct; ++j) {
      const uint32_t cj = __builtin_amdgcn_readlane(cell, j);
      rank += (j < lane && cj == cell) ? 1u : 0u;
    }
    uint64_t todo = ballot64(act);
    for (uint32_t turn = 0; todo; ++turn) {
      const bool mine = act && rank == turn;
      if (mine) {
        u32x4* row4 = (u32x4*)(tv.ivals + cell * kSippRowWords);  // bounds words 0 .. 14, the count in word 15
        uint32_t rw[kSippRowWords];
#pragma unroll
        for (uint32_t v4 = 0; v4 < kSippRowWords / 4; ++v4) {
          const u32x4 v = row4[v4];
          rw[4 * v4] = v.x; rw[4 * v4 + 1] = v.y; rw[4 * v4 + 2] = v.z; rw[4 * v4 + 3] = v.w;
        }
        const uint32_t n1 = rw[15];
        const uint32_t n = n1 ? n1 - 1 : 1u;
        int32_t rs[kSippCap], re[kSippCap];
        if (n1) {
#pragma unroll
          for (uint32_t q = 0; q < kSippCap; ++q) {
            rs[q] = SippView<true>::bStart(rw[q]);
            re[q] = SippView<true>::bEnd(rw[q]);
          }
        } else {
#pragma unroll
          for (uint32_t q = 0; q < kSippCap; ++q) { rs[q] = 0; re[q] = -1; }
          rs[0] = 0;
          re[0] = kIntMax;
        }
        uint32_t kk = kSippCap;  // the safe interval that contains the stay
#pragma unroll
        for (uint32_t q = kSippCap; q-- > 0;)
          if (q < n && rs[q] <= s0 && e0 <= re[q]) kk = q;
        int32_t a = 0, b = 0;
#pragma unroll
        for (uint32_t q = 0; q < kSippCap; ++q)
          if (q == kk) { a = rs[q]; b = re[q]; }
        const bool left = a <= s0 - 1, right = e0 < b;
        const int32_t d = (left ? 1 : 0) + (right ? 1 : 0) - 1;
        if (kk == kSippCap || n + d > kSippCap) {
          bad = true;
        } else {
          int32_t ns[kSippCap], ne[kSippCap];
#pragma unroll
          for (uint32_t q = 0; q < kSippCap; ++q) {
            // entry q of the new list: below kk unchanged; at kk the left part, else the right part, else (both gone)
            // the old successor; above kk the old list shifted by d
            int32_t vs = rs[q], ve = re[q];
            if (q >= kk) {
              const int32_t ps = q > 0 ? rs[q - 1] : 0, pe = q > 0 ? re[q - 1] : 0;          // old[q - 1]
              const int32_t fs = q + 1 < kSippCap ? rs[q + 1] : 0, fe = q + 1 < kSippCap ? re[q + 1] : 0;  // old[q + 1]
              if (d == 1) {
                if (q == kk) { vs = a; ve = s0 - 1; }
                else if (q == kk + 1) { vs = e0 + 1; ve = b; }
                else { vs = ps; ve = pe; }
              } else if (d == 0) {
                if (q == kk) { vs = left ? a : e0 + 1; ve = left ? s0 - 1 : b; }
              } else {
                vs = fs; ve = fe;
              }
            }
            ns[q] = vs;
            ne[q] = ve;
          }
          // (slots beyond the new list get whatever the shift brought along; nobody reads them.  The status words are
          // left alone: they belong to this job's epoch, and the next job of the table has another)
#pragma unroll
          for (uint32_t q = 0; q < kSippCap; ++q) rw[q] = SippView<true>::bPack(ns[q] & 0xFFFF, ne[q] == kIntMax ? kIntMax : (ne[q] & 0xFFFF));
          rw[15] = n + d + 1;
#pragma unroll
          for (uint32_t v4 = 0; v4 < kSippRowWords / 4; ++v4) {
            u32x4 v;
            v.x = rw[4 * v4]; v.y = rw[4 * v4 + 1]; v.z = rw[4 * v4 + 2]; v.w = rw[4 * v4 + 3];
            row4[v4] = v;
          }
        }
      }
      todo &= ~ballot64(mine);
      // the next turn reads rows this one wrote (other lanes of the same wave; the table is uncached memory, so a store
      // that has been acknowledged is what a later load sees)
      if (todo) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (base + 64 < len) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  return ballot64(bad) == 0;
}

// LDS of a resident SIPP workgroup: TierLdsSipp's nodes, positions, g and open list — or TierMix's open list alone
// 768 nodes = 9.2 KB = 16 searches per CU.  With the tables in uncached memory and no fence pair per job, residency pays
// (scripts/r4_run35.sh, r4_run36.sh, 100 / 200 agents: 2048 nodes, 6 per CU: 5.5 / 5.5e8 expansions/s; 1536, 8 per CU:
// 6.5 / 6.5e8; 1024, 12 per CU: 7.2 / 7.4e8; 768, 16 per CU: 7.8 / 8.0e8; 512, 16 per CU: 7.6 / 7.1e8) although every
// expansion gets slower (2.2 -> 2.7 us) and more searches continue in the middle tier (open list in LDS, nodes in the arena).
#ifndef MRP_LL_SIPP_LDS_NODES
#define MRP_LL_SIPP_LDS_NODES 768
#endif
constexpr uint32_t kSippLdsCap = MRP_LL_SIPP_LDS_NODES;  // <= TierLdsSipp::kMaxNodes; ids 0 .. kSippLdsCap - 2 are used
static_assert(kSippLdsCap <= TierLdsSipp::kMaxNodes && kSippLdsCap % 4 == 0, "SIPP LDS tier capacity");
constexpr uint32_t kSippLdsBytes = kSippLdsCap * (4 + 2 + 2) + kSippLdsCap * 4 + 16;

template <bool RES>
DEVI void runSipp(const LaunchParams& P, const DevJob& J, uint8_t* arenaSlot, uint8_t* ldsTier, uint32_t ldsNodes, DevResult& res,
                  uint16_t* outPath) {
  const uint32_t lane = threadIdx.x;
  const uint32_t dimx = J.dimx, dimy = J.dimy, cells = dimx * dimy;
  const uint32_t K = J.n_vc, totalIv = J.n_ec;
  const uint32_t gx = J.gx, gy = J.gy;
  typedef TierHbm T;
  Mem<T> g = cutArena(P, arenaSlot);
  const Mem<T>::PNode4 gNodes = (Mem<T>::PNode4)g.nodes;
  uint32_t* tab = (uint32_t*)slot::pathsCopy(arenaSlot, P.arena_scratch_off, P.out_stride);
  SippView<RES> tv;
  tv.cells = cells;
  tv.epochBits = 0;
  if constexpr (RES) {
    uint8_t* rt = (uint8_t*)((uint64_t)J.n_agents_pad | ((uint64_t)J.path_off << 32));
    uint32_t* rec = (uint32_t*)rt;  // bounds rows, then status rows (ll_device.h)
    tv.ivals = (const int32_t*)rec;
    tv.status = rec + (size_t)cells * kSippRowWords;
    tv.epochBits = J.n_ctx << kSippEpochShift;
    tv.cellIdx = nullptr;
    tv.specFirst = nullptr;
    // (the table was last written by another workgroup, possibly on another XCD: it is uncached memory, that workgroup's
    // stores had been acknowledged before it published its job as done, and the host packed this job after seeing that)
    const uint32_t nRec = J.ec_off & 0x7FFFFFFFu;
    if (J.ec_off >> 31) {  // first job of the table (or its epochs are used up): no cell has a list, no state is seen
      u32x4 z;
      z.x = z.y = z.z = z.w = 0;
      u32x4* s4 = (u32x4*)rec;
      for (uint32_t i = lane; i < cells * (2u * kSippRowWords / 4); i += 64) s4[i] = z;
      __syncthreads();
    }
    // the cells whose lists changed since the table's previous job, out of pinned host memory: lane u copies 16 bytes
    // (four bounds words) of record u / recUnits, four rounds in flight
    const uint32_t* hdr = P.cons + J.vc_off;
    const u32x4* recs = (const u32x4*)(hdr + ((nRec + 3u) & ~3u));
    const uint32_t recUnits = J.n_vc / 4;      // 16-byte units per record of this job (a power of two, 1 .. 4)
    const uint32_t recShift = 31u - (uint32_t)__builtin_clz(recUnits | 1u);
    const uint32_t nUnits = nRec * recUnits;
    for (uint32_t u0 = 0; u0 < nUnits; u0 += 256) {
      uint32_t h[4];
      u32x4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t u = u0 + q * 64 + lane;
        if (u < nUnits) {
          h[q] = __builtin_nontemporal_load(hdr + (u >> recShift));
          v[q] = __builtin_nontemporal_load(recs + u);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t u = u0 + q * 64 + lane;
        if (u < nUnits) {
          const uint32_t cell = h[q] & 0xFFFFu;
          // the unit holds bounds words q0 .. q0 + 3; word 15 of a row is the count, which the host has put into the last
          // word of a 16-word record (packSippResident), and which the lane of unit 0 writes for a shorter one
          const uint32_t q0 = u & (recUnits - 1u);
          ((u32x4*)rec)[cell * (kSippRowWords / 4) + q0] = v[q];
          if (q0 == 0 && recUnits < 4u) rec[cell * kSippRowWords + 15u] = (h[q] >> 16) + 1u;
        }
      }
    }
    __syncthreads();
  } else {
  const uint32_t cw = (cells + 1) / 2;  // cellIdx is a halfword per cell (cells <= 65025, so K + 1 fits)
  const uint32_t tabWords = cw + K + 1 + 2 * totalIv;
  const uint32_t nStates = cells + totalIv;
  if (tabWords * 4 > P.arena_paths_bytes || nStates > P.arena_rows * P.arena_row_words) {
    res.status = ST_CAP_NODES;
    return;
  }
  {
    // The job's safe-interval table (10-30 KB) comes out of pinned HOST memory: every load instruction is a PCIe round
    // trip, so the copy is made of 16-byte lanes with eight loads in flight per lane (8 KB per round trip); dword by
    // dword it was ~100 dependent round trips and the largest part of a job's time.
    const uint32_t* src = P.cons + J.vc_off;
    uint32_t done = 0;
    if ((J.vc_off & 3u) == 0) {  // session slots are 16-byte aligned; a batch's tables start wherever the previous ended
      const u32x4* src4 = (const u32x4*)src;
      u32x4* dst4 = (u32x4*)tab;
      const uint32_t n4 = tabWords / 4;
      uint32_t i = lane;
      for (; i + 7 * 64 < n4; i += 8 * 64) {
        u32x4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = __builtin_nontemporal_load(src4 + i + q * 64);
#pragma unroll
        for (int q = 0; q < 8; ++q) dst4[i + q * 64] = v[q];
      }
      for (; i < n4; i += 64) dst4[i] = __builtin_nontemporal_load(src4 + i);
      done = n4 * 4;
    }
    for (uint32_t i = done + lane; i < tabWords; i += 64) tab[i] = src[i];
    u32x4 z;
    z.x = z.y = z.z = z.w = 0;  // status: 0 unseen, node+1 in open, bit 31 closed
    u32x4* st4 = (u32x4*)(uint32_t*)g.bits;
    for (uint32_t i = lane; i < (nStates + 3) / 4; i += 64) st4[i] = z;
  }
  __syncthreads();
  tv.cellIdx = (const uint16_t*)tab;
  tv.specFirst = tab + cw;
  tv.ivals = (const int32_t*)(tab + cw + K + 1);
  tv.status = (uint32_t*)g.bits;
  }
  // start interval (findSafeInterval, sipp.hpp:286-296): found by the host for a table that travels with the job, here
  // for a resident one (the host's copy may be behind)
  uint32_t startIv = J.t_pad, startInf = 0;
  if constexpr (RES) {
    const uint32_t sc = J.sy * dimx + J.sx;
    const int32_t st0 = J.last_goal_constraint;
    const uint32_t n1 = rfl((uint32_t)tv.ivals[sc * kSippRowWords + 15u]);
    if (n1 == 0) {
      startIv = 0;
      startInf = 1;
    } else {
      int32_t a = 0, b = -1;
      if (lane < n1 - 1) {
        const uint32_t bw = (uint32_t)tv.ivals[sc * kSippRowWords + lane];
        a = SippView<true>::bStart(bw);
        b = SippView<true>::bEnd(bw);
      }
      const uint64_t hit = ballot64(lane < n1 - 1 && a <= st0 && b >= st0);
      if (hit) {
        startIv = (uint32_t)__builtin_ctzll(hit);
        startInf = __builtin_amdgcn_readlane(b == kIntMax ? 1u : 0u, startIv);
      } else {
        startIv = 0xFFFFFFFFu;
      }
    }
  }
  if (startIv == 0xFFFFFFFFu) {  // no safe interval contains the start time: SIPP::search returns false (sipp.hpp:98-100)
    res.status = ST_NO_SOLUTION; // (after the table update: a resident table must not miss this job's delta)
    return;
  }

  // start node
  SippState s;
  s.nNodes = 1;
  s.nOpen = 1;
  s.expansions = 0;
  u32x4 n0;
  uint64_t e0;
  {
    const uint32_t sc = J.sy * dimx + J.sx;
    const uint32_t si = startIv;
    const uint32_t h0 = (J.sx > gx ? J.sx - gx : gx - J.sx) + (J.sy > gy ? J.sy - gy : gy - J.sy);
    n0.x = sc | (si << 16) | (RES ? startInf << 31 : 0u);  // RES: bit 31 = the start interval ends at INT_MAX
    n0.y = kNoParent;
    // SIPP::search(..., startTime) (sipp.hpp:92-103): the start node's g is startTime, its f is h(start) alone
    // (a_star.hpp:78 pushes Node(start, h, initialCost))
    const uint32_t startTime = (uint32_t)J.last_goal_constraint;
    n0.z = startTime;
    n0.w = 0;
    e0 = TierHbm::pack(0, h0, startTime, 0);
    uint32_t k, f0, n0c;
    tv.lookup(sc, k, f0, n0c);
    tv.putSt(tv.sid(sc, rfl(k), rfl(f0), si), 1);
  }
  int32_t rc = kSippNextTier;
  if constexpr (RES) {
    if (ldsTier) {
      // fast tier: nodes and open list in LDS (the table and the status words stay in HBM, one round trip per expansion)
      typedef TierLdsSipp TL;
      Mem<TL> gl = {};
      auto l8 = (__attribute__((address_space(3))) uint8_t*)ldsTier;
      gl.nodes = (Mem<TL>::PN32)l8;
      gl.pos = (Mem<TL>::P16)(l8 + (size_t)ldsNodes * 4);
      gl.gOf = (Mem<TL>::P16)(l8 + (size_t)ldsNodes * 6);
      gl.open = (Mem<TL>::PE)(l8 + (size_t)ldsNodes * 8 + 4);
      gl.capNodes = ldsNodes - 1;  // ids below kSippNoParentLds
      gl.capHeap = ldsNodes;
      sippNodeNew<TL>(gl, 0, n0.x, kNoParent, n0.z);
      gl.pos[0] = 0;
      gl.open[0] = TL::pack(0, TierHbm::f(e0), n0.z, 0);
      __syncthreads();
      const uint64_t tl0 = __builtin_amdgcn_s_memrealtime();
      rc = sippLoop<TL, RES>(P, J, gl, tv, s, res, outPath);
      res.prof[0] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);  // 100 MHz ticks / expansions in the LDS tier
      res.prof[1] = (uint32_t)s.expansions;
      if (rc == kSippNextTier) {
        __syncthreads();
        for (uint32_t i = lane; i < s.nNodes; i += 64) {
          const uint32_t w = gl.nodes[i];
          u32x4 nn;
          nn.x = sippUnpackX(w);
          nn.y = (w >> kSippXBits) == kSippNoParentLds ? kNoParent : (w >> kSippXBits);
          nn.z = gl.gOf[i];
          nn.w = gl.pos[i];
          gNodes[i] = nn;
        }
        // the open list: 64-bit entries with the node's x word (TierMix), staged through the arena's open array because
        // the new list covers the area the old one and the node records occupy
        for (uint32_t i = lane; i < s.nOpen; i += 64) {
          const uint32_t e = gl.open[i];
          const uint32_t w = gl.nodes[TL::id(e)];
          g.open[i] = TierMix::withX(TierHbm::pack(0, TL::f(e), TL::g(e), TL::id(e)), sippUnpackX(w));
        }
        __syncthreads();
        Mem<TierMix> gm = viewAs<TierMix>(g);  // the arena's node records, the open list in LDS
        gm.open = (Mem<TierMix>::PE)(l8 + 8);
        gm.capHeap = (kSippLdsBytes - 16) / 8;
        for (uint32_t i = lane; i < s.nOpen; i += 64) gm.open[i] = g.open[i];
        __syncthreads();
        res.tier = 2;  // started in LDS, the open list still there
        const uint64_t tm0 = __builtin_amdgcn_s_memrealtime();
        const int64_t e0m = s.expansions;
        rc = sippLoop<TierMix, RES>(P, J, gm, tv, s, res, outPath);
        res.prof[6] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tm0);  // ... in the middle tier
        res.prof[7] = (uint32_t)(s.expansions - e0m);
        if (rc == kSippNextTier) {  // the open list has outgrown LDS too: everything in the arena
          __syncthreads();
          for (uint32_t i = lane; i < s.nOpen; i += 64) g.open[i] = gm.open[i];
          __syncthreads();
          res.tier = 3;
        }
      } else {
        res.tier = 0;
      }
    } else {
      gNodes[0] = n0;
      g.open[0] = TierHbmX::withX(e0, n0.x);
    }
  } else {
    gNodes[0] = n0;
    g.open[0] = e0;
  }
  if (rc == kSippNextTier) {
    const uint64_t th0 = __builtin_amdgcn_s_memrealtime();
    const int64_t e0h = s.expansions;
    if constexpr (RES) {
      Mem<TierHbmX> gx = viewAs<TierHbmX>(g);
      rc = sippLoop<TierHbmX, RES>(P, J, gx, tv, s, res, outPath);
    } else {
      rc = sippLoop<TierHbm, RES>(P, J, g, tv, s, res, outPath);
    }
    res.prof[2] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - th0);  // ... in the arena tier
    res.prof[3] = (uint32_t)(s.expansions - e0h);
    if (res.tier == 0) res.tier = 1;
  }
  res.status = rc;
  res.expanded = s.expansions;
  res.nodes_created = s.nNodes;
  if constexpr (RES) {
    if (rc == ST_OK && (J.ctx_flags & kSippCommit)) {
      __syncthreads();
      if (!sippCommitPath(tv, (const uint32_t*)outPath, (uint32_t)res.n_states)) res.tier |= kSippTierCommitFailed;
    }
  }
}

// One SIPP job whose descriptor is at `jobSrc` (host memory): result + raw A* states back to host memory.
// `ldsTier` (sessions): kSippLdsCap node records + the open list, for jobs on device-resident tables.
DEVI void processSippJob(const LaunchParams& P, const DevJob* jobSrc, DevResult* resDst, uint16_t* pathDst,
                         uint8_t* arenaSlot, uint8_t* ldsTier, DevJob& jobS, DevResult& resS) {
  const uint32_t lane = threadIdx.x;
  DevResult res;
  beginJob<false>(jobSrc, jobS, res, 1);
  uint16_t* outPath = slot::outPath(arenaSlot, P.arena_scratch_off, P.out_stride);
  const uint64_t tj0 = __builtin_amdgcn_s_memrealtime();
  if (rfl(jobS.algo) == 2) {  // anything else stays ST_BAD
    if (rfl(jobS.ctx_flags) & kSippResident) {
      if (ldsTier)  // sessions only (else ST_BAD)
        runSipp<true>(P, jobS, arenaSlot, (rfl(jobS.ctx_flags) & kSippNoLds) ? nullptr : ldsTier, kSippLdsCap, res, outPath);
    } else {
      runSipp<false>(P, jobS, arenaSlot, nullptr, 0, res, outPath);
    }
  }
  res.prof[4] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tj0);  // the whole of runSipp (table update + search)
  res.prof[5] = 1;
  endJob(res, resS, resDst);
  if (res.status == ST_OK) {  // one u32 (cell | g << 16) per raw A* state
    const uint32_t* src = (const uint32_t*)outPath;
    uint32_t* dst = (uint32_t*)pathDst;
    for (uint32_t i = lane; i < (uint32_t)res.n_states; i += 64) hostStore32(dst + i, src[i]);
  }
}

}  // namespace mrp

#endif  // MRP_LL_SIPP_H
