// The LDS tier of MRP_LL_ASTAR_EPS_TA: AStarEpsilon::search (a_star_epsilon.hpp:86-285) over the task-assignment
// Environment (example/ecbs_ta.cpp:283-445) as a wave program in ll_compact.h's vocabulary and window.  Semantics are those
// of ll_ta.h runJobTaEps, line for line; what differs is where the state lives.
//
// g != time here (a Wait at the goal is free), a state can be discovered again with a smaller g, and
// a_star_epsilon.hpp:254-269 is live — so a state is not its heap entry, as it is in compactSearch.  The encoding:
//   * entry   [31:23] 511 - focalH   [22:16] 127 - f   [15:10] g   [9:0] node id   — the Narrow entry with an id for the
//     cell; the same word in the open and in the focal list, so the popped focal entry names its open entry by id;
//   * node table: one halfword per node, t << 10 | cell (cell = y * 32 + x), 1024 of them behind the heuristic table in the
//     window's path area; 0xFFFF names no node, id 1023 is never given out (kEmpty and kFront carry it);
//   * the (time, cell) bitmap of the window holds "discovered" (obstacles: the obstacle row; vertex and edge constraints:
//     one key per lane), as in compactSearchTA;
//   * a discovered successor finds its id with two 16-byte reads per lane of the node table, then its open position with
//     the id scan openSet.erase uses (found = still open, with g and f in the entry; not found = closed), then its focal
//     position the same way;
//   * cameFrom: compactSearchTA's byte table in the arena slot, overwritten when a state is re-parented;
//   * the focal path table is read where runJobTaEps keeps it, in the arena slot's path area (CJob::pathsG); the task's
//     shortest-path table (CJob::bitsG names it: this instance's bitmap is in the window) is copied into the window.
//
// A node re-keyed while it sits in the focal list gets its entry rewritten where it lies and NOTHING is sifted: from then
// on the focal array need not be a heap, and every focal step must make exactly the comparisons boost's d_ary_heap makes
// on that array.  The steps used here do, for any array:
//   dualDescend   a node is on the hole's path iff every ancestor let the hole pass (larger child >= x) and turned towards
//                 it; each node's decision looks at its own two children and x alone — boost's siftdown, node by node;
//   dualSiftUp,   the stop is the FIRST ancestor that is not less than the element (ctz of the inverted ballot), not a
//   pushPairs     count of the ancestors that are less — boost's siftup; pushPairs is used with one focal push at a time
//                 (the ordered walk), where its second-chain fix-up does not run;
//   the band test of the ordered walk reads the open list only.
// The kept roots of compactSearch (MRP_CT_KEEP_TOPS) assume a heap and are not used: the roots are loaded.
// (The ordered walk is compactSearch's, restated here and not shared with it: that function's instruction stream and
// register allocation are what the benchmark measures, and stay what they are.)
//
// Limits (the search returns C_CAP_NODES, C_CAP_HORIZON or C_OVERFLOW and is run again, from the start, by the arena tier):
// 1023 node records, CJob::openCap open and focal entries — room for five more of each is asked in front of every expansion
// —, an expanded node at t <= CJob::maxT <= 61, f and h <= 124, focalH <= 511; maps up to 32 x 32, at most 64 vertex and
// 64 edge constraints and 128 agents in the focal context (the caller's tests: the keys and columns are one per lane).
#pragma once
#include "ll_compact.h"

namespace mrp {
namespace ct {

constexpr uint32_t kTeHeurBytes = 2048u, kTeNodeBytes = 2048u;
constexpr uint32_t oTeHeur = oPaths, oTeNodes = oPaths + kTeHeurBytes;
constexpr uint32_t kTePathBytes = kTeHeurBytes + kTeNodeBytes;  // what the tier needs of the window's path area
constexpr uint32_t kTeNodeCap = 1023u;                          // ids 0 .. 1022
constexpr uint32_t kTeFMax = Narrow::kFMax - 3u;                // 124: every real key is above kEmpty's
constexpr uint32_t kTeMaxAgents = 128u;
enum : int32_t { C_BAD = 5 };  // the focal list ran empty (w < 1): runJobTaEps's ST_BAD
static_assert(kTeNodeBytes == 2u * (kTeNodeCap + 1u) && Narrow::kGMax == 63u && Narrow::kMaxT == 61u, "one halfword per node: t <= 62 above the cell");
// What the job itself must satisfy to be tried here (one definition for the kernels and for the emulator's driver)
WV_FN bool taEpsJobFits(uint32_t dimx, uint32_t dimy, uint32_t nVc, uint32_t nEc, uint32_t nAgentsPad) {
  return dimx <= 32u && dimy <= 32u && nVc <= 64u && nEc <= 64u && nAgentsPad <= kTeMaxAgents;
}

// The job: CJob as compactSearchTA reads it, and
//   pathsG      the focal path table [tPad][nAgentsPad] (x | y << 8 halfwords, 0xFFFF nobody), nAgentsPad <= 128
//   bitsG       const uint16_t*: the task's shortest-path table [32][32]
//   rows        node records this search may use (<= kTeNodeCap)
//   openCap     entries of the open and of the focal list (<= kCap)
// MRP_CT_COUNTX 45: decrease-key events; 46: those that re-keyed a node sitting in the focal list.
WV_ENTRY int32_t compactSearchTaEps(Lds window) {
  constexpr uint32_t kFShift = Narrow::kFShift, kFhShift = Narrow::kFhShift, kFMax = Narrow::kFMax, kFhMax = Narrow::kFhMax;
  constexpr uint32_t kGMax = Narrow::kGMax, kMOAux = Narrow::kMOAux, kAuxCap = Narrow::kAuxCap, kAuxClamp = Narrow::kAuxClamp;
  const Lds lds = windowBase(window);
  const Sides S = makeSides();
  const Rows Rw = makeRows();
  const V lane = S.lane;
  const V hb = bothSides(S, oOpen + 4u, oFocal + 4u);  // side A = open list, side B = focal list
  const V km = bothSides(S, kMO, kMF);
  const V hbAux = splat(oAux + 4u), kmAux = splat(kMOAux);
  const uint32_t dimx = MRP_CT_JOB_U32(lds, dimx), dimy = MRP_CT_JOB_U32(lds, dimy);
  const uint32_t gx = MRP_CT_JOB_U32(lds, gx), gy = MRP_CT_JOB_U32(lds, gy);
  const uint32_t nEc = MRP_CT_JOB_U32(lds, nEc), nVc = MRP_CT_JOB_U32(lds, nVc);
  const uint32_t nAgentsPad = MRP_CT_JOB_U32(lds, nAgentsPad), tPad = MRP_CT_JOB_U32(lds, tPad);
  const bool noGoal = MRP_CT_JOB_U32(lds, taNoGoal) != 0u;
  int32_t status = C_NO_SOLUTION, cost = 0, fmin = 0, nStates = 0;
  uint32_t nOpen = 1, nFocal = 1, nodes = 1, expansions = 0;
  sync();  // the previous job's LDS reads are done; the CJob block is written
  {  // obstacle row (stride 32) as in compactSearch
    const uint32_t* obst = MRP_CT_JOB_PTR(const uint32_t, lds, obst);
    const uint32_t obstWords = MRP_CT_JOB_U32(lds, obstWords);
    const V y = S.l5;
    const V bitOff = y * dimx;
    const V wi = bitOff >> 5, sh = bitOff & 31u;
    const B rowIn = (y < dimy) & !S.isB;
    const V lo = gLoad32m(obst, wi, rowIn & (wi < obstWords));
    const V hi = gLoad32m(obst, wi + 1u, rowIn & ((wi + 1u) < obstWords));
    V w = sel(sh == 0u, lo, (lo >> sh) | (hi << (splat(32u) - sh)));
    const uint32_t colMask = dimx >= 32u ? 0xFFFFFFFFu : ((1u << dimx) - 1u);
    w = (w & colMask) | ~colMask;
    w = sel(rowIn, w, splat(0xFFFFFFFFu));
    ldsStore32m(lds, splat(oObst) + y * 4u, w, !S.isB);
  }
  // constraint keys, one per lane each: vertex t << 16 | y << 8 | x, edge t << 19 | (y * dimx + x) << 3 | k; they pass
  // through the window (the bitmap's area, zeroed below) so that the loop holds no register a vector-memory load is still
  // writing
  V vcReg = splat(0xFFFFFFFFu), ecReg = splat(0xFFFFFFFFu);
  {
    const uint32_t* vc = MRP_CT_JOB_PTR(const uint32_t, lds, vc);
    const uint32_t* ec = MRP_CT_JOB_PTR(const uint32_t, lds, ec);
    ldsStore32(lds, splat(oBits) + lane * 4u, sel(lane < nVc, gLoad32m(vc, lane, lane < nVc), splat(0xFFFFFFFFu)));
    ldsStore32(lds, splat(oBits + 256u) + lane * 4u, sel(lane < nEc, gLoad32m(ec, lane, lane < nEc), splat(0xFFFFFFFFu)));
    sync();
    vcReg = ldsLoad32(lds, splat(oBits) + lane * 4u);
    ecReg = ldsLoad32(lds, splat(oBits + 256u) + lane * 4u);
    sync();
  }
  {  // heaps and walk queue: every slot "no element"; bitmap: nothing discovered; node table: no node; the heuristic table
    const V4 none{splat(kEmpty), splat(kEmpty), splat(kEmpty), splat(kEmpty)};
    const V4 head{sel(lane == 0u, splat(kFront), splat(kEmpty)), splat(kEmpty), splat(kEmpty), splat(kEmpty)};
    const V4 zero{splat(0u), splat(0u), splat(0u), splat(0u)};
    const V4 ones{splat(0xFFFFFFFFu), splat(0xFFFFFFFFu), splat(0xFFFFFFFFu), splat(0xFFFFFFFFu)};
    ldsStore128(lds, splat(oOpen) + lane * 16u, head);
    ldsStore128(lds, splat(oFocal) + lane * 16u, head);
    ldsStore128(lds, splat(oAux) + lane * 16u, head);
    for (uint32_t g = 1; g < kGroups; ++g) {
      ldsStore128(lds, splat(oOpen + g * 1024u) + lane * 16u, none);
      ldsStore128(lds, splat(oFocal + g * 1024u) + lane * 16u, none);
    }
    ldsStore128m(lds, splat(oOpen + kGroups * 1024u), none, lane == 0u);
    ldsStore128m(lds, splat(oFocal + kGroups * 1024u), none, lane == 0u);
    for (uint32_t b = 1024u; b < kAuxBytes; b += 1024u) ldsStore128m(lds, splat(oAux + b) + lane * 16u, none, (lane * 16u + b) < kAuxBytes);
    for (uint32_t i = 0; i < kRows / 8u; ++i) ldsStore128(lds, splat(oBits + i * 1024u) + lane * 16u, zero);
    for (uint32_t i = 0; i < kTeNodeBytes / 1024u; ++i) ldsStore128(lds, splat(oTeNodes + i * 1024u) + lane * 16u, ones);
    if (!noGoal) {
      const uint32_t* heur = (const uint32_t*)MRP_CT_JOB_PTR(const uint16_t, lds, bitsG);
      for (uint32_t q = 0; q < kTeHeurBytes / 256u; ++q)
        ldsStore32(lds, splat(oTeHeur + q * 256u) + lane * 4u, gLoad32m(heur, splat(q * 64u) + lane, bsplat(true)));
    }
  }
  sync();
  const V dx = sel(lane == 1u, splat(0xFFFFFFFFu), sel(lane == 2u, splat(1u), sel(lane < 5u, splat(0u), splat(0x4000u))));
  const V dy = sel(lane == 3u, splat(1u), sel(lane == 4u, splat(0xFFFFFFFFu), splat(0u)));
  // focal context: one agent (column of the path table) per lane, two loads for up to 128; a lane beyond the row's end
  // looks at the row's last agent and is left out where the values are counted
  const B in0 = lane < nAgentsPad, in1 = (lane + 64u) < nAgentsPad;
  const V col0 = sel(in0, lane, splat(nAgentsPad ? nAgentsPad - 1u : 0u));
  const V col1 = sel(in1, lane + 64u, splat(nAgentsPad ? nAgentsPad - 1u : 0u));
  const uint16_t* pathsG = MRP_CT_JOB_PTR(const uint16_t, lds, pathsG);
  const int32_t lastGoal = (int32_t)MRP_CT_JOB_U32(lds, lastGoal);
  const float wBound = uintAsFloat(MRP_CT_JOB_U32(lds, w));
  const uint32_t maxExp = MRP_CT_JOB_U32(lds, maxExp), openCap = MRP_CT_JOB_U32(lds, openCap), maxT = MRP_CT_JOB_U32(lds, maxT);
  const uint32_t nodeCap = MRP_CT_JOB_U32(lds, rows);
  uint8_t* parentTab = MRP_CT_JOB_PTR(uint8_t, lds, parentTab);
  const uint32_t goalCell = gx | (gy << 5);
  int32_t bestF = 0;
  uint32_t evenHalf = 0;  // the node table's halfword of the last node with an even id (its odd neighbour completes the word)
  {
    const uint32_t sx = MRP_CT_JOB_U32(lds, sx), sy = MRP_CT_JOB_U32(lds, sy);
    const uint32_t sc = sx | (sy << 5);
    const uint32_t h0 = noGoal ? 0u : first(ldsLoadU16(lds, splat(oTeHeur + sc * 2u)));
    if (h0 > kTeFMax) status = C_CAP_HORIZON;  // (the start cannot reach its task at all, or not within this tier's f)
    bestF = (int32_t)h0;
    const uint32_t e0 = (kFhMax << kFhShift) | ((kFMax - (h0 & kFMax)) << kFShift);  // focalH 0, g 0, node 0
    ldsStoreS(lds, oOpen + 4u, e0);
    ldsStoreS(lds, oFocal + 4u, e0);
    evenHalf = sc;  // node 0: t = 0
    ldsStoreS(lds, oTeNodes, sc | 0xFFFF0000u);
  }
  sync();

  while (status == C_NO_SOLUTION) {
    if (nOpen == 0u) break;  // open list exhausted (a_star_epsilon.hpp:284)
    const V tops = ldsLoad32(lds, hb);  // lanes 0..31: open.top(), lanes 32..63: focal.top()
    const uint32_t topO = readlane(tops, 0);
    uint32_t curE = readlane(tops, 32);
    {  // a_star_epsilon.hpp:134-154: bestFScore follows open.top() (also down); the ordered walk only when it rose
      const int32_t fTop = (int32_t)(kFMax - ((topO >> kFShift) & kFMax));
      const int32_t oldBest = bestF;
      bestF = fTop;
      if (fTop > oldBest) {
        // every open node with old * w < f <= new * w joins the focal list, in the order of open.ordered_begin(): the walk of
        // compactSearch (a std::priority_queue over the open array: push = sift-up, pop = hole down to a leaf, then sift-up)
        const float lo = fmulRn((float)oldBest, wBound), hi = fmulRn((float)fTop, wBound);  // binary32, no contraction
        // skipped when no open node has an f inside the band (it changes the focal list only through those): f is an integer,
        // the band is f in [floor(lo) + 1, floor(hi)]; empty slots read as f = 127 or 0, never inside
        bool bandEmpty = true;
        {
          const int32_t fA = (int32_t)lo + 1, fBraw = (int32_t)hi;
          const int32_t fB = fBraw > (int32_t)kFMax - 1 ? (int32_t)kFMax - 1 : fBraw;
          if (fB >= fA) {
            const V base = splat(kFMax - (uint32_t)fB), span = splat((uint32_t)(fB - fA));
            for (uint32_t g = 0; g < kGroups && g * 256u <= nOpen; ++g) {
              const V4 grp = ldsLoad128(lds, splat(oOpen + g * 1024u) + lane * 16u);
              const B in = ((((grp.x >> kFShift) & kFMax) - base) <= span) | ((((grp.y >> kFShift) & kFMax) - base) <= span) |
                           ((((grp.z >> kFShift) & kFMax) - base) <= span) | ((((grp.w >> kFShift) & kFMax) - base) <= span);
              if (ballot(in)) {
                bandEmpty = false;
                break;
              }
            }
          }
        }
        if (!bandEmpty) {
          uint32_t npq = 0, npqHigh = 0;
          uint32_t cur = 0, curKey = topO & kMO, eCur = topO;  // the node being visited: open index, open key, entry
          // lanes 0, 1: the children of the node in the open array (past the end of the list: "no element"); lane 2: the node
          V trio = ldsLoad32(lds, splat(oOpen + 4u) + sel(lane == 2u, splat(cur), splat(2u * cur + 1u) + (lane & 1u)) * 4u);
          for (;;) {
            const uint32_t firstC = 2u * cur + 1u;
            const uint32_t nCh = firstC + 1u < nOpen ? 2u : firstC < nOpen ? 1u : 0u;
            if (npq + 2u > kAuxCap || nFocal >= kCap) {  // (a focal list never holds more than the open list: never overrun it)
              status = C_CAP_NODES;
              break;
            }
            const uint32_t e1 = readlane(trio, 0), e2 = readlane(trio, 1);
            const float fv = (float)(int32_t)(kFMax - ((curKey >> kFShift) & kFMax));
            const bool inBand = fv > lo && fv <= hi;
            // the children into the walk's queue (a heap), the node — if in the band — into the focal list: ONE focal push, whose
            // stop is the first ancestor that is not less than it
            pushPairs<false>(lds, Rw, oAux + 4u, kMOAux, npq, nCh, (e1 & kMO) | firstC, (e2 & kMO) | (firstC + 1u), oFocal + 4u, kMF,
                             nFocal, inBand ? 1u : 0u, eCur, 0u);
            npq += nCh;
            nFocal += inBand ? 1u : 0u;
            npqHigh = npq > npqHigh ? npq : npqHigh;
            if (fv > hi) break;
            if (npq == 0u) break;
            npq -= 1u;
            const V two = ldsLoad32(lds, splat(oAux + 4u) + sel(lane == 0u, splat(0u), splat(npq)) * 4u);
            ldsStoreS(lds, oAux + 4u + 4u * npq, kEmpty);
            uint32_t hole = 0, above = kFront;
            bool firstBlock = true;
            uint32_t value = 0;
            for (;;) {
              const V node = ((splat(hole) + 1u) << S.lvl) + S.off1;
              V c = node * 2u + 1u;
              c = sel(c < kAuxClamp, c, splat(kAuxClamp));
              const V2 pr = ldsLoad64(lds, splat(oAux + 4u) + c * 4u);
              if (firstBlock) {
                firstBlock = false;
                const uint32_t curA = readlane(two, 0);
                value = readlane(two, 1);
                cur = curA & Narrow::kAuxIdxMask;
                curKey = curA & kMO;
                trio = ldsLoad32(lds, splat(oOpen + 4u) + sel(lane == 2u, splat(cur), splat(2u * cur + 1u) + (lane & 1u)) * 4u);
                if (npq == 0u) break;
              }
              const V kl = pr.x & kMOAux, kr = pr.y & kMOAux;
              const B right = kr >= kl;
              const V pe = sel(right, pr.y, pr.x);
              const B go = kl > (kEmpty & kMOAux);
              const uint32_t goM = lo32(ballot(go)), rM = lo32(ballot(right));
              const B onPath = ((S.anc & goM) == S.anc) & (((S.needR ^ rM) & S.anc) == 0u) & go;
              const uint32_t pm = lo32(ballot(onPath & !S.isB));
              ldsStore32m(lds, splat(oAux + 4u) + node * 4u, pe, onPath);
              if (pm == 0u) break;
              const uint32_t steps = (uint32_t)__builtin_popcount(pm), d = lg2(pm);
              hole = ((hole + 1u) << steps) + 2u * d + 1u + ((rM >> d) & 1u) - (1u << steps);
              above = readlane(pe, d);
              if (steps < 5u) break;
            }
            eCur = readlane(trio, 2);
            if (npq > 0u) {
              if (hole == 0u || !((above & kMOAux) < (value & kMOAux)))
                ldsStoreS(lds, oAux + 4u + 4u * hole, value);
              else
                dualSiftUp<false>(lds, S, hbAux, kmAux, splat(hole + 1u), value, false, false);
            }
          }
          for (uint32_t b = 0; b <= 4u * npqHigh; b += 1024u) {  // what the walk leaves in its queue is dropped
            const V4 none{splat(kEmpty), splat(kEmpty), splat(kEmpty), splat(kEmpty)};
            const V4 head{sel(lane == 0u, splat(kFront), splat(kEmpty)), splat(kEmpty), splat(kEmpty), splat(kEmpty)};
            ldsStore128m(lds, splat(oAux + b) + lane * 16u, b == 0u ? head : none, (lane * 16u + b) < kAuxBytes);
          }
          if (status != C_NO_SOLUTION) break;
          curE = ldsLoadS(lds, oFocal + 4u);
        }
      }
    }
    if (nFocal == 0u) {  // (w < 1: the reference reads the top of an empty heap here)
      status = C_BAD;
      break;
    }
    // focalSet.top(): g, f, focalH as they are NOW (re-keyed in place); time and cell from the node table
    const uint32_t curId = curE & 1023u, g = (curE >> 10) & kGMax, curFh = kFhMax - (curE >> kFhShift);
    const uint32_t tc = first(ldsLoadU16(lds, splat(oTeNodes + curId * 2u)));
    const uint32_t cell = tc & 1023u, t = tc >> 10;
    const uint32_t x = cell & 31u, y = cell >> 5;
    const bool atGoal = noGoal || cell == goalCell;
    expansions += 1u;  // onExpandNode (a_star_epsilon.hpp:193) — counts the goal pop too
    if (expansions > maxExp) {
      status = C_CAP_EXP;
      break;
    }
    if (atGoal && (int32_t)t > lastGoal) {  // isSolution (ecbs_ta.cpp:384-390) -> a_star_epsilon.hpp:195-213
      status = C_OK;
      cost = (int32_t)g;
      fmin = (int32_t)(kFMax - ((topO >> kFShift) & kFMax));  // openSet.top().fScore (a_star_epsilon.hpp:210)
      nStates = (int32_t)t + 1;
      uint16_t* outPath = MRP_CT_JOB_PTR(uint16_t, lds, outPath);
      sync();  // this wave's action stores have left the CU
      uint32_t c = cell;
      const uint32_t* tab32 = (const uint32_t*)parentTab;
      for (int32_t k0 = (int32_t)t; k0 >= 1; k0 -= 8) {  // eight rows of the cameFrom table per round trip, as compactSearchTA
        V rowW[8][4];
        for (int32_t r = 0; r < 8; ++r)
          for (uint32_t q = 0; q < 4; ++q)
            rowW[r][q] = (k0 - r >= 1) ? gLoad32Coherent(tab32, splat((uint32_t)(k0 - r) * 256u + q * 64u) + lane) : splat(0u);
        for (int32_t r = 0; r < 8; ++r)
          for (uint32_t q = 0; q < 4; ++q) ldsStore32(lds, splat(oBits + (uint32_t)r * 1024u + q * 256u) + lane * 4u, rowW[r][q]);
        sync();
        for (int32_t r = 0; r < 8 && k0 - r >= 1; ++r) {
          gStoreU16m(outPath, splat((uint32_t)(k0 - r)), splat((c & 31u) | ((c >> 5) << 8)), lane == 0u);
          const uint32_t a = first(ldsLoadU8(lds, splat(oBits + (uint32_t)r * 1024u + c)));
          c = a == 1u ? c + 1u : a == 2u ? c - 1u : a == 3u ? c - 32u : a == 4u ? c + 32u : c;
        }
        sync();
      }
      gStoreU16m(outPath, splat(0u), splat((c & 31u) | ((c >> 5) << 8)), lane == 0u);
      break;
    }
    // the tier's limits, in front of everything this expansion would touch (the expansion is not counted)
    if (t > maxT) {
      expansions -= 1u;
      status = C_CAP_HORIZON;
      break;
    }
    if (nodes + 5u > nodeCap || nOpen + 5u > openCap || nFocal + 5u > openCap) {
      expansions -= 1u;
      status = C_CAP_NODES;
      break;
    }
    // getNeighbors (ecbs_ta.cpp:392-438): the five probes on lanes 0..4, requested before the pops
    const uint32_t t1 = t + 1u;
    const V nx = splat(x) + dx, ny = splat(y) + dy;
    const B inb = (nx < dimx) & (ny < dimy);
    const V ncell = (nx & 31u) | ((ny & 31u) << 5);
    const V obstW = ldsLoad32(lds, splat(oObst) + ((ny & 31u) << 2));
    const V wordAddr = splat(oBits + t1 * kRowBytes) + ((ny & 31u) << 2);
    const V seenW = ldsLoad32(lds, wordAddr);
    const V hN = noGoal ? splat(0u) : ldsLoadU16(lds, splat(oTeHeur) + ncell * 2u);
    // other agents' cells at t (a) and t + 1 (b); rows beyond the table repeat its last one
    V a0 = splat(0xFFFFu), b0 = splat(0xFFFFu), a1 = splat(0xFFFFu), b1 = splat(0xFFFFu);
    if (nAgentsPad) {
      const uint32_t ra = t < tPad ? t : tPad - 1u;
      const uint32_t rb = t1 < tPad ? t1 : tPad - 1u;
      a0 = gLoadU16(pathsG, splat(ra * nAgentsPad) + col0);
      b0 = gLoadU16(pathsG, splat(rb * nAgentsPad) + col0);
      if (nAgentsPad > 64u) {
        a1 = gLoadU16(pathsG, splat(ra * nAgentsPad) + col1);
        b1 = gLoadU16(pathsG, splat(rb * nAgentsPad) + col1);
      }
    }
    // ---- a_star_epsilon.hpp:215-216: focalSet.pop(), openSet.erase(handle of the same node)
    {
      const uint32_t nOld = nOpen;
      nOpen -= 1u;
      nFocal -= 1u;
      const V lastAddr = hb + bothSides(S, nOpen, nFocal) * 4u;  // the elements that pop() moves to the roots: the last ones
      const V lastV = ldsLoad32(lds, lastAddr);
      uint32_t p = 0;
      if (((curE ^ topO) & 1023u) != 0u) {  // where is the popped node in the open array?  Lane L looks at elements 4L - 1 .. 4L + 2
        const V key = splat(curId);
        for (uint32_t grp = 0; grp < kGroups && grp * 256u <= nOld; ++grp) {
          const V4 q = ldsLoad128(lds, splat(oOpen + grp * 1024u) + lane * 16u);
          const B m0 = (q.x & 1023u) == key, m1 = (q.y & 1023u) == key, m2 = (q.z & 1023u) == key, m3 = (q.w & 1023u) == key;
          const uint64_t any = ballot(m0 | m1 | m2 | m3);
          if (any) {
            const V pos = lane * 4u + sel(m0, splat(0xFFFFFFFFu), sel(m1, splat(0u), sel(m2, splat(1u), splat(2u))));
            p = grp * 256u + readlane(pos, ctz64(any));
            break;
          }
        }
      }
      uint32_t lastO = readlane(lastV, 0);
      const uint32_t lastF = readlane(lastV, 32);
      ldsStore32(lds, lastAddr, splat(kEmpty));  // the vacated slots: "no element" (every lane of a side names its side's slot)
      if (p != 0u) {  // boost erase = bubble to the root (every ancestor of p moves down one level), then pop
        const uint32_t depth = lg2(p + 1u);
        const B act = (!S.isB) & (S.l5 < depth);
        const V ancPos = (splat(p + 1u) >> (S.l5 + 1u)) - 1u;
        const V ae = ldsLoad32(lds, splat(oOpen + 4u) + ancPos * 4u);
        ldsStoreSel(lds, splat(oOpen + 4u) + ((splat(p + 1u) >> S.l5) - 1u) * 4u, ae, act);
        // ... which has just overwritten the last element if the erased node WAS the last one: it is the node's parent then,
        // and the slot it sat in is vacated after all
        if (p == nOld - 1u) {
          lastO = readlane(ae, 0);
          ldsStoreS(lds, oOpen + 4u + 4u * p, kEmpty);
        }
      }
      const V xk = bothSides(S, lastO & kMO, lastF & kMF);
      const V xe = bothSides(S, lastO, lastF);
      const B some = bothSides(S, nOpen, nFocal) != 0u;
      const V hole = dualDescend(lds, S, hb, km, splat(kHeapClamp), xk);
      ldsStoreSel(lds, hb + hole * 4u, xe, some);
    }
    uint32_t mask = lo32(ballot(inb & (((obstW >> (nx & 31u)) & 1u) == 0u))) & 0x1Fu;
    const V nxy = (nx & 0xFFu) | ((ny & 0xFFu) << 8);
    if (nVc) {  // stateValid (ecbs_ta.cpp:483-489)
      const V nkey = nxy | (t1 << 16);
      for (uint32_t mm = mask; mm; mm &= mm - 1u) {
        const uint32_t k = ctz32(mm);
        if (ballot(vcReg == readlane(nkey, k))) mask &= ~(1u << k);
      }
    }
    if (nEc) {  // transitionValid (ecbs_ta.cpp:491-496)
      const uint32_t base = (t << 19) | ((y * dimx + x) << 3);
      const V d = ecReg - base;
      if (ballot(d < 5u))
        for (uint32_t k = 0; k < 5u; ++k)
          if (ballot(d == k)) mask &= ~(1u << k);
    }
    const uint32_t seenMask = lo32(ballot(((seenW >> (nx & 31u)) & 1u) != 0u));
    const float bound = fmulRn((float)bestF, wBound);  // bestFScore * m_w (a_star_epsilon.hpp:240,265), binary32
    const uint32_t curXy = x | (y << 8);
    const uint64_t valid0 = ballot(in0), valid1 = ballot(in1);
    const uint64_t swap0 = ballot(b0 == curXy) & valid0, swap1 = ballot(b1 == curXy) & valid1;
    for (uint32_t mm = mask; mm; mm &= mm - 1u) {  // a_star_epsilon.hpp:223-281, neighbour by neighbour
      const uint32_t k = ctz32(mm);
      const uint32_t nc = readlane(ncell, k);
      const uint32_t g2 = g + ((k == 0u && atGoal) ? 0u : 1u);  // tentative_gScore (:225)
      const uint32_t tcN = (t1 << 10) | nc;
      if (!((seenMask >> k) & 1u)) {  // a new node (:227-247)
        const uint32_t h = readlane(hN, k);
        const uint32_t f2 = g2 + h;
        if (h > kTeFMax || f2 > kTeFMax) {
          status = C_CAP_HORIZON;
          break;
        }
        // focalStateHeuristic + focalTransitionHeuristic (ecbs_ta.cpp:314-344): an agent counts once if it stands on the
        // successor's cell at time t + 1 and once more if it is there at t and on this node's cell at t + 1 (a Wait too)
        uint32_t fh = curFh;
        if (nAgentsPad) {
          const uint32_t cc = readlane(nxy, k);
          fh += popc64(ballot(b0 == cc) & valid0) + popc64(ballot(a0 == cc) & swap0);
          if (nAgentsPad > 64u) fh += popc64(ballot(b1 == cc) & valid1) + popc64(ballot(a1 == cc) & swap1);
        }
        if (fh > kFhMax) {
          status = C_OVERFLOW;
          break;
        }
        const uint32_t nid = nodes++;
        if (nid & 1u) {
          ldsStoreS(lds, oTeNodes + (nid - 1u) * 2u, evenHalf | (tcN << 16));
        } else {
          evenHalf = tcN;
          ldsStoreS(lds, oTeNodes + nid * 2u, tcN | 0xFFFF0000u);
        }
        ldsOr32m(lds, wordAddr, splat(1u) << (nx & 31u), lane == k);
        gStore8m(parentTab, splat(tcN), splat(k), lane == 0u);
        const uint32_t e = ((kFhMax - fh) << kFhShift) | ((kFMax - f2) << kFShift) | (g2 << 10) | nid;
        const bool inFocal = (float)(int32_t)f2 <= bound;  // focalSet.push (:240-243)
        dualSiftUp(lds, S, hb, km, bothSides(S, nOpen + 1u, inFocal ? nFocal + 1u : 1u), e, false, !inFocal);  // openSet.push (:237)
        nOpen += 1u;
        nFocal += inFocal ? 1u : 0u;
        continue;
      }
      // discovered before (:248-270): its id from the node table, eight halfwords per lane and read
      uint32_t nid = 0xFFFFFFFFu;
      for (uint32_t grp = 0; grp < kTeNodeBytes / 1024u && grp * 512u < nodes; ++grp) {
        const V4 q = ldsLoad128(lds, splat(oTeNodes + grp * 1024u) + lane * 16u);
        const V key = splat(tcN);
        const B m0 = (q.x & 0xFFFFu) == key, m1 = (q.x >> 16) == key, m2 = (q.y & 0xFFFFu) == key, m3 = (q.y >> 16) == key;
        const B m4 = (q.z & 0xFFFFu) == key, m5 = (q.z >> 16) == key, m6 = (q.w & 0xFFFFu) == key, m7 = (q.w >> 16) == key;
        const uint64_t any = ballot(m0 | m1 | m2 | m3 | m4 | m5 | m6 | m7);
        if (any) {
          const V idx = sel(m0, splat(0u), sel(m1, splat(1u), sel(m2, splat(2u), sel(m3, splat(3u), sel(m4, splat(4u), sel(m5, splat(5u), sel(m6, splat(6u), splat(7u))))))));
          nid = grp * 512u + ctz64(any) * 8u + readlane(idx, ctz64(any));
          break;
        }
      }
      // still in the open list (then its entry says with which g, f and focalH), or closed (:224)
      uint32_t p = 0xFFFFFFFFu, eOld = 0;
      for (uint32_t grp = 0; grp < kGroups && grp * 256u <= nOpen; ++grp) {  // (element 256 grp - 1 belongs to group grp)
        const V4 q = ldsLoad128(lds, splat(oOpen + grp * 1024u) + lane * 16u);
        const V key = splat(nid);  // (no node: no entry carries an id above 1023)
        const B m0 = (q.x & 1023u) == key, m1 = (q.y & 1023u) == key, m2 = (q.z & 1023u) == key, m3 = (q.w & 1023u) == key;
        const uint64_t any = ballot(m0 | m1 | m2 | m3);
        if (any) {
          const uint32_t l = ctz64(any);
          const V pos = lane * 4u + sel(m0, splat(0xFFFFFFFFu), sel(m1, splat(0u), sel(m2, splat(1u), splat(2u))));
          const V ent = sel(m0, q.x, sel(m1, q.y, sel(m2, q.z, q.w)));
          p = grp * 256u + readlane(pos, l);
          eOld = readlane(ent, l);
          break;
        }
      }
      if (p == 0xFFFFFFFFu) continue;  // closed
      const uint32_t gOld = (eOld >> 10) & kGMax;
      if (g2 >= gOld) continue;        // not an improvement (:251-253)
      MRP_CT_COUNTX(45, 1u);
      const uint32_t fOld = kFMax - ((eOld >> kFShift) & kFMax);
      const uint32_t fNew = fOld - (gOld - g2);                    // fScore -= delta (:256-257)
      gStore8m(parentTab, splat(tcN), splat(k), lane == 0u);       // cameFrom is replaced (:275-279)
      const uint32_t e = (eOld & (kFhMax << kFhShift)) | ((kFMax - fNew) << kFShift) | (g2 << 10) | nid;  // focalH keeps its value
      uint32_t fpos = 0xFFFFFFFFu;
      for (uint32_t grp = 0; grp < kGroups && grp * 256u <= nFocal; ++grp) {
        const V4 q = ldsLoad128(lds, splat(oFocal + grp * 1024u) + lane * 16u);
        const V key = splat(nid);
        const B m0 = (q.x & 1023u) == key, m1 = (q.y & 1023u) == key, m2 = (q.z & 1023u) == key, m3 = (q.w & 1023u) == key;
        const uint64_t any = ballot(m0 | m1 | m2 | m3);
        if (any) {
          const V pos = lane * 4u + sel(m0, splat(0xFFFFFFFFu), sel(m1, splat(0u), sel(m2, splat(1u), splat(2u))));
          fpos = grp * 256u + readlane(pos, ctz64(any));
          break;
        }
      }
      // not in the focal list: pushed iff its f crossed the bound (:265-269)
      const bool cross = fpos == 0xFFFFFFFFu && (float)(int32_t)fNew <= bound && (float)(int32_t)fOld > bound;
      dualSiftUp(lds, S, hb, km, bothSides(S, p + 1u, cross ? nFocal + 1u : 1u), e, false, !cross);  // openSet.increase(handle) (:262)
      nFocal += cross ? 1u : 0u;
      if (fpos != 0xFFFFFFFFu) {
        // already in the focal list: its entry reads the new f and g where it lies; the array is not repaired
        MRP_CT_COUNTX(46, 1u);
        ldsStoreS(lds, oFocal + 4u + 4u * fpos, e);
      }
    }
  }
  ldsStoreS(lds, oRes + (uint32_t)offsetof(CRes, status), (uint32_t)status);
  ldsStoreS(lds, oRes + (uint32_t)offsetof(CRes, cost), (uint32_t)cost);
  ldsStoreS(lds, oRes + (uint32_t)offsetof(CRes, fmin), (uint32_t)fmin);
  ldsStoreS(lds, oRes + (uint32_t)offsetof(CRes, nStates), (uint32_t)nStates);
  ldsStoreS(lds, oRes + (uint32_t)offsetof(CRes, expanded), expansions);
  ldsStoreS(lds, oRes + (uint32_t)offsetof(CRes, nodes), nodes);
  sync();
  MRP_CT_DONE(lds);
  return status;
}

}  // namespace ct
}  // namespace mrp
