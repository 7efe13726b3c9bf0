// The conflicts of a conflict-tree child, found by the wavefront that ran the child's low-level search, as a wave program
// (vocabulary: wave_dev.h on the device, tests/support/wave_emu.h on the host):
//   Environment::getFirstConflict   example/ecbs.cpp:401-452
//   Environment::focalHeuristic     example/ecbs.cpp:315-350
// over the node's solution S: S[agentIdx] = the path the search just found (newPath, nStates cells), S[j] = column j of the
// search's focal table — the time-major table [tPad][nPad] of the other agents' cells (x | y << 8) whose row tPad - 1 repeats
// forever and whose longest path has exactly tPad cells (ll_jobs.h runJob builds it from the path store).  The answer is what
// conflict_kernel.hip gives for S, word for word: t = 0 .. max(tPad, nStates) - 2 ascending (the final time step is never
// checked), at one t every vertex pair before every edge pair, pairs (i, j), i < j, in lexicographic order; every agent
// holds its last cell beyond its end.
// nodeScan looks at every pair at every time step; nodeScanFromParent (below) gives the same ten words from what the
// caller knows of the parent node, with all-pairs work for a few time steps only.  Both share nsStepAllPairs.
// ONE wavefront does the whole scan: lanes are agents j, 64 at a time; a wave-uniform loop runs over i, whose cells come out
// of chunk i / 64's registers with a lane read, and one ballot tests 64 pairs.  The job is the NsJob at JOB_OFF of the
// window, the answer ten words (mrp_ll_conflict of include/mrp_ll.h) at OUT_OFF.  Control flow is wave-uniform (scalars from
// ballots and lane reads only); integer work only, results are exact.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mrp {
namespace ns {

using namespace wv;

constexpr uint32_t kTableInGlobal = 0xFFFFFFFFu;
constexpr uint32_t kOutWords = 10;

struct NsJob {             // at JOB_OFF of the window; pointers as two words
  uint32_t nAgents;        // agents of the node, >= 1
  uint32_t nPad, tPad;     // the table's row length and rows (tPad = the longest other path; unused when nAgents == 1)
  uint32_t agentIdx;       // the column the new path stands in for
  uint32_t nStates;        // cells of the new path, >= 1
  uint32_t tabLds;         // byte offset of the table inside the window, or kTableInGlobal: it is at tabG
  uint64_t tabG;           // const uint16_t*
  uint64_t newPath;        // const uint16_t*: x | y << 8 per time step
};

struct NsBase {            // at BASE_OFF of the window, for nodeScanFromParent only
  uint64_t oldSlot;        // const uint32_t*: the path-store slot of the REPLACED path: halfword 0 = its length, then its cells
  uint32_t oldCap;         // the most cells a slot holds (a longer length word is cut to this)
  uint32_t parentCount;    // the parent node's number of conflicts (the replaced path in place)
  uint32_t cleanBefore;    // the parent node has no conflict at any time step below this
  uint32_t pad_;
};

template <class T>
WV_FN T* nsPtr(Lds l, uint32_t off) {
  const uint64_t lo = ldsLoadS(l, off), hi = ldsLoadS(l, off + 4u);
  return (T*)(uintptr_t)(lo | (hi << 32));
}

// cells of agents 64 * chunk + lane in table row `row`; lanes without an agent read column 0 (never compared)
WV_FN V nsRow(Lds l, uint32_t tabLds, const uint16_t* tabG, uint32_t row, uint32_t nPad, V col, B in) {
  const V idx = splat(row * nPad) + sel(in, col, splat(0u));
  if (tabLds != kTableInGlobal) return ldsLoadU16(l, splat(tabLds) + (idx << splat(1u)));
  return gLoadU16m(tabG, idx, in);
}

// What both scans read of the job, and what follows from it.
struct NsNode {
  Lds l;
  uint32_t nAgents, nPad, tPad, agentIdx, nStates, tabLds;
  const uint16_t* tabG;
  const uint16_t* newPath;
  uint32_t T;              // time steps to look at: max(tPad, nStates) - 1; 0 for a node of one agent (no pair, no table)
  uint32_t nChunks, ownChunk;
  V lane;
  B ownLane;
};
template <uint32_t JOB_OFF>
WV_FN NsNode nsNode(Lds l) {
  NsNode n;
  n.l = l;
  n.nAgents = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, nAgents));
  n.nPad = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, nPad));
  n.tPad = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, tPad));
  n.agentIdx = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, agentIdx));
  n.nStates = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, nStates));
  n.tabLds = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, tabLds));
  n.tabG = nsPtr<const uint16_t>(l, JOB_OFF + (uint32_t)offsetof(NsJob, tabG));
  n.newPath = nsPtr<const uint16_t>(l, JOB_OFF + (uint32_t)offsetof(NsJob, newPath));
  const uint32_t longest = n.tPad > n.nStates ? n.tPad : n.nStates;
  n.T = (n.nAgents >= 2u && n.tPad >= 1u && n.nStates >= 1u) ? longest - 1u : 0u;
  n.nChunks = (n.nAgents + 63u) >> 6;
  n.ownChunk = n.agentIdx >> 6;
  n.lane = laneId();
  n.ownLane = n.lane == splat(n.agentIdx & 63u);
  return n;
}

// The new path at t = t0 + lane (cur) and one step later (nxt), held at its last cell beyond its end
WV_FN void nsNewPath(const NsNode& n, uint32_t t0, V& cur, V& nxt) {
  const V tt = splat(t0) + n.lane, last = splat(n.nStates - 1u);
  cur = gLoadU16m(n.newPath, sel(tt < last, tt, last), bsplat(true));
  nxt = gLoadU16m(n.newPath, sel(tt + splat(1u) < last, tt + splat(1u), last), bsplat(true));
}

// The answer: found, and for the first conflict its time, type (0 vertex, 1 edge), pair (i << 16 | j, i < j) and agent i's
// cell (vertex) or move (edge); count = all conflicts.
struct NsAnswer {
  uint32_t found, time, type, pair, cell1, cell2, count;
};
// mrp_ll_conflict: found, time, agent1, agent2, type, x1, y1, x2, y2, count (Edge: agent1's move, ecbs.cpp:439-445)
template <uint32_t OUT_OFF>
WV_FN void nsStore(Lds l, const NsAnswer& a) {
  ldsStoreS(l, OUT_OFF + 0u, a.found);
  ldsStoreS(l, OUT_OFF + 4u, a.time);
  ldsStoreS(l, OUT_OFF + 8u, a.pair >> 16);
  ldsStoreS(l, OUT_OFF + 12u, a.pair & 0xFFFFu);
  ldsStoreS(l, OUT_OFF + 16u, a.type);
  ldsStoreS(l, OUT_OFF + 20u, a.found ? (a.cell1 & 0xFFu) : 0u);
  ldsStoreS(l, OUT_OFF + 24u, a.found ? (a.cell1 >> 8) : 0u);
  ldsStoreS(l, OUT_OFF + 28u, a.type ? (a.cell2 & 0xFFu) : 0u);
  ldsStoreS(l, OUT_OFF + 32u, a.type ? (a.cell2 >> 8) : 0u);
  ldsStoreS(l, OUT_OFF + 36u, a.count);
}

// ALL pairs of the node at ONE time step t (ownC / ownN: the new path's cell at t and at t + 1): adds the step's conflicts to
// a.count and, while a.found == 0, takes the step's first conflict — every vertex pair before every edge pair, pairs (i, j),
// i < j, lexicographic.  Lanes are agents j; a wave-uniform loop runs over i, whose cells come out of chunk i / 64's
// registers with a lane read, and one ballot tests 64 pairs.
WV_FN void nsStepAllPairs(const NsNode& n, uint32_t t, uint32_t ownC, uint32_t ownN, NsAnswer& a) {
  const Lds l = n.l;
  const V lane = n.lane;
  const uint32_t nAgents = n.nAgents, nPad = n.nPad, tPad = n.tPad, tabLds = n.tabLds, nChunks = n.nChunks, ownChunk = n.ownChunk;
  const uint16_t* tabG = n.tabG;
  const B ownLane = n.ownLane;
  uint32_t count = 0;
  const uint32_t rowC = t < tPad ? t : tPad - 1u, rowN = t + 1u < tPad ? t + 1u : tPad - 1u;
  // this time step's first vertex / edge pair (i << 16 | j) and agent i's cells there
  uint32_t firstV = 0xFFFFFFFFu, firstE = 0xFFFFFFFFu, cellV = 0, cellE1 = 0, cellE2 = 0;
  for (uint32_t ci = 0; ci < nChunks; ++ci) {
    const V colI = lane + splat(ci << 6);
    const B inI = colI < splat(nAgents);
    V curI = nsRow(l, tabLds, tabG, rowC, nPad, colI, inI), nxtI = nsRow(l, tabLds, tabG, rowN, nPad, colI, inI);
    if (ci == ownChunk) {
      curI = sel(ownLane, splat(ownC), curI);
      nxtI = sel(ownLane, splat(ownN), nxtI);
    }
    const uint32_t iEnd = nAgents - (ci << 6) < 64u ? nAgents - (ci << 6) : 64u;
    for (uint32_t cj = ci; cj < nChunks; ++cj) {
      V curJ = curI, nxtJ = nxtI;
      B inJ = inI;
      if (cj != ci) {
        const V colJ = lane + splat(cj << 6);
        inJ = colJ < splat(nAgents);
        curJ = nsRow(l, tabLds, tabG, rowC, nPad, colJ, inJ);
        nxtJ = nsRow(l, tabLds, tabG, rowN, nPad, colJ, inJ);
        if (cj == ownChunk) {
          curJ = sel(ownLane, splat(ownC), curJ);
          nxtJ = sel(ownLane, splat(ownN), nxtJ);
        }
      }
      for (uint32_t il = 0; il < iEnd; ++il) {
        const uint32_t ic = readlane(curI, il), in = readlane(nxtI, il);
        const B pair = cj != ci ? inJ : (inJ & (lane > splat(il)));  // j > i
        const uint64_t vm = ballot(pair & (curJ == splat(ic)));
        const uint64_t em = ballot(pair & (curJ == splat(in)) & (nxtJ == splat(ic)));
        count += (uint32_t)__builtin_popcountll(vm) + (uint32_t)__builtin_popcountll(em);
        if (vm != 0) {
          const uint32_t k = (((ci << 6) + il) << 16) | ((cj << 6) + (uint32_t)__builtin_ctzll(vm));
          if (k < firstV) {
            firstV = k;
            cellV = ic;
          }
        }
        if (em != 0) {
          const uint32_t k = (((ci << 6) + il) << 16) | ((cj << 6) + (uint32_t)__builtin_ctzll(em));
          if (k < firstE) {
            firstE = k;
            cellE1 = ic;
            cellE2 = in;
          }
        }
      }
    }
  }
  a.count += count;
  if (a.found == 0u && (firstV & firstE) != 0xFFFFFFFFu) {
    a.found = 1u;
    a.time = t;
    if (firstV != 0xFFFFFFFFu) {
      a.type = 0u; a.pair = firstV; a.cell1 = cellV; a.cell2 = 0u;
    } else {
      a.type = 1u; a.pair = firstE; a.cell1 = cellE1; a.cell2 = cellE2;
    }
  }
}

// The whole node: every pair at every time step.
WV_FN NsAnswer nsScanAll(const NsNode& n) {
  NsAnswer a{0u, 0u, 0u, 0u, 0u, 0u, 0u};
  V pathC = splat(0u), pathN = splat(0u);  // the new path at t = 64 k + lane and one step later
  for (uint32_t t = 0; t < n.T; ++t) {
    if ((t & 63u) == 0u) nsNewPath(n, t, pathC, pathN);
    nsStepAllPairs(n, t, readlane(pathC, t & 63u), readlane(pathN, t & 63u), a);
  }
  return a;
}

template <uint32_t JOB_OFF, uint32_t OUT_OFF>
WV_ENTRY void nodeScan(Lds window) {
  const Lds l = windowBase(window);
  const NsNode n = nsNode<JOB_OFF>(l);
  nsStore<OUT_OFF>(l, nsScanAll(n));
}

// ---- the same answer from what the PARENT node's scan established --------------------------------------------------------
// A child differs from its parent in ONE path (agentIdx's: the replaced one is still in its path-store slot), and the caller
// knows two facts about the parent: its number of conflicts, and a time before which it has none (ct_solver.hpp keeps both:
// focalHeuristic, and the time of the conflict the parent was split on).  With
//   T_x = max(tPad, L_x) - 1,  C(p, T) = conflicts between path p and every other agent at t < T (grid_mapf.hpp conflictsOfAgent)
// the child's count is  parentCount - C(old, T) + C(new, T)  when T_new == T_old: two passes of T * ceil(N / 64) iterations,
// two ballots each, lanes = the other agents j.  When the horizons differ — the extra or missing steps count stationary
// agents that share a last cell — the whole node is scanned as nodeScan does it.
// The first conflict: none when the count is 0.  Below cleanBefore only pairs with agentIdx can conflict, so the first hit
// of the new-path pass is the answer if it lies there: at its time step vertex before edge, and the smallest j — pairs
// (j, a), j < a, come before pairs (a, j), j > a, and an edge conflict reports the move of the pair's FIRST agent.  From
// cleanBefore on, nsStepAllPairs looks at one time step after the other until one has a conflict.
// Untruthful parentCount / cleanBefore give a wrong answer and nothing else: every loop runs over t < T, every index is cut
// to its array (the table's rows, the two paths' lengths, oldCap).
WV_FN V nsOldCells(const uint32_t* slot, V tt, uint32_t lenOld) {  // the replaced path at time steps tt, held at its last cell
  const V last = splat(lenOld - 1u);
  const V h = sel(tt < last, tt, last) + splat(1u);  // halfword of the slot (0 is the length)
  const V w = gLoad32Coherent(slot, h >> splat(1u));
  return sel((h & splat(1u)) != splat(0u), w >> splat(16u), w & splat(0xFFFFu));
}

template <uint32_t JOB_OFF, uint32_t OUT_OFF, uint32_t BASE_OFF>
WV_ENTRY void nodeScanFromParent(Lds window) {
  const Lds l = windowBase(window);
  const NsNode n = nsNode<JOB_OFF>(l);
  const uint32_t* oldSlot = nsPtr<const uint32_t>(l, BASE_OFF + (uint32_t)offsetof(NsBase, oldSlot));
  const uint32_t oldCap = ldsLoadS(l, BASE_OFF + (uint32_t)offsetof(NsBase, oldCap));
  const uint32_t parentCount = ldsLoadS(l, BASE_OFF + (uint32_t)offsetof(NsBase, parentCount));
  uint32_t cleanBefore = ldsLoadS(l, BASE_OFF + (uint32_t)offsetof(NsBase, cleanBefore));
  const uint32_t T = n.T;
  uint32_t lenOld = 0;
  if (T != 0u) {
    lenOld = first(gLoad32Coherent(oldSlot, splat(0u))) & 0xFFFFu;
    if (lenOld > oldCap) lenOld = oldCap;
  }
  const uint32_t tOld = (n.tPad > lenOld ? n.tPad : lenOld) - 1u;
  if (T == 0u || lenOld == 0u || tOld != T) {  // (also: one agent, an empty slot)
    nsStore<OUT_OFF>(l, nsScanAll(n));
    return;
  }
  if (cleanBefore > T) cleanBefore = T;
  const V lane = n.lane;
  const uint32_t a = n.agentIdx;
  // C(old, T) and C(new, T); the new path's first hit: its time, type, partner and the new path's two cells there
  uint32_t cOld = 0, cNew = 0, hitT = 0xFFFFFFFFu, hitType = 0, hitJ = 0, hitC = 0, hitN = 0;
  V newC = splat(0u), newN = splat(0u), oldC = splat(0u), oldN = splat(0u);
  for (uint32_t t = 0; t < T; ++t) {
    if ((t & 63u) == 0u) {
      nsNewPath(n, t, newC, newN);
      oldC = nsOldCells(oldSlot, splat(t) + lane, lenOld);
      oldN = nsOldCells(oldSlot, splat(t + 1u) + lane, lenOld);
    }
    const uint32_t nc = readlane(newC, t & 63u), nn = readlane(newN, t & 63u);
    const uint32_t oc = readlane(oldC, t & 63u), on = readlane(oldN, t & 63u);
    const uint32_t rowC = t < n.tPad ? t : n.tPad - 1u, rowN = t + 1u < n.tPad ? t + 1u : n.tPad - 1u;
    uint32_t vJ = 0xFFFFFFFFu, eJ = 0xFFFFFFFFu;  // this step's smallest partner of a vertex / an edge hit of the new path
    for (uint32_t c = 0; c < n.nChunks; ++c) {
      const V col = lane + splat(c << 6);
      B in = col < splat(n.nAgents);
      if (c == n.ownChunk) in = in & !n.ownLane;
      const V cur = nsRow(l, n.tabLds, n.tabG, rowC, n.nPad, col, in), nxt = nsRow(l, n.tabLds, n.tabG, rowN, n.nPad, col, in);
      const uint64_t vmN = ballot(in & (cur == splat(nc))), emN = ballot(in & (cur == splat(nn)) & (nxt == splat(nc)));
      const uint64_t vmO = ballot(in & (cur == splat(oc))), emO = ballot(in & (cur == splat(on)) & (nxt == splat(oc)));
      cNew += (uint32_t)__builtin_popcountll(vmN) + (uint32_t)__builtin_popcountll(emN);
      cOld += (uint32_t)__builtin_popcountll(vmO) + (uint32_t)__builtin_popcountll(emO);
      if (vmN != 0 && vJ == 0xFFFFFFFFu) vJ = (c << 6) + (uint32_t)__builtin_ctzll(vmN);
      if (emN != 0 && eJ == 0xFFFFFFFFu) eJ = (c << 6) + (uint32_t)__builtin_ctzll(emN);
    }
    if (hitT == 0xFFFFFFFFu && (vJ & eJ) != 0xFFFFFFFFu) {
      hitT = t;
      hitType = vJ != 0xFFFFFFFFu ? 0u : 1u;
      hitJ = hitType ? eJ : vJ;
      hitC = nc;
      hitN = nn;
    }
  }
  NsAnswer ans{0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const uint32_t count = parentCount - cOld + cNew;
  if (count != 0u) {
    if (hitT < cleanBefore) {
      const bool jFirst = hitJ < a;  // the pair is (j, a): an edge conflict reports j's move, the new path's reversed
      ans.found = 1u;
      ans.time = hitT;
      ans.type = hitType;
      ans.pair = jFirst ? (hitJ << 16) | a : (a << 16) | hitJ;
      ans.cell1 = (hitType && jFirst) ? hitN : hitC;
      ans.cell2 = hitType ? (jFirst ? hitC : hitN) : 0u;
    } else {
      for (uint32_t t = cleanBefore; t < T && ans.found == 0u; ++t) {
        if (t == cleanBefore || (t & 63u) == 0u) nsNewPath(n, t & ~63u, newC, newN);
        nsStepAllPairs(n, t, readlane(newC, t & 63u), readlane(newN, t & 63u), ans);
      }
    }
  }
  ans.count = count;
  nsStore<OUT_OFF>(l, ans);
}

}  // namespace ns
}  // namespace mrp
