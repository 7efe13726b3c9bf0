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

template <uint32_t JOB_OFF, uint32_t OUT_OFF>
WV_ENTRY void nodeScan(Lds window) {
  const Lds l = windowBase(window);
  const uint32_t nAgents = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, nAgents));
  const uint32_t nPad = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, nPad));
  const uint32_t tPad = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, tPad));
  const uint32_t agentIdx = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, agentIdx));
  const uint32_t nStates = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, nStates));
  const uint32_t tabLds = ldsLoadS(l, JOB_OFF + (uint32_t)offsetof(NsJob, tabLds));
  const uint16_t* tabG = nsPtr<const uint16_t>(l, JOB_OFF + (uint32_t)offsetof(NsJob, tabG));
  const uint16_t* newPath = nsPtr<const uint16_t>(l, JOB_OFF + (uint32_t)offsetof(NsJob, newPath));
  const V lane = laneId();
  // a node of one agent has no pair to look at (and no table)
  const uint32_t longest = tPad > nStates ? tPad : nStates;
  const uint32_t T = (nAgents >= 2u && tPad >= 1u && nStates >= 1u) ? longest - 1u : 0u;
  const uint32_t nChunks = (nAgents + 63u) >> 6;
  const uint32_t ownChunk = agentIdx >> 6;
  const B ownLane = lane == splat(agentIdx & 63u);
  uint32_t count = 0, found = 0, fTime = 0, fType = 0, fPair = 0, fCell1 = 0, fCell2 = 0;
  V pathC = splat(0u), pathN = splat(0u);  // the new path at t = 64 k + lane and one step later
  for (uint32_t t = 0; t < T; ++t) {
    if ((t & 63u) == 0u) {
      const V tt = splat(t) + lane, last = splat(nStates - 1u);
      pathC = gLoadU16m(newPath, sel(tt < last, tt, last), bsplat(true));
      pathN = gLoadU16m(newPath, sel(tt + splat(1u) < last, tt + splat(1u), last), bsplat(true));
    }
    const uint32_t ownC = readlane(pathC, t & 63u), ownN = readlane(pathN, t & 63u);
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
    if (found == 0u && (firstV & firstE) != 0xFFFFFFFFu) {
      found = 1u;
      fTime = t;
      if (firstV != 0xFFFFFFFFu) {
        fType = 0u; fPair = firstV; fCell1 = cellV; fCell2 = 0u;
      } else {
        fType = 1u; fPair = firstE; fCell1 = cellE1; fCell2 = cellE2;
      }
    }
  }
  // mrp_ll_conflict: found, time, agent1, agent2, type, x1, y1, x2, y2, count (Edge: agent1's move, ecbs.cpp:439-445)
  ldsStoreS(l, OUT_OFF + 0u, found);
  ldsStoreS(l, OUT_OFF + 4u, fTime);
  ldsStoreS(l, OUT_OFF + 8u, fPair >> 16);
  ldsStoreS(l, OUT_OFF + 12u, fPair & 0xFFFFu);
  ldsStoreS(l, OUT_OFF + 16u, fType);
  ldsStoreS(l, OUT_OFF + 20u, found ? (fCell1 & 0xFFu) : 0u);
  ldsStoreS(l, OUT_OFF + 24u, found ? (fCell1 >> 8) : 0u);
  ldsStoreS(l, OUT_OFF + 28u, fType ? (fCell2 & 0xFFu) : 0u);
  ldsStoreS(l, OUT_OFF + 32u, fType ? (fCell2 >> 8) : 0u);
  ldsStoreS(l, OUT_OFF + 36u, count);
}

}  // namespace ns
}  // namespace mrp
