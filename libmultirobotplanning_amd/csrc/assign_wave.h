// Constrained min-cost task assignment as a wave program (vocabulary: wave_dev.h on the device,
// tests/support/wave_emu_assign.h on the host): ONE wavefront solves ONE problem — what Assignment::solve
// (assignment.hpp:81-118) and NextBestAssignment::constrainedMatching (next_best_assignment.hpp:129-189) compute with
// Boost's min-cost flow: a matching of maximum cardinality and, among those, of minimum total cost, under a node's
// constraints (forbidden pairs O, forced pairs I, agents that must stay without a task, agents that must get one).
//
// Method: shortest augmenting paths with potentials (the Hungarian method, one agent inserted at a time) over the columns
// "tasks + one private no-task column per free agent".  Lane t owns task column t (its potential, its distance, the agent
// that holds it); lane i also holds what belongs to agent i (its potential, its task, its constraint record).  The cost
// rows sit in LDS, 64 words apart: lane t reads cost[i][t] of the row being scanned, one bank per lane.  A no-task column
// is adjacent to its own agent only, so it is never an inner vertex of an augmenting path: it needs no lane, only the
// scalar "cheapest way to end this path by leaving some agent of the tree without a task".
// Numbers: the price of a no-task column is M = 2^32, above any sum of real costs (64 x (2^24 - 1) < 2^30), so that
// cardinality is maximised first.  Potentials reach 64 x M: distances and potentials are 64-BIT integers, a (high, low)
// pair of lane words with carry, signed in two's complement; distances themselves are never negative.
// A forced pair leaves the graph with its agent and its task, as in the reference; so does an agent that must stay
// without a task.  An agent that must get a task has no no-task column: when its path search finds nothing the problem
// is infeasible.
// Ties: the nearest column is the one of the lowest lane among equals and a task column wins over a no-task end of the
// same price, so the matching depends on the problem alone — the emulator and the device give the same one.
// Control flow is wave-uniform (scalars from ballots and lane reads only); integer work only, results are exact.
#pragma once
#include <stdint.h>

#include "assign_layout.h"

namespace mrp {
namespace as {

using namespace wv;

// (AssignJob, the staged records, the result record, ldsBytes: assign_layout.h, shared with the host)

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int64_t kInf = INT64_MAX;
constexpr int64_t kNoTaskPrice = (int64_t)1 << 32;

struct D {  // one signed 64-bit value per lane
  V hi, lo;
};
WV_FN D dsplat(int64_t s) { return D{splat((uint32_t)((uint64_t)s >> 32)), splat((uint32_t)(uint64_t)s)}; }
WV_FN D dadd(const D& a, const D& b) {
  const V lo = a.lo + b.lo;
  return D{a.hi + b.hi + sel(lo < a.lo, splat(1u), splat(0u)), lo};
}
WV_FN D dsub(const D& a, const D& b) { return D{a.hi - b.hi - sel(a.lo < b.lo, splat(1u), splat(0u)), a.lo - b.lo}; }
WV_FN B dless(const D& a, const D& b) { return (a.hi < b.hi) | ((a.hi == b.hi) & (a.lo < b.lo)); }  // neither negative
WV_FN D dsel(B c, const D& a, const D& b) { return D{sel(c, a.hi, b.hi), sel(c, a.lo, b.lo)}; }
WV_FN int64_t dread(const D& a, uint32_t lane) {
  return (int64_t)((uint64_t)readlane(a.hi, lane) << 32 | (uint64_t)readlane(a.lo, lane));
}
WV_FN uint32_t lowestLane(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }  // m != 0

WV_ENTRY void assignSolve(Lds window, const uint32_t* maps, const uint32_t* data, uint32_t* out, const AssignJob job) {
  const Lds l = windowBase(window);
  const V lane = laneId();
  const uint32_t nA = job.nA, nT = job.nT;
  const B isAgent = lane < splat(nA), isTask = lane < splat(nT);
  const uint64_t taskMask = nT >= 64u ? ~0ull : (1ull << nT) - 1ull;

  // lane i: the record of agent i
  const V rec = splat(job.agentOff) + lane * splat(kAgentWords);
  const V forbLo = gLoad32m(data, rec, isAgent), forbHi = gLoad32m(data, rec + splat(1u), isAgent);
  const V mode = sel(isAgent, gLoad32m(data, rec + splat(2u), isAgent), splat(kModeNoTask));

  // the cost rows
  const V col4 = lane << splat(2u);
  if (job.costOff != kNoCostOff) {
    for (uint32_t a = 0; a < nA; ++a)
      ldsStore32m(l, splat(a * kRowBytes) + col4, gLoad32m(data, splat(job.costOff + a * nT) + lane, isTask), isTask);
  } else {
    // cost[a][t] = the halfword of task t's table at agent a's start cell; 0xFFFF (unreachable) is no edge.  (A table
    // may start beyond 2^31 halfwords of the maps buffer: the word is addressed, the half taken by a shift.)
    const V tab = gLoad32m(data, splat(job.taskOff) + lane, isTask);
    const V half = gLoad32m(data, rec + splat(3u), isAgent);
    for (uint32_t a = 0; a < nA; ++a) {
      const uint32_t h = readlane(half, a);
      const V w = gLoad32m(maps, tab + splat(h >> 1), isTask);
      const V c = (w >> splat((h & 1u) << 4)) & splat(0xFFFFu);
      ldsStore32m(l, splat(a * kRowBytes) + col4, sel(c == splat(0xFFFFu), splat(kNoEdge), c), isTask);
    }
  }
  sync();

  bool ok = true;
  V holder = splat(kNone);  // lane t: the agent that holds task t
  V taskOf = splat(kNone);  // lane i: the task of agent i

  // forced pairs leave the graph
  uint64_t taken = 0;
  for (uint64_t fm = ballot(isAgent & (mode < splat(kMaxDim))); fm != 0 && ok; fm &= fm - 1ull) {
    const uint32_t i = lowestLane(fm), t = readlane(mode, i);
    const uint64_t forb = (uint64_t)readlane(forbHi, i) << 32 | (uint64_t)readlane(forbLo, i);
    const uint32_t c = t < nT ? ldsLoadS(l, i * kRowBytes + 4u * t) : kNoEdge;
    if (c > kMaxCost || ((forb | taken) >> t & 1ull) != 0) {
      ok = false;  // no such edge, forbidden, or two agents forced to one task
    } else {
      taken |= 1ull << t;
      holder = writelane(holder, i, t);
      taskOf = writelane(taskOf, t, i);
    }
  }

  D u = dsplat(0), v = dsplat(0);  // potentials: lane i of agent i, lane t of task t (a no-task column's stays 0)
  for (uint64_t rows = ballot(isAgent & ((mode == splat(kModeFree)) | (mode == splat(kModeSomeTask)))); rows != 0 && ok;
       rows &= rows - 1ull) {
    const uint32_t root = lowestLane(rows);
    D dist = dsplat(kInf);     // lane t: the shortest way found so far from the root to task t, in reduced costs
    D rowDist = dsplat(0);     // lane i: the distance at which agent i joined the tree
    V way = splat(kNone);      // lane t: the agent that way comes from
    uint64_t used = 0, tree = 0;
    int64_t bestEnd = kInf;    // the cheapest way to end by leaving an agent of the tree without a task ...
    uint32_t bestEndRow = kNone;  // ... and that agent
    uint32_t cur = root, endCol = kNone;
    int64_t curDist = 0, fin = 0;
    for (;;) {
      tree |= 1ull << cur;
      rowDist = dsel(lane == splat(cur), dsplat(curDist), rowDist);
      const int64_t uCur = dread(u, cur);
      const uint64_t forb = (uint64_t)readlane(forbHi, cur) << 32 | (uint64_t)readlane(forbLo, cur);
      const B open = laneMask(taskMask & ~forb & ~taken & ~used);
      const V c = ldsLoad32m(l, splat(cur * kRowBytes) + col4, open);
      const D nd = dsub(dadd(dsplat(curDist - uCur), D{splat(0u), c}), v);
      const B better = open & (c <= splat(kMaxCost)) & dless(nd, dist);
      dist = dsel(better, nd, dist);
      way = sel(better, splat(cur), way);
      if (readlane(mode, cur) == kModeFree) {
        const int64_t e = curDist + kNoTaskPrice - uCur;
        if (e < bestEnd) {
          bestEnd = e;
          bestEndRow = cur;
        }
      }
      // the nearest task outside the tree: the minimum of the high words, then of the low words among those
      const B outside = laneMask(taskMask & ~taken & ~used);
      const uint32_t mh = waveMinU32(sel(outside, dist.hi, splat(0x7FFFFFFFu)));
      const B atHigh = outside & (dist.hi == splat(mh));
      const uint32_t ml = waveMinU32(sel(atHigh, dist.lo, splat(0xFFFFFFFFu)));
      const int64_t colMin = (int64_t)((uint64_t)mh << 32 | (uint64_t)ml);
      if (colMin == kInf || bestEnd < colMin) {
        if (bestEnd == kInf) ok = false;  // an agent that must get a task cannot
        fin = bestEnd;
        break;
      }
      const uint32_t j = lowestLane(ballot(atHigh & (dist.lo == splat(ml))));
      used |= 1ull << j;
      curDist = colMin;
      const uint32_t h = readlane(holder, j);
      if (h == kNone) {
        fin = colMin;
        endCol = j;
        break;
      }
      cur = h;
    }
    if (!ok) break;
    u = dsel(laneMask(tree), dadd(u, dsub(dsplat(fin), rowDist)), u);
    v = dsel(laneMask(used), dsub(v, dsub(dsplat(fin), dist)), v);
    // augment: every agent on the path moves to the task it reached the next agent through
    uint32_t j = endCol;
    if (j == kNone) {  // bestEndRow gives its task up (the root has none)
      j = readlane(taskOf, bestEndRow);
      taskOf = writelane(taskOf, kNone, bestEndRow);
    }
    while (j != kNone) {
      const uint32_t i = readlane(way, j), next = readlane(taskOf, i);
      taskOf = writelane(taskOf, j, i);
      holder = writelane(holder, i, j);
      j = next;
    }
  }

  uint32_t matched = 0;
  uint64_t total = 0;
  if (ok) {
    const uint64_t has = ballot(isAgent & (taskOf != splat(kNone)));
    for (uint64_t m = has; m != 0; m &= m - 1ull) {
      const uint32_t i = lowestLane(m);
      total += ldsLoadS(l, i * kRowBytes + 4u * readlane(taskOf, i));
      ++matched;
    }
    if (matched < job.minMatching) ok = false;
  }
  if (!ok) {
    matched = 0;
    total = 0;
    taskOf = splat(kNone);
  }
  const V head = sel(lane == splat(0u), splat(ok ? kStatusSolved : kStatusInfeasible),
                     sel(lane == splat(1u), splat(matched),
                         sel(lane == splat(2u), splat((uint32_t)total), splat((uint32_t)(total >> 32)))));
  gStore32m(out, splat(job.outOff) + lane, head, lane < splat(kOutHeadWords));
  gStore32m(out, splat(job.outOff + kOutHeadWords) + lane, taskOf, isAgent);
}

}  // namespace as
}  // namespace mrp
