// The assignment wave program of assign_wave.h for up to 256 agents x 256 tasks: the same method (shortest augmenting
// paths with 64-bit potentials, one agent inserted at a time, a private no-task column per free agent at the price
// 2^32), the same contract and result record, still ONE wavefront per problem with wave-uniform control flow.
//
// Lane l owns the task columns l + 64k and the agents l + 64k, k < C, C = wordsWide(nA, nT) in 1 .. 4: what is one lane
// word in the narrow program (dist, v, way, holder, u, rowDist, taskOf, mode) is an array of C here, and the scalar sets
// (taken, used, tree) are C 64-bit words.  The program is a template over C and every loop over k is unrolled, so the
// arrays are only ever indexed by constants and stay in registers; a wave-uniform index (the row being scanned, the
// column just reached) picks its word by a chain of scalar compares.
// Cost rows, by AssignJobWide::rowSource:
//   kRowsLds  the rows sit in LDS, 64C words apart (a lane's C reads stay on one bank each).  A forbidden pair is written
//             as "no edge" when the rows are filled, so the scan needs no mask of the row.
//   kRowsMem  the rows are an [nA][nT] word matrix in device memory, read coalesced: the staged cost words themselves
//             (matrix form), or a matrix the wave first writes into its scratch region of the result area, one table
//             load per (agent, column slot) (gather form).  The row's forbidden words are loaded beside its costs.
// Either way a forbidden pair is a pair without an edge — also for a forced pair, which is infeasible in both cases.
// Ties: among equally near columns the lowest COLUMN INDEX wins (word k first, then the lane), and a task column wins
// over a no-task end of the same price: with nA, nT <= 64 this is the narrow program's matching, entry for entry.
#pragma once
#include <stdint.h>

#include "assign_wave.h"

#if defined(__HIPCC__)
#define AS_UNROLL _Pragma("unroll")
#else
#define AS_UNROLL
#endif

namespace mrp {
namespace as {

// ---- a wave-uniform index into C lane words / C mask words ----
WV_FN uint64_t bitOfWord(uint32_t idx, uint32_t k) { return (idx >> 6) == k ? 1ull << (idx & 63u) : 0ull; }
template <uint32_t C>
WV_FN uint32_t readAt(const V (&a)[C], uint32_t idx) {
  uint32_t r = readlane(a[0], idx & 63u);
  AS_UNROLL
  for (uint32_t k = 1; k < C; ++k) {
    const uint32_t x = readlane(a[k], idx & 63u);
    r = (idx >> 6) == k ? x : r;
  }
  return r;
}
template <uint32_t C>
WV_FN void writeAt(V (&a)[C], uint32_t val, uint32_t idx) {
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k) a[k] = sel(laneMask(bitOfWord(idx, k)), splat(val), a[k]);
}
template <uint32_t C>
WV_FN int64_t dreadAt(const D (&a)[C], uint32_t idx) {
  int64_t r = dread(a[0], idx & 63u);
  AS_UNROLL
  for (uint32_t k = 1; k < C; ++k) {
    const int64_t x = dread(a[k], idx & 63u);
    r = (idx >> 6) == k ? x : r;
  }
  return r;
}
template <uint32_t C>
WV_FN void setBit(uint64_t (&m)[C], uint32_t idx) {
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k) m[k] |= bitOfWord(idx, k);
}
template <uint32_t C>
WV_FN bool testBit(const uint64_t (&m)[C], uint32_t idx) {
  uint64_t r = 0;
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k) r |= m[k] & bitOfWord(idx, k);
  return r != 0;
}
template <uint32_t C>
WV_FN uint32_t lowestBit(const uint64_t (&m)[C]) {  // kNone when empty
  uint32_t r = kNone;
  AS_UNROLL
  for (uint32_t k = C; k-- > 0;)
    if (m[k] != 0) r = 64u * k + lowestLane(m[k]);
  return r;
}
WV_FN V vmin(const V& a, const V& b) { return sel(a < b, a, b); }

template <uint32_t C>
WV_FN void assignSolveWide(Lds window, const uint32_t* maps, const uint32_t* data, uint32_t* out, const AssignJobWide job) {
  constexpr uint32_t kRowB = rowBytesWide(C), kRecWords = agentWordsWide(C);
  const Lds l = windowBase(window);
  const V lane = laneId();
  const B all = laneMask(~0ull);
  const uint32_t nA = job.nA, nT = job.nT;
  const bool ldsRows = job.rowSource == kRowsLds, gather = job.costOff == kNoCostOff;
  // memory rows: the matrix the scan reads (the wave's own stores, or the staged costs), and the records' forbidden words
  const uint32_t* rows = gather ? out + job.scratchOff : data + job.costOff;
  const uint32_t forbOff = job.agentOff + kAgentHeadWordsWide;

  V col[C], mode[C];
  B isAgent[C], isTask[C];
  uint64_t taskMask[C];
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k) {
    col[k] = lane + splat(64u * k);
    isAgent[k] = col[k] < splat(nA);
    isTask[k] = col[k] < splat(nT);
    taskMask[k] = ballot(isTask[k]);
    // lane l, word k: the record of agent l + 64k
    mode[k] = sel(isAgent[k], gLoad32m(data, splat(job.agentOff) + col[k] * splat(kRecWords), isAgent[k]), splat(kModeNoTask));
  }

  // the cost rows
  if (ldsRows || gather) {
    V tab[C], half[C];
    AS_UNROLL
    for (uint32_t k = 0; k < C; ++k) {
      tab[k] = gather ? gLoad32m(data, splat(job.taskOff) + col[k], isTask[k]) : splat(0u);
      half[k] = gather ? gLoad32m(data, splat(job.agentOff + 1u) + col[k] * splat(kRecWords), isAgent[k]) : splat(0u);
    }
    for (uint32_t a = 0; a < nA; ++a) {
      const uint32_t h = readAt(half, a);
      AS_UNROLL
      for (uint32_t k = 0; k < C; ++k) {
        V c;
        if (!gather) {
          c = gLoad32m(data, splat(job.costOff + a * nT) + col[k], isTask[k]);
        } else {
          // the halfword of the task's table at agent a's start cell; 0xFFFF (unreachable) is no edge (assign_wave.h)
          const V w = gLoad32m(maps, tab[k] + splat(h >> 1), isTask[k]);
          c = (w >> splat((h & 1u) << 4)) & splat(0xFFFFu);
          c = sel(c == splat(0xFFFFu), splat(kNoEdge), c);
        }
        if (ldsRows) {
          // column l + 64k is bit l of mask word k: bit l & 31 of the record's 32-bit word 2k + (l >> 5)
          const V fw = gLoad32m(data, splat(forbOff + a * kRecWords + 2u * k) + (lane >> splat(5u)), isTask[k]);
          const B forb = ((fw >> (lane & splat(31u))) & splat(1u)) != splat(0u);
          ldsStore32m(l, splat(a * kRowB) + (col[k] << splat(2u)), sel(forb, splat(kNoEdge), c), isTask[k]);
        } else {
          gStore32m(out, splat(job.scratchOff + a * nT) + col[k], c, isTask[k]);
        }
      }
    }
    sync();
  }
  // cost[i][t] as a scalar (t < nT), "no edge" where the pair is forbidden
  auto costAt = [&](uint32_t i, uint32_t t) -> uint32_t {
    if (ldsRows) return ldsLoadS(l, i * kRowB + 4u * t);
    const uint32_t c = first(gLoad32CoherentM(rows, splat(i * nT + t), all));
    const uint32_t fw = first(gLoad32m(data, splat(forbOff + i * kRecWords + (t >> 5)), all));
    return (fw >> (t & 31u) & 1u) != 0 ? kNoEdge : c;
  };

  bool ok = true;
  V holder[C], taskOf[C];  // lane l, word k: the agent that holds task l + 64k; the task of agent l + 64k
  uint64_t taken[C], rowsLeft[C];
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k) {
    holder[k] = splat(kNone);
    taskOf[k] = splat(kNone);
    taken[k] = 0;
    rowsLeft[k] = ballot(isAgent[k] & (mode[k] < splat(kMaxDimWide)));
  }

  // forced pairs leave the graph
  for (uint32_t i = lowestBit(rowsLeft); i != kNone && ok; i = lowestBit(rowsLeft)) {
    AS_UNROLL
    for (uint32_t k = 0; k < C; ++k) rowsLeft[k] &= ~bitOfWord(i, k);
    const uint32_t t = readAt(mode, i);
    const uint32_t c = t < nT ? costAt(i, t) : kNoEdge;
    if (c > kMaxCost || testBit(taken, t)) {
      ok = false;  // no such edge, forbidden, or two agents forced to one task
    } else {
      setBit(taken, t);
      writeAt(holder, i, t);
      writeAt(taskOf, t, i);
    }
  }

  D u[C], v[C];  // potentials: of agent l + 64k, of task l + 64k (a no-task column's stays 0)
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k) {
    u[k] = dsplat(0);
    v[k] = dsplat(0);
    rowsLeft[k] = ballot(isAgent[k] & ((mode[k] == splat(kModeFree)) | (mode[k] == splat(kModeSomeTask))));
  }
  for (uint32_t root = lowestBit(rowsLeft); root != kNone && ok; root = lowestBit(rowsLeft)) {
    D dist[C], rowDist[C];  // as in assign_wave.h, per owned column / agent
    V way[C];
    uint64_t used[C], tree[C];
    AS_UNROLL
    for (uint32_t k = 0; k < C; ++k) {
      rowsLeft[k] &= ~bitOfWord(root, k);
      dist[k] = dsplat(kInf);
      rowDist[k] = dsplat(0);
      way[k] = splat(kNone);
      used[k] = 0;
      tree[k] = 0;
    }
    int64_t bestEnd = kInf;
    uint32_t bestEndRow = kNone;
    uint32_t cur = root, endCol = kNone;
    int64_t curDist = 0, fin = 0;
    for (;;) {
      setBit(tree, cur);
      const int64_t uCur = dreadAt(u, cur);
      const D base = dsplat(curDist - uCur);
      AS_UNROLL
      for (uint32_t k = 0; k < C; ++k) {
        rowDist[k] = dsel(laneMask(bitOfWord(cur, k)), dsplat(curDist), rowDist[k]);
        const B open = laneMask(taskMask[k] & ~taken[k] & ~used[k]);
        V c;
        if (ldsRows) {
          c = ldsLoad32m(l, splat(cur * kRowB) + (col[k] << splat(2u)), open);
        } else {
          c = gLoad32CoherentM(rows, splat(cur * nT) + col[k], open);
          const V fw = gLoad32m(data, splat(forbOff + cur * kRecWords + 2u * k) + (lane >> splat(5u)), open);
          c = sel(((fw >> (lane & splat(31u))) & splat(1u)) != splat(0u), splat(kNoEdge), c);
        }
        const D nd = dsub(dadd(base, D{splat(0u), c}), v[k]);
        const B better = open & (c <= splat(kMaxCost)) & dless(nd, dist[k]);
        dist[k] = dsel(better, nd, dist[k]);
        way[k] = sel(better, splat(cur), way[k]);
      }
      if (readAt(mode, cur) == kModeFree) {
        const int64_t e = curDist + kNoTaskPrice - uCur;
        if (e < bestEnd) {
          bestEnd = e;
          bestEndRow = cur;
        }
      }
      // the nearest task outside the tree: each lane's nearest of its C columns first, then across the wave
      B outside[C];
      V hiMin = splat(0x7FFFFFFFu), loMin = splat(0xFFFFFFFFu);
      AS_UNROLL
      for (uint32_t k = 0; k < C; ++k) {
        outside[k] = laneMask(taskMask[k] & ~taken[k] & ~used[k]);
        hiMin = vmin(hiMin, sel(outside[k], dist[k].hi, splat(0x7FFFFFFFu)));
      }
      const uint32_t mh = waveMinU32(hiMin);
      AS_UNROLL
      for (uint32_t k = 0; k < C; ++k) {
        outside[k] = outside[k] & (dist[k].hi == splat(mh));
        loMin = vmin(loMin, sel(outside[k], dist[k].lo, splat(0xFFFFFFFFu)));
      }
      const uint32_t ml = waveMinU32(loMin);
      const int64_t colMin = (int64_t)((uint64_t)mh << 32 | (uint64_t)ml);
      if (colMin == kInf || bestEnd < colMin) {
        if (bestEnd == kInf) ok = false;  // an agent that must get a task cannot
        fin = bestEnd;
        break;
      }
      uint64_t nearest[C];  // the lowest column index among the equally near
      AS_UNROLL
      for (uint32_t k = 0; k < C; ++k) nearest[k] = ballot(outside[k] & (dist[k].lo == splat(ml)));
      const uint32_t j = lowestBit(nearest);
      setBit(used, j);
      curDist = colMin;
      const uint32_t h = readAt(holder, j);
      if (h == kNone) {
        fin = colMin;
        endCol = j;
        break;
      }
      cur = h;
    }
    if (!ok) break;
    AS_UNROLL
    for (uint32_t k = 0; k < C; ++k) {
      u[k] = dsel(laneMask(tree[k]), dadd(u[k], dsub(dsplat(fin), rowDist[k])), u[k]);
      v[k] = dsel(laneMask(used[k]), dsub(v[k], dsub(dsplat(fin), dist[k])), v[k]);
    }
    // augment: every agent on the path moves to the task it reached the next agent through
    uint32_t j = endCol;
    if (j == kNone) {  // bestEndRow gives its task up (the root has none)
      j = readAt(taskOf, bestEndRow);
      writeAt(taskOf, kNone, bestEndRow);
    }
    while (j != kNone) {
      const uint32_t i = readAt(way, j), next = readAt(taskOf, i);
      writeAt(taskOf, j, i);
      writeAt(holder, i, j);
      j = next;
    }
  }

  uint32_t matched = 0;
  uint64_t total = 0;
  if (ok) {
    AS_UNROLL
    for (uint32_t k = 0; k < C; ++k) {
      const B has = isAgent[k] & (taskOf[k] != splat(kNone));
      const V c = ldsRows ? ldsLoad32m(l, col[k] * splat(kRowB) + (taskOf[k] << splat(2u)), has)
                          : gLoad32CoherentM(rows, col[k] * splat(nT) + taskOf[k], has);
      for (uint64_t m = ballot(has); m != 0; m &= m - 1ull) {
        total += readlane(c, lowestLane(m));
        ++matched;
      }
    }
    if (matched < job.minMatching) ok = false;
  }
  if (!ok) {
    matched = 0;
    total = 0;
  }
  const V head = sel(lane == splat(0u), splat(ok ? kStatusSolved : kStatusInfeasible),
                     sel(lane == splat(1u), splat(matched),
                         sel(lane == splat(2u), splat((uint32_t)total), splat((uint32_t)(total >> 32)))));
  gStore32m(out, splat(job.outOff) + lane, head, lane < splat(kOutHeadWords));
  AS_UNROLL
  for (uint32_t k = 0; k < C; ++k)
    gStore32m(out, splat(job.outOff + kOutHeadWords) + col[k], ok ? taskOf[k] : splat(kNone), isAgent[k]);
}

// One problem, by its C.
WV_FN void assignSolveWideAny(Lds window, const uint32_t* maps, const uint32_t* data, uint32_t* out, const AssignJobWide& job) {
  switch (job.words) {
    case 1: assignSolveWide<1>(window, maps, data, out, job); break;
    case 2: assignSolveWide<2>(window, maps, data, out, job); break;
    case 3: assignSolveWide<3>(window, maps, data, out, job); break;
    default: assignSolveWide<4>(window, maps, data, out, job); break;
  }
}

}  // namespace as
}  // namespace mrp
