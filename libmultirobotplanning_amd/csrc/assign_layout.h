// What the host (mrp_ll_assign_batch, host/assign_pack.h) and the assignment wave program (assign_wave.h) agree on: the
// per-problem descriptor, the staged records it points at, the result record and the LDS one problem needs.  Plain C++,
// no wave vocabulary.
#pragma once
#include <stdint.h>

namespace mrp {
namespace as {

constexpr uint32_t kMaxDim = 64;               // agents and tasks per problem: one lane each
constexpr uint32_t kMaxCost = (1u << 24) - 1;  // 64 of them sum to less than 2^30
constexpr uint32_t kNoEdge = 0xFFFFFFFFu;      // what the LDS cost rows hold where there is no edge (anything > kMaxCost)
constexpr uint32_t kNoCostOff = 0xFFFFFFFFu;   // AssignJob::costOff of the gather form

// mode word of an agent record: a forced task (0 .. 63) or one of these (mrp_ll.h MRP_LL_ASSIGN_FREE / _NO_TASK / _SOME_TASK)
constexpr uint32_t kModeFree = 0xFFFFFFFFu, kModeNoTask = 0xFFFFFFFEu, kModeSomeTask = 0xFFFFFFFDu;

struct AssignJob {       // one problem; every offset counts words of the staged data area
  uint32_t nA, nT;       // 0 .. 64 each
  uint32_t minMatching;  // the required cardinality (0: none)
  uint32_t costOff;      // [nA][nT] cost words (> kMaxCost: no edge), or kNoCostOff: the rows are gathered from the tables
  uint32_t agentOff;     // [nA] agent records of kAgentWords words: forbidden mask (low, high), mode, start halfword
  uint32_t taskOff;      // gather form: [nT] word offsets of the tasks' heuristic tables inside the maps buffer
  uint32_t outOff;       // the result record, counted in words of the result area
  uint32_t pad;
};
constexpr uint32_t kAgentWords = 4;

// result record: status, pairs, cost (low, high), then task_of[nA] (0xFFFFFFFF = none)
constexpr uint32_t kOutHeadWords = 4;
constexpr uint32_t kStatusSolved = 0, kStatusInfeasible = 1;
constexpr uint32_t outWords(uint32_t nA) { return kOutHeadWords + nA; }

// The LDS window of one problem: its cost rows, 64 words apart (lane t reads cost[i][t] of the row being scanned: one
// bank per lane).  16 KB at 64 agents.
constexpr uint32_t kRowBytes = 4u * kMaxDim;
constexpr uint32_t ldsBytes(uint32_t nA) { return kRowBytes * (nA ? nA : 1u); }

}  // namespace as
}  // namespace mrp
