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

// ---- the wide form (assign_wave_wide.h, mrp_ll_assign_batch_w): up to 256 agents x 256 tasks ----
// Lane l owns the columns and the agents l + 64k, k < C, with C = wordsWide(nA, nT) in 1 .. 4.  The result record is the
// narrow one with up to 256 task_of entries.
constexpr uint32_t kMaxDimWide = 256;    // 256 x kMaxCost = 2^32 - 256: still below the no-task price 2^32
constexpr uint32_t kMaxWordsWide = 4;    // 64-bit mask words per agent
constexpr uint32_t kLdsBudgetWide = 64u * 1024u;  // the default budget of the LDS rows (MRP_LL_ASSIGN_LDS_BYTES lowers it)
constexpr uint32_t kRowsLds = 0, kRowsMem = 1;    // AssignJobWide::rowSource

struct AssignJobWide {   // one problem; offsets count words of the staged data area unless said otherwise
  uint32_t nA, nT;       // 0 .. 256 each
  uint32_t minMatching;
  uint32_t costOff;      // as AssignJob::costOff; with memory rows the program reads its rows from these words themselves
  uint32_t agentOff;     // [nA] agent records of agentWordsWide(words) words
  uint32_t taskOff;      // gather form: [nT] table offsets
  uint32_t outOff;       // the result record, in words of the result area
  uint32_t words;        // C
  uint32_t rowSource;    // kRowsLds: the cost rows sit in LDS, rowBytesWide(C) apart; kRowsMem: an [nA][nT] matrix in memory
  uint32_t scratchOff;   // gather form with memory rows: where the wave writes that matrix, in words of the result area
  uint32_t pad[2];
};
// agent record: mode, start halfword, then C forbidden mask words as (low, high) pairs
constexpr uint32_t kAgentHeadWordsWide = 2;
constexpr uint32_t agentWordsWide(uint32_t C) { return kAgentHeadWordsWide + 2u * C; }
constexpr uint32_t wordsWide(uint32_t nA, uint32_t nT) {
  return ((nA > nT ? nA : nT) + 63u) / 64u ? ((nA > nT ? nA : nT) + 63u) / 64u : 1u;
}
// An LDS row is 64C words, so the C reads of a lane (columns l + 64k) stay on the lane's own bank.
constexpr uint32_t rowBytesWide(uint32_t C) { return 256u * C; }
// The row source is a pure function of (nA, nT, budget): LDS rows when all nA of them fit the budget.
constexpr uint32_t rowSourceWide(uint32_t nA, uint32_t nT, uint32_t budget) {
  return nA * rowBytesWide(wordsWide(nA, nT)) <= budget ? kRowsLds : kRowsMem;
}
constexpr uint32_t ldsBytesWide(uint32_t nA, uint32_t nT, uint32_t budget) {
  return rowSourceWide(nA, nT, budget) == kRowsLds ? nA * rowBytesWide(wordsWide(nA, nT)) : 0u;
}
constexpr uint32_t scratchWordsWide(uint32_t nA, uint32_t nT, bool gather, uint32_t budget) {
  return gather && rowSourceWide(nA, nT, budget) == kRowsMem ? nA * nT : 0u;
}

}  // namespace as
}  // namespace mrp
