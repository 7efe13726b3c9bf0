// Safe-interval tables on the host (MRP_LL_SIPP): collision intervals -> safe intervals, and the incrementally maintained
// mrp_ll_sipp_table with what a job that comes back reports to it.  HIP-free; included by ll_pack.h.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../../include/mrp_ll.h"
#include "../ll_device.h"

namespace mrp {
namespace host {

// SIPP job tables (see runSipp in ll_sipp.h).  Safe intervals are derived from the collision intervals exactly as
// SIPPEnvironment::setCollisionIntervals does (sipp.hpp:245-284): sort by start; a safe interval [start, ci.start-1]
// in front of every collision interval when non-empty; a final [start, INT_MAX] unless the last one ends at INT_MAX.
struct SippScratch {  // reused across jobs of a context: packSipp allocates nothing in the steady state
  struct Iv { int32_t s, e; };
  std::vector<int32_t> cellIdx;            // cell -> special index + 1
  std::vector<uint32_t> first, count;      // per special cell: block of safe intervals inside `pool`
  std::vector<Iv> pool, ci;
};

// setCollisionIntervals for one location (sipp.hpp:245-284): collision intervals sorted by start -> safe intervals
// appended to `out`.  `scratch` holds the sorted copy.
static inline void safeFromCollisions(const int32_t* civ, int cnt, std::vector<SippScratch::Iv>& scratch,
                                      std::vector<SippScratch::Iv>& out) {
  typedef SippScratch::Iv Iv;
  scratch.clear();
  bool sorted = true;
  for (int k = 0; k < cnt; ++k) {
    scratch.push_back(Iv{civ[2 * k], civ[2 * k + 1]});
    if (k && scratch[k].s < scratch[k - 1].s) sorted = false;
  }
  if (!sorted) std::stable_sort(scratch.begin(), scratch.end(), [](const Iv& a, const Iv& b) { return a.s < b.s; });
  long long start = 0;
  int32_t lastEnd = 0;
  for (const Iv& c : scratch) {
    if (start <= static_cast<long long>(c.s) - 1) out.push_back(Iv{static_cast<int32_t>(start), c.s - 1});
    start = static_cast<long long>(c.e) + 1;
    lastEnd = c.e;
  }
  if (lastEnd < INT32_MAX) out.push_back(Iv{static_cast<int32_t>(start), INT32_MAX});
}

}  // namespace host
}  // namespace mrp

// Incrementally maintained safe-interval table of one agent-planning context (include/mrp_ll.h, mrp_ll_sipp_table_*):
// what SIPP::setCollisionIntervals would hold after the same calls, kept per cell so that adding one collision interval
// recomputes one cell's list, and a job only has to be COPIED into its slot instead of being rebuilt from every
// collision interval of the instance.
struct mrp_ll_sipp_table {
  typedef mrp::host::SippScratch::Iv Iv;
  int32_t mapId = -1, dimx = 0, dimy = 0;
  std::vector<int32_t> cellIdx;                       // cell -> special index + 1
  std::vector<uint16_t> cellIdx16;                    // the same as the device reads it
  struct Spec {
    std::vector<int32_t> collisions;                  // [n][2] in the order they were added
    std::vector<Iv> safe;
    bool disjoint = true;                             // no two collision intervals of the cell have overlapped so far
  };
  std::vector<Spec> spec;
  uint32_t totalSafe = 0;
  std::vector<Iv> scratch;
  // device-resident copy (session mode): the jobs carry only the cells that changed since the previous job
  void* owner = nullptr;                              // the engine that created the table (PackEnv::owner)
  int32_t devIndex = -1;                              // slot in the engine's table pool (-1: none)
  bool devFresh = true;                               // the device copy has never been written: the next job resets it
  bool inFlight = false;                              // a job is using (and writing) the device copy
  uint32_t epoch = 0;                                 // of the last job (status words of other epochs read as unseen)
  bool overflow = false;                              // some cell has more than kSippCap safe intervals: ship whole tables
  std::vector<int32_t> dirty;                         // cells changed since the last job was packed
  std::vector<uint8_t> isDirty;
  // sipp_commit: stays (cell, start, end) the DEVICE copy already holds and this host copy does not yet; replayed
  // (sippTableSync) before anything reads the host copy
  std::vector<int32_t> log;
};

namespace mrp {
namespace host {

static inline void sippTableAddCell(mrp_ll_sipp_table* t, size_t cell, int32_t start, int32_t end, bool markDirty) {
  typedef SippScratch::Iv Iv;
  if (!t->cellIdx[cell]) {
    t->spec.emplace_back();
    t->cellIdx[cell] = static_cast<int32_t>(t->spec.size());
    t->cellIdx16[cell] = static_cast<uint16_t>(t->spec.size());
  }
  mrp_ll_sipp_table::Spec& sp = t->spec[t->cellIdx[cell] - 1];
  const bool first = sp.collisions.empty();
  sp.collisions.push_back(start);
  sp.collisions.push_back(end);
  t->totalSafe -= static_cast<uint32_t>(sp.safe.size());
  // The usual case (a planner adds the stays of a path that avoided every earlier one): the new collision interval lies
  // inside ONE safe interval, and sorting it into the list splits exactly that gap — [a, start - 1] if non-empty and
  // [end + 1, b] if non-empty — which is what setCollisionIntervals' loop (sipp.hpp:258-277) yields for the longer list.
  // Anything else (overlaps, start > end) recomputes the cell from all its collision intervals, as before.
  bool split = false;
  if (first) sp.safe.assign(1, Iv{0, INT32_MAX});
  if (sp.disjoint && start <= end && start >= 0) {
    for (size_t k = 0; k < sp.safe.size(); ++k) {
      const Iv g = sp.safe[k];
      if (g.s <= start && end <= g.e) {
        const bool left = g.s <= start - 1, right = end < g.e;
        if (left && right) {
          sp.safe[k].e = start - 1;
          sp.safe.insert(sp.safe.begin() + k + 1, Iv{end + 1, g.e});
        } else if (left) {
          sp.safe[k].e = start - 1;
        } else if (right) {
          sp.safe[k].s = end + 1;
        } else {
          sp.safe.erase(sp.safe.begin() + k);
        }
        split = true;
        break;
      }
    }
  }
  if (!split) {
    sp.disjoint = false;
    sp.safe.clear();
    safeFromCollisions(sp.collisions.data(), static_cast<int>(sp.collisions.size() / 2), t->scratch, sp.safe);
  }
  t->totalSafe += static_cast<uint32_t>(sp.safe.size());
  // what the resident layout cannot hold — more than kSippCap intervals on a cell, a finite bound that does not fit a
  // halfword: from now on this table travels whole (packSippFromTable)
  if (sp.safe.size() > kSippCap) t->overflow = true;
  for (const Iv& v : sp.safe)
    if (v.s < 0 || v.s >= static_cast<int32_t>(kSippEndInf) || (v.e != INT32_MAX && (v.e < 0 || v.e >= static_cast<int32_t>(kSippEndInf))))
      t->overflow = true;
  if (markDirty && !t->isDirty[cell]) {
    t->isDirty[cell] = 1;
    t->dirty.push_back(static_cast<int32_t>(cell));
  }
}
static inline void sippTableSync(mrp_ll_sipp_table* t) {
  for (size_t k = 0; k + 2 < t->log.size(); k += 3)
    sippTableAddCell(t, static_cast<size_t>(t->log[k]), t->log[k + 1], t->log[k + 2], false);
  t->log.clear();
}
// the stays of a raw solution (cell | arrival << 16 per state): one collision interval per state (mrp_ll.h, sipp_commit)
template <class F>
static inline void forEachStay(const uint32_t* raw, int n, F&& f) {
  for (int k = 0; k < n; ++k)
    f(static_cast<int32_t>(raw[k] & 0xFFFFu), static_cast<int32_t>(raw[k] >> 16),
      k + 1 < n ? static_cast<int32_t>(raw[k + 1] >> 16) - 1 : INT32_MAX);
}
// A job on an mrp_ll_sipp_table has come back.  flags: bit 0 = it ran on the device-resident copy, bit 1 = sipp_commit.
static inline void finishSippTableJob(mrp_ll_sipp_table* T, uint32_t flags, const DevResult& d, const uint16_t* rawPath) {
  if (flags & 1u) T->inFlight = false;
  if (!(flags & 2u) || d.status != ST_OK) return;
  const uint32_t* raw = reinterpret_cast<const uint32_t*>(rawPath);
  if (flags & 1u) {
    // the workgroup has already put the stays into the device copy; this copy catches up when somebody needs it
    forEachStay(raw, d.n_states, [&](int32_t cell, int32_t s0, int32_t e0) {
      T->log.push_back(cell);
      T->log.push_back(s0);
      T->log.push_back(e0);
    });
    if (d.tier & kSippTierCommitFailed) {  // ... unless a stay did not fit the fixed layout: redo the table here,
      sippTableSync(T);                    // and from now on it travels whole
      T->overflow = true;
      T->devFresh = true;
    }
  } else {
    if (!T->log.empty()) sippTableSync(T);
    forEachStay(raw, d.n_states, [&](int32_t cell, int32_t s0, int32_t e0) { sippTableAddCell(T, cell, s0, e0, true); });
  }
}

}  // namespace host
}  // namespace mrp
