// TEST INFRASTRUCTURE — the conflict scan of a conflict-tree child FROM WHAT ITS PARENT'S SCAN ESTABLISHED
// (libmultirobotplanning_amd/csrc/ll_node_scan.h nodeScanFromParent, the code the gfx950 kernels run behind a search flagged
// MRP_LL_JOB_SCAN_FROM_PARENT) compiled against the host interpretation of its wave vocabulary and checked against the
// quadratic restatements of getFirstConflict / focalHeuristic in csrc/hl/grid_mapf.hpp, applied to the CHILD.
// A stand-alone program (tests/test_node_scan_parent_cpu.py builds it under the host sanitizers and runs it; never part of
// the product): prints "ok N".  Every array the program under test may read has exactly the size the device gives it, so an
// access outside the table, the new path or the replaced path's slot is a sanitizer report; accesses outside the LDS
// window are counted by the emulator.
// The node generators, the oracle's answer and the window layout are emu_node_scan.cpp's.
#define main emu_node_scan_main
#include "emu_node_scan.cpp"
#undef main

namespace {

struct Base {
  uint32_t parentCount, cleanBefore;
};

// One scan.  `old`: the replaced path as its path-store slot holds it; lenWord: the slot's length word (the old path's
// length when truthful).
Answer runFromParent(const Paths& child, uint32_t ag, const std::vector<uint16_t>& old, uint32_t lenWord, Base b, bool lds, int64_t& oob) {
  const uint32_t n = (uint32_t)child.size(), nPad = (n + 15u) & ~15u;
  uint32_t tPad = 0;
  for (uint32_t a = 0; a < n; ++a)
    if (a != ag) tPad = std::max<uint32_t>(tPad, (uint32_t)child[a].size());
  // exact sizes: no guard halfwords, the sanitizer watches the ends
  std::vector<uint16_t> table((size_t)tPad * nPad, 0xFFFFu);
  for (uint32_t a = 0; a < n; ++a) {
    if (a == ag) continue;
    for (uint32_t t = 0; t < tPad; ++t) table[(size_t)t * nPad + a] = child[a][t < child[a].size() ? t : child[a].size() - 1];
  }
  std::vector<uint16_t> path(child[ag]);
  // the slot: [length][cells ...], a whole number of words
  const uint32_t slotHalfs = ((uint32_t)old.size() + 1u + 1u) & ~1u;
  std::vector<uint32_t> slot(slotHalfs / 2u, 0xDDDDDDDDu);
  {
    uint16_t* h = reinterpret_cast<uint16_t*>(slot.data());
    h[0] = (uint16_t)lenWord;
    std::memcpy(h + 1, old.data(), old.size() * 2);
  }
  const uint32_t tabBytes = tPad * nPad * 2u;
  std::vector<uint8_t> mem(kTabOff + (lds ? tabBytes : 0u), 0xCD);
  if (lds && tabBytes) std::memcpy(mem.data() + kTabOff, table.data(), tabBytes);
  mrp::ns::NsJob job;
  std::memset(&job, 0, sizeof(job));
  job.nAgents = n; job.nPad = n >= 2 ? nPad : 0u; job.tPad = tPad; job.agentIdx = ag;
  job.nStates = (uint32_t)path.size();
  job.tabLds = lds ? kTabOff : mrp::ns::kTableInGlobal;
  job.tabG = lds ? 0ull : (uint64_t)(uintptr_t)table.data();
  job.newPath = (uint64_t)(uintptr_t)path.data();
  mrp::ns::NsBase base;
  std::memset(&base, 0, sizeof(base));
  base.oldSlot = (uint64_t)(uintptr_t)slot.data();
  base.oldCap = slotHalfs - 1u;
  base.parentCount = b.parentCount;
  base.cleanBefore = b.cleanBefore;
  static_assert(kJobOff + sizeof(mrp::ns::NsJob) + sizeof(mrp::ns::NsBase) <= kOutOff, "this program's window layout");
  constexpr uint32_t kBaseOff = kJobOff + sizeof(mrp::ns::NsJob);
  std::memcpy(mem.data() + kJobOff, &job, sizeof(job));
  std::memcpy(mem.data() + kBaseOff, &base, sizeof(base));
  wv::LdsWindow win{mem.data(), (uint32_t)mem.size(), 0, 0};
  mrp::ns::nodeScanFromParent<kJobOff, kOutOff, kBaseOff>(&win);
  oob += (int64_t)(win.oobReads + win.oobWrites);
  Answer a;
  std::memcpy(a.w, mem.data() + kOutOff, sizeof(a.w));
  return a;
}

uint16_t cellAt(const std::vector<uint16_t>& p, uint32_t t) { return p[t < p.size() ? t : p.size() - 1]; }

struct Seen {  // what the issue wants to have occurred at least once, each on the incremental path unless it says otherwise
  long runs = 0, fallbackLonger = 0, fallbackShorter = 0, countZero = 0, othersFirst = 0, ownBeforeLow = 0, ownBeforeHigh = 0,
       edgeFirst = 0, vertexAndEdge = 0, sharedLastCell = 0, untruthful = 0, bad = 0;
  int64_t oob = 0;
  void add(const Seen& q) {
    runs += q.runs; fallbackLonger += q.fallbackLonger; fallbackShorter += q.fallbackShorter; countZero += q.countZero;
    othersFirst += q.othersFirst; ownBeforeLow += q.ownBeforeLow; ownBeforeHigh += q.ownBeforeHigh; edgeFirst += q.edgeFirst;
    vertexAndEdge += q.vertexAndEdge; sharedLastCell += q.sharedLastCell; untruthful += q.untruthful; bad += q.bad; oob += q.oob;
  }
};

uint32_t horizon(const Paths& S, uint32_t ag, size_t lenOwn) {
  size_t tPad = 0;
  for (uint32_t a = 0; a < S.size(); ++a)
    if (a != ag) tPad = std::max(tPad, S[a].size());
  return S.size() >= 2 ? (uint32_t)std::max(tPad, lenOwn) - 1u : 0u;
}

// does time step t of S hold a vertex conflict / an edge conflict?
void kindsAt(const Paths& S, uint32_t t, bool& vertex, bool& edge) {
  vertex = edge = false;
  for (size_t i = 0; i < S.size(); ++i)
    for (size_t j = i + 1; j < S.size(); ++j) {
      if (cellAt(S[i], t) == cellAt(S[j], t)) vertex = true;
      if (cellAt(S[i], t) == cellAt(S[j], t + 1) && cellAt(S[i], t + 1) == cellAt(S[j], t)) edge = true;
    }
}

void report(const char* what, const Paths& S, uint32_t ag, Base b, bool lds, const Answer& got, const Answer& want) {
  std::fprintf(stderr, "%s: %zu agents, agent %u, parent_count %u, clean_before %u, table %s\n  got ", what, S.size(), ag,
               b.parentCount, b.cleanBefore, lds ? "in LDS" : "in memory");
  for (uint32_t k = 0; k < mrp::ns::kOutWords; ++k) std::fprintf(stderr, " %u", got.w[k]);
  std::fprintf(stderr, "\n  want");
  for (uint32_t k = 0; k < mrp::ns::kOutWords; ++k) std::fprintf(stderr, " %u", want.w[k]);
  std::fprintf(stderr, "\n");
}

// One parent node, one agent replaced by `fresh`: truthful bases at every clean_before the issue names, then untruthful ones.
void checkChild(const Paths& parent, const Answer& pe, uint32_t ag, const std::vector<uint16_t>& fresh, Seen& sn) {
  Paths child = parent;
  child[ag] = fresh;
  const Answer e = expected(child);
  const uint32_t tNew = horizon(child, ag, fresh.size()), tOld = horizon(parent, ag, parent[ag].size());
  const bool incremental = tNew == tOld && parent.size() >= 2;
  // clean_before: 0, the parent's first-conflict time, T when the parent has none
  uint32_t cbs[2] = {0u, pe.w[0] ? pe.w[1] : tNew};
  for (int q = 0; q < 2; ++q) {
    const Base b{pe.w[9], cbs[q]};
    for (int lds = 0; lds < 2; ++lds) {
      const Answer a = runFromParent(child, ag, parent[ag], (uint32_t)parent[ag].size(), b, lds != 0, sn.oob);
      sn.runs += 1;
      if (std::memcmp(a.w, e.w, sizeof(a.w)) != 0 && sn.bad++ < 5) report("mismatch", child, ag, b, lds != 0, a, e);
    }
    if (tNew > tOld) sn.fallbackLonger += 1;
    if (tNew < tOld) sn.fallbackShorter += 1;
    if (!incremental) continue;
    sn.countZero += e.w[9] == 0;
    if (e.w[0]) {
      const bool own = e.w[2] == ag || e.w[3] == ag;
      if (!own && e.w[1] >= b.cleanBefore && q == 1) sn.othersFirst += 1;
      if (own && e.w[1] < b.cleanBefore) (e.w[3] == ag ? sn.ownBeforeLow : sn.ownBeforeHigh) += 1;
      sn.edgeFirst += e.w[4] == 1;
      bool v, ed;
      kindsAt(child, e.w[1], v, ed);
      sn.vertexAndEdge += v && ed;
    }
    for (size_t i = 0; i < child.size() && q == 0; ++i)
      for (size_t j = i + 1; j < child.size(); ++j)
        if (i != ag && j != ag && child[i].back() == child[j].back() && std::max(child[i].size(), child[j].size()) <= tNew)
          sn.sharedLastCell += 1;  // both stand still on one cell at t = tNew - 1: a conflict beyond both ends
  }
  // untruthful inputs: the answer may be anything; the scan ends, stays inside the window and its arrays (the sanitizer and
  // the emulator's count say so), and reports a time below T
  const Base lies[4] = {{0u, 0u}, {pe.w[9] > 0 ? pe.w[9] - 1u : 0u, tNew + 5u}, {pe.w[9] / 2u, 0x7FFFFFFFu}, {0x7FFFFFFFu, tNew + 1u}};
  for (int q = 0; q < 4; ++q)
    for (int lds = 0; lds < 2; ++lds) {
      // (q == 3: the slot's length word lies as well — cut to what the slot holds)
      const Answer a = runFromParent(child, ag, parent[ag], q == 3 ? 0xFFFFu : (uint32_t)parent[ag].size(), lies[q], lds != 0, sn.oob);
      sn.untruthful += 1;
      const uint32_t tMax = std::max(tNew, 1u);
      if ((a.w[0] > 1u || (a.w[0] == 1u && a.w[1] >= tMax) || a.w[2] >= child.size() || a.w[3] >= child.size()) && sn.bad++ < 5)
        report("untruthful inputs, answer out of range", child, ag, lies[q], lds != 0, a, e);
    }
}

void shardParent(uint32_t seed, long nSmall, long nWide, Seen& sn) {
  std::mt19937 rng(seed);
  for (long s = 0; s < nSmall; ++s) {
    const int n = 1 + (int)(rng() % 12), dim = 2 + (int)(rng() % 5);
    Paths P(n);
    int lo = 13, hi = 0;
    for (int a = 0; a < n; ++a) {
      P[a] = walk(rng, dim, 1 + (int)(rng() % 12));
      lo = std::min<int>(lo, (int)P[a].size());
      hi = std::max<int>(hi, (int)P[a].size());
    }
    const Answer pe = expected(P);
    for (int ag = 0; ag < n; ++ag) {
      checkChild(P, pe, (uint32_t)ag, walk(rng, dim, (int)P[ag].size()), sn);       // same length: the same horizon
      checkChild(P, pe, (uint32_t)ag, walk(rng, dim, 1 + (int)(rng() % 12)), sn);   // any length
      checkChild(P, pe, (uint32_t)ag, walk(rng, dim, hi + 1 + (int)(rng() % 3)), sn);  // longer than every path
      checkChild(P, pe, (uint32_t)ag, walk(rng, dim, lo > 1 ? lo - 1 : 1), sn);     // no longer than any other path
    }
  }
  // two and three lane chunks: 65-130 agents, the replaced agent at 0, 63, 64 and last
  for (long s = 0; s < nWide; ++s) {
    const int n = 65 + (int)(rng() % 66), dim = 8 + (int)(rng() % 25);
    Paths P(n);
    for (int a = 0; a < n; ++a) P[a] = walk(rng, dim, 1 + (int)(rng() % 24));
    const int at[4] = {0, 63, 64, n - 1};
    for (int q = 0; q < 4; ++q) {
      if (q & 1) P[at[q]] = walk(rng, dim, 25 + (int)(rng() % 50));  // (also past one 64-step block of the paths)
      const Answer pe = expected(P);
      checkChild(P, pe, (uint32_t)at[q], walk(rng, dim, (int)P[at[q]].size()), sn);
      checkChild(P, pe, (uint32_t)at[q], walk(rng, dim, 1 + (int)(rng() % 24)), sn);
      checkChild(P, pe, (uint32_t)at[q], walk(rng, dim, 25 + (int)(rng() % 70)), sn);
    }
  }
}

}  // namespace

int main() {
  constexpr int kShards = 8;
  constexpr long kSmallPerShard = 250, kWidePerShard = 3;
  std::vector<Seen> part(kShards);
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int k = next.fetch_add(1); k < kShards; k = next.fetch_add(1)) shardParent(20241019u + (uint32_t)k, kSmallPerShard, kWidePerShard, part[k]);
  };
  const unsigned hw = std::thread::hardware_concurrency();
  std::vector<std::thread> pool;
  for (unsigned k = 1; k < std::min(8u, hw ? hw : 1u); ++k) pool.emplace_back(work);
  work();
  for (std::thread& th : pool) th.join();
  Seen sn;
  for (const Seen& q : part) sn.add(q);
  std::fprintf(stderr,
               "runs %ld, untruthful %ld; fallback longer %ld shorter %ld; count 0: %ld; others first: %ld; own before clean_before: "
               "j < a %ld, j > a %ld; edge first %ld; vertex and edge %ld; shared last cell %ld\n",
               sn.runs, sn.untruthful, sn.fallbackLonger, sn.fallbackShorter, sn.countZero, sn.othersFirst, sn.ownBeforeLow,
               sn.ownBeforeHigh, sn.edgeFirst, sn.vertexAndEdge, sn.sharedLastCell);
  const bool all = sn.fallbackLonger && sn.fallbackShorter && sn.countZero && sn.othersFirst && sn.ownBeforeLow && sn.ownBeforeHigh &&
                   sn.edgeFirst && sn.vertexAndEdge && sn.sharedLastCell && sn.untruthful;
  if (sn.bad != 0 || sn.oob != 0 || !all) {
    std::fprintf(stderr, "FAILED: %ld mismatches, %lld out-of-window LDS accesses, every case seen: %s\n", sn.bad, (long long)sn.oob,
                 all ? "yes" : "no");
    return 1;
  }
  std::printf("ok %ld scans, %ld with untruthful inputs\n", sn.runs, sn.untruthful);
  return 0;
}
