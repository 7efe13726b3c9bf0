// TEST INFRASTRUCTURE — the conflict scan of a conflict-tree child (libmultirobotplanning_amd/csrc/ll_node_scan.h, the code
// the gfx950 kernels run behind a flagged search) compiled against the host interpretation of its wave vocabulary and
// checked against the quadratic restatements of getFirstConflict / focalHeuristic in csrc/hl/grid_mapf.hpp.
// A stand-alone program (tests/test_node_scan_cpu.py builds and runs it; never part of the product): prints "ok N".
#include <stdint.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "wave_emu.h"
#include "../../libmultirobotplanning_amd/csrc/ll_node_scan.h"
#include "../../libmultirobotplanning_amd/csrc/hl/grid_mapf.hpp"

namespace {

constexpr uint32_t kJobOff = 256, kOutOff = 384, kTabOff = 448;  // this program's own window layout
constexpr uint32_t kGuard = 64;                                  // halfwords of guard around every global array

struct Answer {
  uint32_t w[mrp::ns::kOutWords];
};

typedef std::vector<std::vector<uint16_t>> Paths;  // per agent: x | y << 8 per time step

// The table runJob builds for the search of agent `ag` (every other agent's cells, held beyond its end; kEmptyCell in the
// searching agent's column and in the padding), in the window (lds = true) or in "device memory", then the scan.
Answer runScan(const Paths& S, uint32_t ag, bool lds, int64_t& oob) {
  const uint32_t n = (uint32_t)S.size(), nPad = (n + 15u) & ~15u;
  uint32_t tPad = 0;
  for (uint32_t a = 0; a < n; ++a)
    if (a != ag) tPad = std::max<uint32_t>(tPad, (uint32_t)S[a].size());
  std::vector<uint16_t> table(kGuard + (size_t)tPad * nPad + kGuard, 0xFFFFu);
  for (uint32_t a = 0; a < n; ++a) {
    if (a == ag) continue;
    for (uint32_t t = 0; t < tPad; ++t) table[kGuard + (size_t)t * nPad + a] = S[a][t < S[a].size() ? t : S[a].size() - 1];
  }
  std::vector<uint16_t> path(kGuard + S[ag].size() + kGuard, 0xEEEEu);
  std::memcpy(path.data() + kGuard, S[ag].data(), S[ag].size() * 2);
  const uint32_t tabBytes = tPad * nPad * 2u;
  std::vector<uint8_t> mem(kTabOff + (lds ? tabBytes : 0u), 0xCD);
  if (lds && tabBytes) std::memcpy(mem.data() + kTabOff, table.data() + kGuard, tabBytes);
  mrp::ns::NsJob job;
  std::memset(&job, 0, sizeof(job));
  job.nAgents = n; job.nPad = n >= 2 ? nPad : 0u; job.tPad = tPad; job.agentIdx = ag;
  job.nStates = (uint32_t)S[ag].size();
  job.tabLds = lds ? kTabOff : mrp::ns::kTableInGlobal;
  job.tabG = lds ? 0ull : (uint64_t)(uintptr_t)(table.data() + kGuard);
  job.newPath = (uint64_t)(uintptr_t)(path.data() + kGuard);
  std::memcpy(mem.data() + kJobOff, &job, sizeof(job));
  wv::LdsWindow win{mem.data(), (uint32_t)mem.size(), 0, 0};
  mrp::ns::nodeScan<kJobOff, kOutOff>(&win);
  oob += (int64_t)(win.oobReads + win.oobWrites);
  Answer a;
  std::memcpy(a.w, mem.data() + kOutOff, sizeof(a.w));
  return a;
}

Answer expected(const Paths& S) {
  using namespace mrp_hl;
  PathVec sol;
  sol.assign(S.size(), PathPtr());
  for (size_t a = 0; a < S.size(); ++a) {
    auto p = std::make_shared<Path>();
    for (uint16_t c : S[a]) {
      p->xy.push_back(c & 0xFF);
      p->xy.push_back(c >> 8);
    }
    sol.set(a, p);
  }
  std::vector<int32_t> scratch;
  Conflict c{};
  Answer e;
  std::memset(&e, 0, sizeof(e));
  if (firstConflictQuadratic(sol, c, scratch)) {
    e.w[0] = 1; e.w[1] = (uint32_t)c.time; e.w[2] = (uint32_t)c.agent1; e.w[3] = (uint32_t)c.agent2;
    e.w[4] = c.type == Conflict::Edge ? 1u : 0u;
    e.w[5] = (uint32_t)c.x1; e.w[6] = (uint32_t)c.y1;
    if (c.type == Conflict::Edge) { e.w[7] = (uint32_t)c.x2; e.w[8] = (uint32_t)c.y2; }
  }
  e.w[9] = (uint32_t)countConflictsQuadratic(sol, scratch);
  return e;
}

// a walk of `len` cells on a dim x dim grid: stay or move to a 4-neighbour
std::vector<uint16_t> walk(std::mt19937& rng, int dim, int len) {
  std::vector<uint16_t> p;
  int x = (int)(rng() % dim), y = (int)(rng() % dim);
  for (int k = 0; k < len; ++k) {
    p.push_back((uint16_t)(x | (y << 8)));
    static const int dx[5] = {0, 1, -1, 0, 0}, dy[5] = {0, 0, 0, 1, -1};
    const int m = (int)(rng() % 5), nx = x + dx[m], ny = y + dy[m];
    if (nx >= 0 && nx < dim && ny >= 0 && ny < dim) { x = nx; y = ny; }
  }
  return p;
}

struct Tally {
  long sets = 0, wideSets = 0, scans = 0, edgeFirst = 0, free_ = 0, bad = 0;  // sets: random nodes generated, not scans
  int64_t oob = 0;
};

void check(const Paths& S, uint32_t ag, const Answer& e, Tally& ty) {
  for (int lds = 0; lds < 2; ++lds) {
    const Answer a = runScan(S, ag, lds != 0, ty.oob);
    if (std::memcmp(a.w, e.w, sizeof(a.w)) != 0) {
      if (ty.bad++ < 5) {
        std::fprintf(stderr, "mismatch: %zu agents, agent %u, table %s\n  got ", S.size(), ag, lds ? "in LDS" : "in memory");
        for (uint32_t k = 0; k < mrp::ns::kOutWords; ++k) std::fprintf(stderr, " %u", a.w[k]);
        std::fprintf(stderr, "\n  want");
        for (uint32_t k = 0; k < mrp::ns::kOutWords; ++k) std::fprintf(stderr, " %u", e.w[k]);
        std::fprintf(stderr, "\n");
      }
    }
  }
  ty.scans += 2;
  ty.edgeFirst += e.w[0] && e.w[4];
  ty.free_ += e.w[0] == 0;
}

// one share of the work: its own generator, so the sets do not depend on how many threads run the shares
void shard(uint32_t seed, long nSmall, long nWide, Tally& ty) {
  std::mt19937 rng(seed);
  // small collision-rich sets: 1-12 agents on 2x2 .. 6x6 grids, path lengths 1-12; the replaced agent at every index, its
  // path as drawn, once the longest and once the shortest of the node
  while (ty.sets < nSmall) {
    const int n = 1 + (int)(rng() % 12), dim = 2 + (int)(rng() % 5);
    Paths S(n);
    int lo = 13, hi = 0;
    for (int a = 0; a < n; ++a) {
      S[a] = walk(rng, dim, 1 + (int)(rng() % 12));
      lo = std::min<int>(lo, (int)S[a].size());
      hi = std::max<int>(hi, (int)S[a].size());
    }
    const Answer e = expected(S);  // the node as drawn: one answer, whichever agent's path is called the new one
    for (int ag = 0; ag < n; ++ag) {
      check(S, (uint32_t)ag, e, ty);
      Paths L = S, Sh = S;
      L[ag] = walk(rng, dim, hi + 1 + (int)(rng() % 3));  // longer than every other path
      check(L, (uint32_t)ag, expected(L), ty);
      Sh[ag] = walk(rng, dim, lo > 1 ? lo - 1 : 1);        // no longer than any other path
      check(Sh, (uint32_t)ag, expected(Sh), ty);
    }
    ty.sets += 1;
  }
  // two and three lane chunks: 65-130 agents, the replaced agent at 0, 63, 64 and last
  while (ty.wideSets < nWide) {
    const int n = 65 + (int)(rng() % 66), dim = 8 + (int)(rng() % 25);
    Paths S(n);
    for (int a = 0; a < n; ++a) S[a] = walk(rng, dim, 1 + (int)(rng() % 24));
    const int at[4] = {0, 63, 64, n - 1};
    for (int q = 0; q < 4; ++q) {
      if (q & 1) S[at[q]] = walk(rng, dim, 25 + (int)(rng() % 50));  // (also past one 64-step block of the new path)
      check(S, (uint32_t)at[q], expected(S), ty);
    }
    ty.wideSets += 1;
  }
}

}  // namespace

int main() {
  // 100 000 small and 200 wide sets in 20 equal shares, run by up to 8 threads (the scans are independent of each other)
  constexpr int kShards = 20;
  constexpr long kSmallPerShard = 5000, kWidePerShard = 10;
  std::vector<Tally> part(kShards);
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int k = next.fetch_add(1); k < kShards; k = next.fetch_add(1)) shard(20240607u + (uint32_t)k, kSmallPerShard, kWidePerShard, part[k]);
  };
  const unsigned hw = std::thread::hardware_concurrency();
  std::vector<std::thread> pool;
  for (unsigned k = 1; k < std::min(8u, hw ? hw : 1u); ++k) pool.emplace_back(work);
  work();
  for (std::thread& th : pool) th.join();
  Tally ty;
  for (const Tally& q : part) {
    ty.sets += q.sets; ty.wideSets += q.wideSets; ty.scans += q.scans; ty.edgeFirst += q.edgeFirst; ty.free_ += q.free_;
    ty.bad += q.bad; ty.oob += q.oob;
  }
  if (ty.bad != 0 || ty.oob != 0 || ty.edgeFirst == 0 || ty.free_ == 0) {
    std::fprintf(stderr, "FAILED: %ld mismatches, %lld out-of-window LDS accesses, %ld edge-first sets, %ld conflict-free sets\n",
                 ty.bad, (long long)ty.oob, ty.edgeFirst, ty.free_);
    return 1;
  }
  std::printf("ok %ld sets (%ld small, %ld wide), %ld scans\n", ty.sets + ty.wideSets, ty.sets, ty.wideSets, ty.scans);
  return 0;
}
