// TEST INFRASTRUCTURE — the assignment wave program (libmultirobotplanning_amd/csrc/assign_wave.h, the code the gfx950
// kernel runs) compiled against the host interpretation of its wave vocabulary, behind the engine's own packer
// (host/assign_pack.h) and next-best series (host/assign_series.h).  A program of its own: built by
// tests/test_assign_emu_cpu.py with the host sanitizers, it reads records from stdin and writes results to stdout.
//
//   solve  nA nT minMatching hasMode hasForbidden  cost[nA*nT]  [mode[nA]]  [forbidden[nA]]
//   gsolve dimx dimy nA nT minMatching hasMode hasForbidden hasAllowed  table[nT][dimy*dimx]  starts[nA][2]
//          [allowed[nA]] [mode[nA]] [forbidden[nA]]        (the gather form over tables laid out as the engine lays them)
//   series nA nT cost[nA*nT]                                (the whole series, then two more calls)
// Every record answers with lines "R status matched cost task_of...", a series with "S <lines>" first; the last line is
// "OOB <reads> <writes>": the LDS accesses outside the window assign_layout.h computes.  Every staged area is a heap
// block of exactly its size, so AddressSanitizer sees an access past it.
#include <stdint.h>

#include <climits>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "wave_emu_assign.h"
#include "../../libmultirobotplanning_amd/csrc/assign_wave.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_pack.h"
#include "../../libmultirobotplanning_amd/csrc/host/assign_series.h"

using namespace mrp::host;

namespace {

uint64_t g_oobReads = 0, g_oobWrites = 0;

// what mrp_ll_assign_batch does, with the emulator in the kernel's place: one window per problem, as large as the launch's
int solveBatch(const PackEnv& env, const std::vector<uint32_t>& maps, int32_t n, const mrp_ll_assign_problem* problems,
               mrp_ll_assign_result* results) {
  AssignStaging st;
  packAssignBatch(env, n, problems, results, st);
  std::vector<uint32_t> out(st.outWords, 0xA5A5A5A5u);
  for (const mrp::as::AssignJob& job : st.jobs) {
    std::vector<uint8_t> mem(st.ldsBytes, 0xCD);
    wv::LdsWindow win{mem.data(), mrp::as::ldsBytes(job.nA), 0, 0};
    mrp::as::assignSolve(&win, maps.data(), st.data.data(), out.data(), job);
    g_oobReads += win.oobReads;
    g_oobWrites += win.oobWrites;
  }
  unpackAssignBatch(st, out.data(), results);
  return MRP_LL_SUCCESS;
}

void printResult(const mrp_ll_assign_result& r, int nA) {
  std::printf("R %d %d %lld", r.status, r.matched, (long long)r.cost);
  for (int a = 0; a < nA; ++a) std::printf(" %d", r.task_of[a]);
  std::printf("\n");
}

template <class T>
std::vector<T> readN(size_t n) {
  std::vector<T> v(n);
  for (T& x : v) std::cin >> x;
  return v;
}

}  // namespace

int main() {
  std::string kind;
  const PackEnv noEnv;
  const std::vector<uint32_t> noMaps(1, 0);
  while (std::cin >> kind) {
    if (kind == "solve") {
      int nA, nT, minM, hasMode, hasForb;
      std::cin >> nA >> nT >> minM >> hasMode >> hasForb;
      const size_t rows = nA > 0 ? nA : 0, cols = nT > 0 ? nT : 0;
      const std::vector<int32_t> cost = readN<int32_t>(rows * cols);
      const std::vector<int32_t> mode = readN<int32_t>(hasMode ? rows : 0);
      const std::vector<uint64_t> forb = readN<uint64_t>(hasForb ? rows : 0);
      std::vector<int32_t> taskOf(rows + 1, -7);
      static const int32_t none = 0;
      mrp_ll_assign_problem p{nA, nT, cost.empty() ? &none : cost.data(), nullptr, nullptr, nullptr,
                              hasForb ? forb.data() : nullptr, hasMode ? mode.data() : nullptr, minM};
      mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
      solveBatch(noEnv, noMaps, 1, &p, &r);
      printResult(r, (int)std::min<size_t>(rows, 64));
    } else if (kind == "gsolve") {
      int dimx, dimy, nA, nT, minM, hasMode, hasForb, hasAllowed;
      std::cin >> dimx >> dimy >> nA >> nT >> minM >> hasMode >> hasForb >> hasAllowed;
      PackEnv env;
      env.maps.push_back(MapRec{dimx, dimy, (uint32_t)(dimx * dimy + 31) / 32, 0});
      const MapRec& mp = env.maps[0];
      std::vector<uint32_t> maps(32, 0xA5A5A5A5u);  // tables on their own 128-byte lines, exactly their words
      std::vector<int32_t> ids;
      for (int t = 0; t < nT; ++t) {
        const std::vector<int32_t> dist = readN<int32_t>((size_t)dimx * dimy);
        const uint32_t off = (uint32_t)maps.size();
        maps.resize(maps.size() + heurTableWords(mp), 0xFFFFFFFFu);
        uint16_t* t16 = reinterpret_cast<uint16_t*>(maps.data() + off);
        for (int y = 0; y < dimy; ++y)
          for (int x = 0; x < dimx; ++x) {
            const int32_t v = dist[y * dimx + x];
            t16[y * heurStride(mp) + x] = (v < 0 || v > 0xFFFE) ? 0xFFFFu : (uint16_t)v;
          }
        while (maps.size() & 31u) maps.push_back(0xA5A5A5A5u);
        env.heurs.push_back(HeurRec{0, off});
        ids.push_back(t);
      }
      const std::vector<int32_t> starts = readN<int32_t>(2 * (size_t)nA);
      const std::vector<uint64_t> allowed = readN<uint64_t>(hasAllowed ? nA : 0);
      const std::vector<int32_t> mode = readN<int32_t>(hasMode ? nA : 0);
      const std::vector<uint64_t> forb = readN<uint64_t>(hasForb ? nA : 0);
      std::vector<int32_t> taskOf((size_t)nA + 1, -7);
      mrp_ll_assign_problem p{nA, nT, nullptr, ids.data(), starts.data(), hasAllowed ? allowed.data() : nullptr,
                              hasForb ? forb.data() : nullptr, hasMode ? mode.data() : nullptr, minM};
      mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
      solveBatch(env, maps, 1, &p, &r);
      printResult(r, nA);
    } else if (kind == "series") {
      int nA, nT;
      std::cin >> nA >> nT;
      const std::vector<int32_t> cost = readN<int32_t>((size_t)nA * nT);
      static const int32_t none = 0;
      mrp_ll_assign_problem p{nA, nT, cost.empty() ? &none : cost.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0};
      const AssignSolveFn solve = [&](int32_t n, const mrp_ll_assign_problem* ps, mrp_ll_assign_result* rs) {
        return solveBatch(noEnv, noMaps, n, ps, rs);
      };
      mrp_ll_assign_series* s = nullptr;
      if (assignSeriesCreate(nullptr, 1, &p, &s, solve) != MRP_LL_SUCCESS) {
        std::printf("S 0\n");
        continue;
      }
      std::vector<std::string> lines;
      std::vector<int32_t> taskOf((size_t)nA + 1, -7);
      for (int after = 0; after < 3;) {
        mrp_ll_assign_result r{0, 0, 0, taskOf.data()};
        if (assignSeriesNext(1, &s, &r, solve) != MRP_LL_SUCCESS) break;
        if (r.status != MRP_LL_OK) ++after;  // exhausted: ask twice more
        std::string line = "R " + std::to_string(r.status) + " " + std::to_string(r.matched) + " " + std::to_string(r.cost);
        for (int a = 0; a < nA; ++a) line += " " + std::to_string(taskOf[a]);
        lines.push_back(line);
      }
      std::printf("S %zu\n", lines.size());
      for (const std::string& l : lines) std::printf("%s\n", l.c_str());
      delete s;
    } else {
      std::fprintf(stderr, "emu_assign: unknown record \"%s\"\n", kind.c_str());
      return 2;
    }
  }
  std::printf("OOB %llu %llu\n", (unsigned long long)g_oobReads, (unsigned long long)g_oobWrites);
  return 0;
}
